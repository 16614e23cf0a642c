"""The matrix-free Hubbard sector operator (qbh_mf_hubbard_repr: k_mf_sector, k_mf_sector_orb, k_sec_remainder, k_sec_reduce) and the
generator it shares its rows with (qbh_gen_hubbard_repr), element by element against an independent host assembly
(tests/secforms.py, itself checked on the CPU against Psi^H O Psi in tests/test_secforms.py).

Cases (cu = up patterns per regular block) and what each reaches:

  * 4x2, 4+4, all 8 k, cu 70: the size of the dense projection; 7 regular + 5 stabilised blocks, w_up 12, at most 6 down hops;
    amplitudes -t and -2t (the torus lists its y bonds twice);
  * 4x3, 4+3, cu 495: j = 1 with a partial last wavefront (495 = 256 + 3*64 + 47); w_up 16 = two full rounds of 8; up to 12 down
    hops (second round, partial); 18 regular + 1 stabilised block, 2 regular blocks with remainder entries; two items per block
    under sec_tile=256;
  * 4x4, 4+2, cu 1820: two items per block at the default tile (1024 + 796, 796 = 3*256 + 28); exactly 8 down hops (one full
    round); 6 regular + 3 stabilised blocks, 4 regular blocks with remainder entries; 13,692 rows per momentum;
  * 4x4, 5+2, cu 4368: five items per block, the last 272 rows; w_up 20 (three rounds, the last partial); 32,760 rows;
  * 13x1, 6+2, cu 1716: prime length: no stabilised block, an empty remainder (its launch is skipped); two items per block;
  * ring of 10 with its dihedral group (20 elements), 4+3, cu 210: a non-commuting group in the orbit order, several stabiliser
    kinds.

Momenta: one with real characters first, one genuinely complex last (the ring: its trivial and its sign representation).  Variants
on 4x3 and 4x4 with 4+2: plain; anisotropic (t_y = 0.7: a second up amplitude, the ext slots of utab / uext) and extended
(density-density pairs, uniform number terms: has_number_terms); a Peierls phase on the down species' x hops (the ci path with an
amplitude that is complex by itself).  tests/test_secforms.py asserts all of this from the mirror.

Checks, all within the bounds derived in tests/secforms.py (|y_i - ref_i| <= (terms_i + 8) eps S_i over the UNMERGED terms of the
row, csrforms.epilogue's bounds for the reductions); |x_j| >= 0.5 and |a| >= 0.1, so a dropped, doubled, mis-signed or misplaced
term is far outside.  A failure names the worst row as (block's down pattern, up pattern, item, row inside the item), its term count
and error / bound.

  1. the generator's stored operator against the host assembly: the same structure, every value within (m + 5) eps;
  2. qbh_spmv_dev on complex vectors in both row orders, five (alpha, beta, gamma), y = NaN where beta = 0, both reductions;
     three calls bit-identical, y the same without the reductions;
  3. the vector seams of the orbit order: to_internal / from_internal exact and inverse, MultMv, randomize;
  4. the real forms through the Lanczos continuation probe of test_gpu_realforms.py, three drivers, both row orders, at every
     momentum with real characters (4x2: four of the eight) and every variant with real amplitudes;
  5. launch geometry (QBH_DEBUG sec_tile, sec_grid, sec_walk): every y and both reductions bit for bit the default's;
  6. the other unroll instances (sec_unroll = 4 and 16) in child processes.

Largest error / bound seen on an MI355X (every test prints its own figure, pytest -s): 1. the generator 0.084 (4x4 with 4+2,
k = (1, 3), Peierls phase); 2. qbh_spmv_dev 0.085 (4x2, k = (0, 1), both row orders); 3. MultMv 0.059 (13x1); 4. the real forms 0.16
of test_gpu_realforms' (terms_i + 8) eps (4x4 with 4+2, k = (0, 0), anisotropic, both row orders; the 4x2 momenta with characters
-1 reach 0.105); 5. every knob bit for bit; 6. sec_unroll 4: 0.068 (complex x) and 0.16 (real x), sec_unroll 16: 0.16; all 176 arrays
of the children bit-identical to the default instance.  The whole file (158 tests) takes 17 s on the MI355X; the slowest test is a
child-process test (3.4 s, mostly the child's start), every other test takes under 0.4 s.
"""
import os
import subprocess
import sys
import tempfile
from functools import lru_cache

import numpy as np
import pytest

import kronsum
import secforms as sf
import quantum_basis_amd as q
from quantum_basis_amd import _lib
from test_gpu_kronforms import TRIPLES
from test_gpu_realforms import B1, C_SLACK, MAXIT, _check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = sf.CL
DRIVERS = ("real", "cplx7", "cplx3")
LAST = {c: len(s["ks"]) - 1 for c, s in sf.CASES.items()}           # the complex momentum (the ring: the sign representation)


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _stored(case, ik, variant):
    spec, op = sf.CASES[case], sf.operator(case, variant)
    perms, chars = sf.symmetry(case, ik)
    return q.csr_mat.hubbard_repr(op["n"], spec["nu"], spec["nd"], None, perms, chars, U=op["U"], terms=op["terms"], pairs=op["pairs"],
                                  opts=q.make_opts(value_dict=0))


def _mf(case, ik, variant, orbit, **opts):
    spec, op = sf.CASES[case], sf.operator(case, variant)
    perms, chars = sf.symmetry(case, ik)
    M = q.csr_mat.hubbard_repr_mf(op["n"], spec["nu"], spec["nd"], None, perms, chars, U=op["U"], terms=op["terms"], pairs=op["pairs"],
                                  opts=q.make_opts(sector_orbit=orbit, **opts))
    assert M.info().kernel == _lib.KERNEL_MATRIX_FREE
    assert M.info().basis_internal == (_lib.BASIS_SECTOR_ORBIT if orbit else 0), "the operator did not take the row order asked for"
    return M


class _Ref:
    """Host reference of one (case, momentum, variant): the sector, its block mirror, the probe vectors and the five epilogues."""

    def __init__(self, case, ik, variant):
        self.key = (case, ik, variant)
        self.sec = sf.sector(case, ik, variant)
        self.b = sf.blocks(self.sec)
        dim = self.sec.dim
        self.x, self.y0 = sf.probe_vector(dim, 1), sf.probe_vector(dim, 2)
        self.nan = np.full(dim, np.nan + 1j * np.nan)
        sums = sf.row_sums(self.sec, self.x)
        self.refs = [sf.reference(self.sec, sums, self.x, self.y0, a, b, g) for a, b, g in TRIPLES]


@lru_cache(maxsize=None)
def _ref(case, ik, variant):
    return _Ref(case, ik, variant)


def _caller_rows(M, dim):
    """inv[p] = the caller's row held at position p of the operator's own order (exact: small integers pushed through the seams)."""
    v = M.vec(2)
    try:
        v.upload(np.arange(dim, dtype=np.float64).astype(np.complex128), 0)      # device: internal order
        M.to_internal(v.at(dim), v.at(0))                                         # read as the caller's order once more
        M.sync()
        inv = v.download(dim, dim).real.astype(np.int64)
    finally:
        v.free()
    assert np.array_equal(np.sort(inv), np.arange(dim))
    return inv


def _name(M, R, i, tile=sf.TILE):
    """Row i of the caller's order by block, up pattern, work item and row inside the item of operator M (its own row order)."""
    pos = np.argsort(_caller_rows(M, R.sec.dim))              # the identity for the ascending order
    b = R.b if tile == sf.TILE else sf.blocks(R.sec, tile)
    return sf.name_row(R.sec, b, i, internal=int(pos[i]))


def _name_fresh(R, i, orbit, tile=sf.TILE):
    """_name with an operator created for it: the row order does not depend on the process or on the debug knobs."""
    M = _mf(*R.key, orbit)
    try:
        return _name(M, R, i, tile)
    finally:
        M.destroy()


def _check_rows(what, M, R, y, ref, tile=sf.TILE):
    """M: the operator that produced y."""
    i, ratio, over, err = sf.worst(y, ref)
    if not ratio <= 1.0:
        raise AssertionError("%s: row %d = %s, %d terms: |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
            what, i, _name(M, R, i, tile), int(R.sec.terms_row[i]), err, float(ref["bound"][i]), ratio, over))
    return ratio


def _check_red(what, dot, nrm, ref):
    d = abs(complex(dot) - complex(ref["dot"]))
    assert d <= float(ref["t_dot"]), "%s: <x, y> = %r, reference %r (|diff| %.3e > %.3e)" % (what, dot, complex(ref["dot"]), d,
                                                                                            float(ref["t_dot"]))
    d = abs(nrm - float(ref["nrm"]))
    assert d <= float(ref["t_nrm"]), "%s: |y|^2 = %r, reference %r (|diff| %.3e > %.3e)" % (what, nrm, float(ref["nrm"]), d,
                                                                                           float(ref["t_nrm"]))


def _sweep(what, M, R, repeat=True, tile=sf.TILE):
    """The five triples: rows and reductions within their bounds, y = NaN on the way in where beta = 0; at the third triple three
    calls bit-identical in y and in the reductions and y the same without the reductions.  -> ([(y, dot, nrm)], largest ratio)."""
    dim = R.sec.dim
    assert M.dim == dim
    v = M.vec(2)
    out, top = [], 0.0
    try:
        v.upload(R.x, 0)
        for t, (alpha, beta, gamma) in enumerate(TRIPLES):
            yin = R.nan if beta == 0.0 else R.y0

            def run(red):
                v.upload(yin, dim)
                r = M.spmv(v.at(0), v.at(dim), alpha, beta, gamma, want_red=red)
                return v.download(dim, dim), r
            y, (dot, nrm) = run(True)
            tag = "%s (alpha, beta, gamma) = %r" % (what, (alpha, beta, gamma))
            top = max(top, _check_rows(tag, M, R, y, R.refs[t], tile))
            _check_red(tag, dot, nrm, R.refs[t])
            if t == 2 and repeat:
                for _ in range(2):
                    y2, (dot2, nrm2) = run(True)
                    assert np.array_equal(_bits(y2), _bits(y)), "%s: y differs between calls" % tag
                    assert (dot2, nrm2) == (dot, nrm), "%s: reductions differ between calls: %r, %r" % (tag, (dot, nrm), (dot2, nrm2))
                y3, _ = run(False)
                assert np.array_equal(_bits(y3), _bits(y)), "%s: y differs without the reductions" % tag
            out.append((y, dot, nrm))
    finally:
        v.free()
    return out, top


# ------------------------------------------------------------------------------------- 1. generator against assembly --
@pytest.mark.parametrize("case,ik,variant", sf.all_keys())
def test_generator_against_the_host_assembly(case, ik, variant):
    """qbh_gen_hubbard_repr with value_dict = 0, downloaded: row pointers and columns identical to the host assembly's merged CSR,
    every value within (m + 5) eps of the sum of its m terms' moduli (secforms.value_bound)."""
    sec = _ref(case, ik, variant).sec
    A = _stored(case, ik, variant)
    try:
        assert A.info().ncols == sec.dim
        ia, ja, val = A.download()
    finally:
        A.destroy()
    assert np.array_equal(ia, sec.ia), "row pointers differ, first at row %d" % int(np.nonzero(ia != sec.ia)[0][0] - 1)
    assert np.array_equal(ja.astype(np.int64), sec.ja), "columns differ, first at entry %d" % int(np.nonzero(ja != sec.ja)[0][0])
    err = np.abs(val.astype(CL) - sec.val)
    vb = sf.value_bound(sec)
    ratio = err / np.maximum(vb, sf.L(np.finfo(np.float64).tiny))
    p = int(np.argmax(ratio))
    row = int(np.searchsorted(sec.ia, p, side="right") - 1)
    assert ratio[p] <= 1.0, "entry %d (row %d, column %d, %d terms): %r, reference %r, error / bound %.3g; %d entries over" % (
        p, row, int(ja[p]), int(sec.val_terms[p]), val[p], complex(sec.val[p]), float(ratio[p]), int((ratio > 1).sum()))
    print("1. %s k %r %s: %d entries, largest error / bound %.3g" % (case, sf.CASES[case]["ks"][ik], variant, len(val), float(ratio[p])))


# ------------------------------------------------------------------------------------------------- 2. qbh_spmv_dev --
@pytest.mark.parametrize("orbit", [1, 0])
@pytest.mark.parametrize("case,ik,variant", sf.all_keys())
def test_spmv_every_row_and_both_reductions(case, ik, variant, orbit):
    R = _ref(case, ik, variant)
    what = "%s k %r %s sector_orbit %d" % (case, sf.CASES[case]["ks"][ik], variant, orbit)
    M = _mf(case, ik, variant, orbit)
    try:
        if not orbit:                                     # the tables the mirror predicts: blocks, items, w_up, remainder rows and entries
            assert M.info().bytes_matrix == sf.mf_bytes_ascending(R.sec, R.b), what
        _, top = _sweep(what, M, R)
    finally:
        M.destroy()
    print("2. %s: largest error / bound %.3g" % (what, top))


# ------------------------------------------------------------------------------------------------------ 3. the seams --
@pytest.mark.parametrize("case,variant", [(c, v) for c, s in sf.CASES.items() for v in s["variants"] if v != "peierls"])
def test_vector_seams_of_the_orbit_order(case, variant):
    """M keeps its device vectors orbit by orbit, M0 (sector_orbit = 0) moves bytes unchanged: through M0 the device memory of M's
    vectors is read as it is."""
    ik = LAST[case]
    R = _ref(case, ik, variant)
    dim = R.sec.dim
    M, M0 = _mf(case, ik, variant, 1), _mf(case, ik, variant, 0)
    v = q.DeviceVec(M0, 4 * dim)
    try:
        inv = _caller_rows(M, dim)
        assert not np.array_equal(inv, np.arange(dim)), "the orbit order is the ascending order: nothing is tested"
        # rows of a stabilised block keep their places; a regular block's rows move inside the block only
        blk = R.b.blk_of_row
        assert np.array_equal(blk[inv], blk) and np.array_equal(inv[~R.b.regular[blk]], np.nonzero(~R.b.regular[blk])[0])
        v.upload(R.x, 0)
        M0.sync()
        M.to_internal(v.at(dim), v.at(0))
        M.from_internal(v.at(2 * dim), v.at(dim))
        M.sync()
        xi, xb = v.download(dim, dim), v.download(2 * dim, dim)
        assert np.array_equal(_bits(xi), _bits(R.x[inv])), "to_internal is not the permutation the index vector went through"
        assert np.array_equal(_bits(xb), _bits(R.x)), "from_internal does not invert to_internal"
        w = M.vec(1)
        w.upload(R.x, 0)                                    # the host seam: the same permutation
        M.sync()
        M0.to_internal(v.at(3 * dim), w.at(0))              # a plain copy
        M0.sync()
        assert np.array_equal(_bits(v.download(3 * dim, dim)), _bits(xi)), "upload and to_internal disagree"
        assert np.array_equal(_bits(w.download(0, dim)), _bits(R.x))
        # randomize: the same stream by the caller's element number in both orders
        M.randomize(w.at(0), 9)
        M0.randomize(v.at(0), 9)
        r1, r0 = w.download(0, dim), v.download(0, dim)
        assert np.array_equal(_bits(r1), _bits(r0)) and abs(np.linalg.norm(r0) - 1.0) < 1e-12
        w.free()
        # MultMv on host vectors in the caller's order
        top = 0.0
        for op in (M, M0):
            y = np.full(dim, np.nan + 1j * np.nan)
            op.MultMv(R.x, y)
            top = max(top, _check_rows("%s %s MultMv sector_orbit %d" % (case, variant, op is M), op, R, y, R.refs[0]))
    finally:
        v.free()
        M.destroy()
        M0.destroy()
    print("3. %s %s: MultMv largest error / bound %.3g" % (case, variant, top))


# -------------------------------------------------------------------------------------------------- 4. the real forms --
def _probe_sector(M, raw, inv, x, z, b1, driver):
    """test_gpu_realforms._probe for an operator that may keep its device vectors in an order of its own (inv: _caller_rows, or
    None): the packed-double driver takes device memory as it is, so its vectors are permuted here and moved through `raw`, a
    handle that copies bytes unchanged.  -> (v2, a1, b2) in the caller's order."""
    n = M.dim
    hess = np.zeros(2 * MAXIT)
    hess[1] = b1
    n_real = M.stats().n_spmv_real
    if driver == "real":
        zi, xi = (z, x) if inv is None else (z[inv], x[inv])
        v = q.DeviceVec(raw, n)                               # 16 n bytes: two slots of n doubles
        v.upload(np.ascontiguousarray(np.concatenate([zi, xi])).view(np.complex128))
        raw.sync()
        m = q.lanczos_real(1, 1, MAXIT, M, v, hess, "dnmcs")
        M.sync()
        out = v.download().view(np.float64).copy()
        v.free()
        v2, xo = out[:n], out[n:]
        if inv is not None:
            a, b = np.empty(n), np.empty(n)
            a[inv], b[inv] = v2, xo
            v2, xo = a, b
    else:
        vv = np.zeros(2 * n, dtype=np.complex128)
        vv[:n], vv[n:] = z, x
        m = q.lanczos(1, 1, MAXIT, n, M, vv, hess, "dnmcs")
        assert not np.any(vv.imag[n:]) and not np.any(vv.imag[:n])
        v2, xo = vv.real[:n].copy(), vv.real[n:].copy()
    assert m == 2
    assert np.array_equal(xo, x)                              # the step leaves its x in place
    assert M.stats().n_spmv_real > n_real, "%s: the SpMV did not run the all-real form" % driver
    return v2, hess[MAXIT + 1], hess[2]


def _real_probes(case, ik, variant, orbit, drivers=DRIVERS):
    """Every driver with z = 0, b1 = 0 and with a random z, b1 = 1.3: {(driver, with z): (v2, a1, b2)}."""
    out = {}
    raw = _mf(case, ik, variant, 0, real_forms=7)
    ops = {7: raw} if not orbit else {}
    try:
        n = raw.dim
        x, zr = kronsum.probe_vector(n, 21), kronsum.probe_vector(n, 1021)
        inv = None
        for drv in drivers:
            rf = 3 if drv == "cplx3" else 7
            if rf not in ops:
                ops[rf] = _mf(case, ik, variant, orbit, real_forms=rf)
            if orbit and inv is None:
                inv = _caller_rows(ops[rf], n)
            for beta in (False, True):
                z, b1 = (zr, B1) if beta else (np.zeros(n), 0.0)
                out[(drv, beta)] = _probe_sector(ops[rf], raw, inv, x, z, b1, drv)
    finally:
        for A in set(list(ops.values()) + [raw]):
            A.destroy()
    return out, x, zr


def _check_real(what, sec, out, x, zr):
    assert not np.any(sec.t_val.imag), "%s: the operator is not real" % what
    ref_csr = (sec.t_ia, sec.t_ja, sec.t_val.real)            # the unmerged terms: nnz_i of the bound is terms_i
    top = 0.0
    for (drv, beta), (v2, a1, b2) in out.items():
        z, b1 = (zr, B1) if beta else (np.zeros(len(x)), 0.0)
        recon = _check("%s [%s, b1 = %g]" % (what, drv, b1), ref_csr, x, z, b1, v2, a1, b2)
        # the figure _check asserts on, for the record: |recon - ref| / ((terms_i + C_SLACK) eps scale_i)
        ref, absref = kronsum.row_sums(*ref_csr, x)
        scale = absref + np.abs(sf.L(a1) * x.astype(sf.L)) + np.abs(sf.L(b1) * z.astype(sf.L))
        top = max(top, float(np.max(np.abs(recon - ref) / ((sec.terms_row + C_SLACK) * sf.L(sf.EPS) * scale))))
    return top


# every momentum with real characters (tests/test_secforms.py pins how many each case has) x every variant with real amplitudes
REAL_KEYS = [(c, ik, v) for (c, ik, v) in sf.all_keys() if v != "peierls" and sf.has_real_characters(c, ik)]


@pytest.mark.parametrize("orbit", [1, 0])
@pytest.mark.parametrize("case,ik,variant", REAL_KEYS)
def test_real_forms_through_the_lanczos_probe(case, ik, variant, orbit):
    """(H x)_i = b2 v2_i + a1 x_i + b1 z_i from one continuation step: packed doubles throughout (y_re), complex vectors with
    real_forms 7 and with real_forms 3 (8-byte x gathers, complex y), with and without b1 z; n_spmv_real must advance."""
    sec = _ref(case, ik, variant).sec
    what = "%s k %r %s sector_orbit %d" % (case, sf.CASES[case]["ks"][ik], variant, orbit)
    out, x, zr = _real_probes(case, ik, variant, orbit)
    top = _check_real(what, sec, out, x, zr)
    print("4. %s: three drivers, with and without b1 z: largest error / bound %.3g" % (what, top))


# ----------------------------------------------------------------------------------------------- 5. launch geometry --
WALKS = ["sec_walk=0", "sec_walk=1"]
KNOBS = ["sec_tile=256", "sec_tile=512", "sec_tile=2048"] + WALKS + ["sec_grid=%d,%s" % (g, w) for g in (8, 16) for w in WALKS]
KNOBS_4X3 = ["sec_grid=8,sec_tile=256,%s" % w for w in WALKS]


def _tile_of(knob):
    for part in knob.split(","):
        if part.startswith("sec_tile="):
            return int(part[9:])
    return sf.TILE


@pytest.mark.parametrize("orbit", [1, 0])
@pytest.mark.parametrize("case,variant", [(c, v) for c, s in sf.CASES.items() for v in s["variants"]])
def test_launch_geometry_bit_for_bit(case, variant, orbit, monkeypatch):
    """A row's sum is formed in the same order whatever item or workgroup takes it and k_sec_reduce depends on none of the knobs:
    every y and both reductions equal the default's bit for bit.  sec_grid = 8 / 16: one or two workgroups per XCD, so every
    workgroup walks several items and reloads its hop table per item, under the static assignment and under the ordered walk."""
    ik = LAST[case]
    R = _ref(case, ik, variant)
    what = "%s k %r %s sector_orbit %d" % (case, sf.CASES[case]["ks"][ik], variant, orbit)
    monkeypatch.delenv("QBH_DEBUG", raising=False)
    M = _mf(case, ik, variant, orbit)
    try:
        base, top = _sweep(what, M, R, repeat=False)
    finally:
        M.destroy()
    knobs = KNOBS + (KNOBS_4X3 if case == "4x3_4+3" else [])
    for knob in knobs:
        tile = _tile_of(knob)
        n_items = sf.blocks(R.sec, tile).n_items
        if "sec_grid=8" in knob and case != "ring10_4+3":
            assert n_items > 8, "%s: no workgroup of a grid of 8 takes a second item" % what
        if knob in KNOBS_4X3:
            assert n_items >= 2 * 18
        monkeypatch.setenv("QBH_DEBUG", knob)               # read when the operator is created (tile, walk) and at every launch (grid)
        M = _mf(case, ik, variant, orbit)
        try:
            if not orbit:                                   # the knob was read: the item list is the one of this tile
                assert M.info().bytes_matrix == sf.mf_bytes_ascending(R.sec, sf.blocks(R.sec, tile)), "%s %s" % (what, knob)
            got, _ = _sweep("%s %s" % (what, knob), M, R, repeat=False, tile=tile)
        finally:
            M.destroy()
            monkeypatch.delenv("QBH_DEBUG")
        for t, ((y, dot, nrm), (yb, dotb, nrmb)) in enumerate(zip(got, base)):
            diff = np.nonzero((_bits(y).reshape(-1, 2) != _bits(yb).reshape(-1, 2)).any(axis=1))[0]
            assert len(diff) == 0, "%s %s, triple %d: %d rows differ from the default in the last bits, first %d = %s: %r against %r" % (
                what, knob, t, len(diff), diff[0], _name_fresh(R, int(diff[0]), orbit, tile), y[diff[0]], yb[diff[0]])
            assert (dot, nrm) == (dotb, nrmb), "%s %s, triple %d: reductions %r, default %r" % (what, knob, t, (dot, nrm), (dotb, nrmb))
    print("5. %s: %d knobs bit for bit; default largest error / bound %.3g" % (what, len(knobs), top))


# ------------------------------------------------------------------------------------- 6. the other unroll instances --
CHILD_CASES = ("4x3_4+3", "4x4_4+2")
CHILD_COMPLEX = ("plain", "peierls")         # at the complex momentum
CHILD_REAL = ("plain", "aniso")              # at k = (0, 0)


def _child_jobs(unroll):
    """launch_mf_sector's instances: unroll 4 exists for both kernels and both x; unroll 16 only for the ascending order with real x."""
    cplx = [(c, v, o) for c in CHILD_CASES for v in CHILD_COMPLEX for o in (1, 0)] if unroll == 4 else []
    real = [(c, v, o) for c in CHILD_CASES for v in CHILD_REAL for o in ((1, 0) if unroll == 4 else (0,))]
    return cplx, real


def _child_compute(unroll, cplx, real):
    """{name: array} of the products and probes of _child_jobs, with whatever sec_unroll the process runs under."""
    out = {}
    for (case, variant, orbit) in cplx:
        M = _mf(case, LAST[case], variant, orbit)
        dim = M.dim
        x, y0 = sf.probe_vector(dim, 1), sf.probe_vector(dim, 2)
        v = M.vec(2)
        v.upload(x, 0)
        for t, (alpha, beta, gamma) in enumerate(TRIPLES):
            v.upload(np.full(dim, np.nan + 1j * np.nan) if beta == 0.0 else y0, dim)
            dot, nrm = M.spmv(v.at(0), v.at(dim), alpha, beta, gamma, want_red=True)
            out["y~%s~%s~%d~%d" % (case, variant, orbit, t)] = v.download(dim, dim)
            out["red~%s~%s~%d~%d" % (case, variant, orbit, t)] = np.array([dot.real, dot.imag, nrm])
        v.free()
        M.destroy()
    for (case, variant, orbit) in real:
        probes, x, zr = _real_probes(case, 0, variant, orbit, drivers=("real", "cplx3"))
        for (drv, beta), (v2, a1, b2) in probes.items():
            out["v2~%s~%s~%d~%s~%d" % (case, variant, orbit, drv, beta)] = v2
            out["ab~%s~%s~%d~%s~%d" % (case, variant, orbit, drv, beta)] = np.array([a1, b2])
    return out


@pytest.mark.parametrize("unroll", [4, 16])
def test_other_unroll_instances_in_a_child_process(unroll):
    """launch_mf_sector latches sec_unroll on first use, so another value needs a fresh process.  The child writes its results to a
    temporary file; they are held to the same references and bounds.  Bit equality with this process's default instance (unroll 8)
    is reported, not required: another unroll is another instantiation."""
    cplx, real = _child_jobs(unroll)
    env = dict(os.environ, QBH_DEBUG="sec_unroll=%d" % unroll,
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "child.npz")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(unroll), path], capture_output=True, text=True, env=env,
                           cwd=ROOT, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        got = dict(np.load(path))
    mine = _child_compute(8, cplx, real)
    assert set(mine) == set(got)
    same = sum(1 for k in got if np.array_equal(_bits(got[k]), _bits(mine[k])))
    top, top_real = 0.0, 0.0
    for (case, variant, orbit) in cplx:
        R = _ref(case, LAST[case], variant)
        for t in range(len(TRIPLES)):
            what = "sec_unroll %d %s %s sector_orbit %d %r" % (unroll, case, variant, orbit, TRIPLES[t])
            y, red = got["y~%s~%s~%d~%d" % (case, variant, orbit, t)], got["red~%s~%s~%d~%d" % (case, variant, orbit, t)]
            i, ratio, over, err = sf.worst(y, R.refs[t])
            assert ratio <= 1.0, "%s: row %d = %s, %d terms: |y - ref| = %.3e, error / bound %.3g; %d rows over" % (
                what, i, _name_fresh(R, i, orbit), int(R.sec.terms_row[i]), err, ratio, over)
            _check_red(what, complex(red[0], red[1]), float(red[2]), R.refs[t])
            top = max(top, ratio)
    for (case, variant, orbit) in real:
        sec = _ref(case, 0, variant).sec
        n = sec.dim
        x, zr = kronsum.probe_vector(n, 21), kronsum.probe_vector(n, 1021)
        out = {}
        for drv in ("real", "cplx3"):
            for beta in (0, 1):
                ab = got["ab~%s~%s~%d~%s~%d" % (case, variant, orbit, drv, beta)]
                out[(drv, bool(beta))] = (got["v2~%s~%s~%d~%s~%d" % (case, variant, orbit, drv, beta)], float(ab[0]), float(ab[1]))
        top_real = max(top_real, _check_real("sec_unroll %d %s %s sector_orbit %d" % (unroll, case, variant, orbit), sec, out, x, zr))
    print("6. sec_unroll %d: %d complex jobs, largest error / bound %.3g; %d real jobs, %.3g; %d of %d arrays bit-identical to unroll 8" % (
        unroll, len(cplx), top, len(real), top_real, same, len(got)))


if __name__ == "__main__":                                  # the child of test_other_unroll_instances_in_a_child_process
    _unroll, _path = int(sys.argv[1]), sys.argv[2]
    assert os.environ.get("QBH_DEBUG") == "sec_unroll=%d" % _unroll
    np.savez(_path, **_child_compute(_unroll, *_child_jobs(_unroll)))
