"""The d-level family of qbh_qudit.hip row by row: the generator qbh_gen_qudit (k_qudit_count, k_qudit_fill) entry by entry and the
operator applied without a stored matrix (qbh_mf_qudit: the four instances k_mf_qudit<REALX, TLDS>, k_mf_qudit_count) element by
element, against the host reference of tests/quditforms.py (no library code; pinned on the CPU by tests/test_quditforms.py, which
also asserts every case's edge on the reference alone and shows the comparison rejecting single faults).

Cases (quditforms.CASES) and the branch each reaches:

  * (2, 64, 63), (2, 64, 1), dim 64: words with bit 63; qd_charge's unmasked nb == 64 branch (pairs ending at site 63);
  * (2, 64, 63) with 239 pairs: max_row 240, the fill kernel's 155,648 B of LDS; the real drivers on 64-bit words;
  * (2, 64, 3), dim 41,664: 64-bit words over many workgroups of every kernel;
  * (3, 32, 2 | 62), (4, 32, 2 | 94), dim 528: 64-bit words of 2-bit fields, the unused code 3, both ends of the charge range,
    level 3 at site 31 (bit 63);
  * (6 | 7 | 8, 21, 3), dim 1771, (8, 21, 145), dim 231: 3-bit fields, 63-bit words, the top sites full;
  * (8, 7, 12), (7, 8, 10), (6, 9, 9), dim 17,094 / 18,488 / 22,825: d = 6, 7, 8 at the generator, pairs (0, n-1), (0, 1), (n-2, n-1)
    and drawn ones, about half of them handed over as (j, i);
  * (8, 12, 5) with 34 full pairs: max_row 239 from 7-entry class rows; 34 classes, tables in global memory;
  * (2, 32, 16), the 4096 rows around the alternating word of 601,080,390, 239 even-odd pairs: rows of up to 240 entries (51 of 200
    and more, none below 100): the insertion sort at full depth.  Its x (9.6 GB) is drawn on the device;
  * (8, 12, 5) with 15 and with 16 classes of maxk 7, complex and real: 145,600 and 155,072 B against the 153,600 B budget: TLDS on
    and off one class apart, for both REALX;
  * (8, 5, 0), (8, 5, 35): dimension 1;  (3, 15, 15), dim 1,787,607: the grid-stride loop and its tail, one epilogue;
  * the slot list on (4, 6, 9), dim 580: a diagonal pair beside others (maxk = 0, slot base 0), a diagonal-only operator, three pairs
    sharing one class, a repeated pair with one element cancelling exactly (nnz drops), no single-site term (has_single = 0);
    padding slots occur in most cases and none in four.

Checks.  1. generator: pointers and columns exactly, off-diagonal values by bits, the diagonal within (n + n_pairs + 2) eps
sum |terms|; whole and as shards (first row, last row, 63 / 64 / 65 rows, across a 64-row fill block).  2. matrix-free on complex x:
every row within (terms_i + 8) eps S_i over the UNMERGED terms, both reductions within csrforms.epilogue's bounds, five (alpha, beta,
gamma) with y = NaN where beta = 0, three calls bit-identical, y the same without the reductions, guard zones around y intact, x
unchanged; info's kron_table_kernel, bytes_matrix and nnz equal to the mirror's.  3. real amplitudes through the three real drivers
(test_gpu_realforms' Lanczos probe).  4. ragged row shards bit for bit against the whole operator.  5. deep rows without a vector:
nnz of 4096 rows from unrank and the classes' row lengths.  6. the coverage gate.

Largest error / bound seen on an MI355X (every test prints its own figure, pytest -s; the gate prints the table):
k_mf_qudit<REALX 0, TLDS 1> 0.050 (the diagonal-only operator; 0.043 with off-diagonal slots, slots_diagonal_class; the 1,787,607-row
case 0.039), <REALX 0, TLDS 0> 0.022 (16 classes), <REALX 1, TLDS 1> 0.081 of test_gpu_realforms' (terms_i + 8) eps (diagonal-only; 0.055
slots_no_singles), <REALX 1, TLDS 0> 0.019 (16 real classes); the generator's diagonal 0.090 of (n + n_pairs + 2) eps sum |terms|
(slots_diagonal_class); every pointer, column and off-diagonal value exact.  No fault was found in the library.
The whole file (82 tests) takes 12 s on the MI355X; the slowest test is the 1,787,607-row case (3.2 s, of which the host reference is
most), then the generator at max_row 239 (0.7 s) and on the alternating shard (0.5 s); every other test takes under 0.4 s.
"""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest

import quditforms as qf
import quantum_basis_amd as q
from quantum_basis_amd import _lib
from test_gpu_kronforms import TRIPLES
from test_gpu_realforms import B1, C_SLACK, DRIVERS, _check, _probe
import kronsum

pytestmark = pytest.mark.gpu

PLAIN = dict(kron_split=0, sector_cut=-1, value_dict=0, real_fast_path=0)
GUARD = 64
SENTINEL = complex(7.25, -3.5)
GEN_CASES = [n for n, c in qf.CASES.items() if c["gen"]]
MF_CASES = list(qf.CASES)
DRIVER_CASES = [n for n, c in qf.CASES.items() if c["real"] and c["rows"] is None and c["dim"] <= 50_000]
SHARD_CASES = ["d2_n64_q63_239pairs", "d2_n64_q3", "d3_n32_q62", "d4_n32_q94", "d8_n21_q145", "d6_n9_q9", "d8_n12_q5_16cls", "d8_n5_q0"]
TOP = {}                    # (kernel, instance) -> (largest error / bound, case)


def _note(key, ratio, name):
    if ratio >= TOP.get(key, (-1.0, ""))[0]:
        TOP[key] = (ratio, name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _args(name):
    c = qf.CASES[name]
    pairs, sg = qf.operator(name)
    return c["n"], c["d"], c["total"], pairs, sg


def _gen(name, rows):
    return q.csr_mat.qudit(*_args(name), rows=rows, opts=q.make_opts(**PLAIN))


def _mf(name, rows=None, **opts):
    M = q.csr_mat.qudit(*_args(name), rows=rows, matrix_free=True, opts=q.make_opts(**opts) if opts else None)
    i = M.info()
    lay = qf.layout_of(name)
    assert i.kernel == _lib.KERNEL_MATRIX_FREE and i.ncols == qf.CASES[name]["dim"]
    assert i.kron_table_kernel == lay.tables_lds, "%s: tables in %s, the mirror says %s" % (name, i.kron_table_kernel, lay.tables_lds)
    assert i.bytes_matrix == lay.bytes_matrix, "%s: %d bytes held, the mirror says %d" % (name, i.bytes_matrix, lay.bytes_matrix)
    return M


def _triples(name):
    k = qf.CASES[name]["epilogues"]
    return list(TRIPLES) if k == 5 else [TRIPLES[0], TRIPLES[4]] if k == 2 else [TRIPLES[4]]


def _device_x(dim, seed):
    """0.5 <= |x_j| <= 1 with a random phase, drawn on the device (a vector too large to come from the host in a test)"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mod = torch.rand(dim, generator=g, device="cuda", dtype=torch.float64) * 0.5 + 0.5
    ph = torch.rand(dim, generator=g, device="cuda", dtype=torch.float64) * (2 * math.pi)
    x = torch.polar(mod, ph)
    del mod, ph
    torch.cuda.synchronize()
    return x


class _X:
    """The probe vector of a case on the device and, on the host, at the columns the case's rows touch."""

    def __init__(self, R, M):
        self.R, self.M, self.t, self.v = R, M, None, None
        if R.rows is None:
            self.v = q.DeviceVec(M, R.asm.dim)
            self.v.upload(R.x_host)
            self.ptr = self.v.ptr
        else:
            import torch
            self.t = _device_x(R.asm.dim, 1)
            self.idx = torch.from_numpy(R.need).cuda()
            self.ptr = C.c_void_p(self.t.data_ptr())

    def at_need(self):
        if self.t is None:
            return self.v.download()[self.R.need]
        import torch
        torch.cuda.synchronize()
        return self.t[self.idx].cpu().numpy()

    def free(self):
        if self.v is not None:
            self.v.free()
        if self.t is not None:
            import torch
            self.t = self.idx = None
            torch.cuda.empty_cache()


class _Ref:
    """Host reference of one case: the assembly, the mirror, the probe vectors and (on demand) the epilogues."""

    def __init__(self, name):
        self.name, self.c = name, qf.CASES[name]
        self.asm, self.lay = qf.reference_of(name), qf.layout_of(name)
        self.rows = qf.case_rows(name)
        self.need, self.jc, self.own = qf.compact_columns(self.asm)
        self.x_host = qf.probe_vector(self.asm.dim, 1) if self.rows is None else None
        self.y0 = qf.probe_vector(self.asm.nrows, 2)
        self.nan = np.full(self.asm.nrows, np.nan + 1j * np.nan)
        self.xc = self.sums = None
        self.refs = {}

    def bind(self, xc):
        """xc: x at self.need, as the device holds it"""
        if self.xc is None:
            self.xc = xc
            assert np.all(np.abs(xc) >= 0.5 - 1e-12) and np.all(np.abs(xc) <= 1 + 1e-12)
            self.sums = qf.row_sums(self.asm, xc, self.jc)
        assert np.array_equal(_bits(xc), _bits(self.xc))

    def ref(self, t):
        if t not in self.refs:
            self.refs[t] = qf.reference(self.asm, self.sums, self.xc[self.own], self.y0, *t)
        return self.refs[t]


@lru_cache(maxsize=None)
def _ref(name):
    return _Ref(name)


def _check_rows(what, R, y, ref):
    i, ratio, over, err = qf.worst(y, ref)
    if not ratio <= 1.0:
        raise AssertionError("%s: %s: |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
            what, qf.name_row(R.asm, i), err, float(ref["bound"][i]), ratio, over))
    return ratio


def _check_red(what, dot, nrm, ref):
    d = abs(complex(dot) - complex(ref["dot"]))
    assert d <= float(ref["t_dot"]), "%s: <x, y> = %r, reference %r (|diff| %.3e > %.3e)" % (what, dot, complex(ref["dot"]), d, float(ref["t_dot"]))
    d = abs(nrm - float(ref["nrm"]))
    assert d <= float(ref["t_nrm"]), "%s: |y|^2 = %r, reference %r (|diff| %.3e > %.3e)" % (what, nrm, float(ref["nrm"]), d, float(ref["t_nrm"]))


def _sweep(name, M, R, X):
    """Every triple of the case: rows and reductions within their bounds, y = NaN on the way in where beta = 0, guard zones around y;
    at the last triple three calls bit-identical in y and in the reductions and y the same without them.  -> largest error / bound"""
    m = R.asm.nrows
    assert M.dim == m
    R.bind(X.at_need())
    yv = q.DeviceVec(M, m + 2 * GUARD)
    guard = np.full(GUARD, SENTINEL)
    top, triples = 0.0, _triples(name)
    try:
        for k, t in enumerate(triples):
            alpha, beta, gamma = t
            yin = np.concatenate([guard, R.nan if beta == 0.0 else R.y0, guard])

            def run(red):
                yv.upload(yin)
                r = M.spmv(X.ptr, yv.at(GUARD), alpha, beta, gamma, want_red=red)
                out = yv.download()
                assert np.array_equal(_bits(out[:GUARD]), _bits(guard)) and np.array_equal(_bits(out[GUARD + m:]), _bits(guard)), \
                    "%s %r: the kernel wrote outside its rows" % (name, t)
                return out[GUARD:GUARD + m], r
            y, (dot, nrm) = run(True)
            tag = "%s (alpha, beta, gamma) = %r" % (name, t)
            top = max(top, _check_rows(tag, R, y, R.ref(t)))
            _check_red(tag, dot, nrm, R.ref(t))
            if k == len(triples) - 1:
                for _ in range(2):
                    y2, red2 = run(True)
                    assert np.array_equal(_bits(y2), _bits(y)), "%s: y differs between calls" % tag
                    assert red2 == (dot, nrm), "%s: reductions differ between calls: %r, %r" % (tag, (dot, nrm), red2)
                y3, _ = run(False)
                assert np.array_equal(_bits(y3), _bits(y)), "%s: y differs without the reductions" % tag
        assert np.array_equal(_bits(X.at_need()), _bits(R.xc)), "%s: x changed" % name
    finally:
        yv.free()
    return top


# ------------------------------------------------------------------------------------------------------ 1. generator --
@pytest.mark.parametrize("name", GEN_CASES)
def test_generator_entry_by_entry(name):
    R = _ref(name)
    asm = R.asm
    r0 = asm.r0
    A = _gen(name, R.rows)
    try:
        i = A.info()
        assert i.ncols == asm.dim and i.nrows == asm.nrows and i.row_offset == r0 and A.nnz == int(asm.ia[-1])
        top = qf.assert_same_csr(A.download(), asm)
    finally:
        A.destroy()
    shards = qf.gen_shards(asm.nrows)
    for what, (a, b) in shards.items():
        S = _gen(name, (r0 + a, r0 + b))
        try:
            got = S.download()
        finally:
            S.destroy()
        sub = qf.assemble(R.c["n"], R.c["d"], R.c["total"], *qf.operator(name), rows=(r0 + a, r0 + b), keep_terms=False)
        assert np.array_equal(sub.ja, asm.ja[asm.ia[a]:asm.ia[b]])
        top = max(top, qf.assert_same_csr(got, sub))
    _note(("k_qudit_fill", "diagonal"), top, name)
    print("1. %s: %d entries, longest row %d of max_row %d, fill LDS %d B, %d shards; diagonal error / bound %.3g" % (
        name, int(asm.ia[-1]), int(np.diff(asm.ia).max()), R.lay.max_row, qf.gen_fill_lds(R.lay.max_row, R.c["n"], R.c["total"] + 1),
        len(shards), top))


# ---------------------------------------------------------------------------------------- 2. matrix-free, complex x --
@pytest.mark.parametrize("name", MF_CASES)
def test_matrix_free_every_row_and_both_reductions(name):
    R = _ref(name)
    M = _mf(name, R.rows)
    X = _X(R, M)
    try:
        assert M.nnz == int(R.asm.ia[-1]), "%s: nnz %d, the reference has %d entries" % (name, M.nnz, int(R.asm.ia[-1]))
        top = _sweep(name, M, R, X)
        assert M.stats().n_spmv_real == 0
    finally:
        X.free()
        M.destroy()
        if not R.c["gen"]:                                 # too large to keep for the rest of the session
            _ref.cache_clear()
            qf.reference_of.cache_clear()
    inst = (False, bool(R.lay.tables_lds))
    _note(("k_mf_qudit", inst), top, name)
    print("2. %s: k_mf_qudit<REALX %d, TLDS %d>, %d classes, %d slots (%d padding), has_single %d: largest error / bound %.3g" % (
        name, inst[0], inst[1], R.lay.n_cls, R.lay.n_slots, R.lay.padding, R.lay.has_single, top))


def test_a_cancelled_element_drops_from_nnz():
    name = "slots_cancelled"
    n, d, total, pairs, sg = _args(name)
    both = _mf(name)
    once = q.csr_mat.qudit(n, d, total, pairs[:-1], sg, matrix_free=True)
    try:
        want_once = qf.assemble(n, d, total, pairs[:-1], sg, keep_terms=False)
        assert once.nnz == int(want_once.ia[-1]) and both.nnz == int(_ref(name).asm.ia[-1]) and both.nnz < once.nnz
    finally:
        both.destroy()
        once.destroy()


# --------------------------------------------------------------------------------------------- 3. the real drivers --
@pytest.mark.parametrize("name", DRIVER_CASES)
def test_real_amplitudes_through_the_three_real_drivers(name):
    """(H x)_i = b2 v2_i + a1 x_i + b1 z_i from one Lanczos continuation step (tests/test_gpu_realforms.py): packed doubles, complex
    vectors with real_forms 7 and with real_forms 3, with and without b1 z; the bound is test_gpu_realforms' (terms_i + 8) eps over the
    unmerged terms."""
    R = _ref(name)
    asm = R.asm
    ref_csr = (asm.t_ia, asm.t_ja, asm.t_val.real)
    n = asm.dim
    x, zr = kronsum.probe_vector(n, 21), kronsum.probe_vector(n, 1021)
    ref, absref = kronsum.row_sums(*ref_csr, x)
    top, ops = 0.0, {}
    try:
        for drv in DRIVERS:
            rf = 3 if drv == "cplx3" else 7
            if rf not in ops:
                ops[rf] = _mf(name, real_forms=rf)
            for beta in (False, True):
                z, b1 = (zr, B1) if beta else (np.zeros(n), 0.0)
                v2, a1, b2 = _probe(ops[rf], x, z, b1, drv)
                recon = _check("%s [%s, b1 = %g]" % (name, drv, b1), ref_csr, x, z, b1, v2, a1, b2)
                scale = absref + np.abs(qf.L(a1) * x.astype(qf.L)) + np.abs(qf.L(b1) * z.astype(qf.L))
                top = max(top, float(np.max(np.abs(recon - ref) / ((asm.terms + C_SLACK) * qf.L(qf.EPS) * scale))))
    finally:
        for A in ops.values():
            A.destroy()
    inst = (True, bool(R.lay.tables_lds))
    _note(("k_mf_qudit", inst), top, name)
    print("3. %s: k_mf_qudit<REALX 1, TLDS %d>, three drivers, with and without b1 z: largest error / bound %.3g" % (name, inst[1], top))


# ----------------------------------------------------------------------------------------------------- 4. row shards --
@pytest.mark.parametrize("name", SHARD_CASES + ["d2_n32_q16_alternating"])
def test_ragged_row_shards_bit_for_bit(name):
    R = _ref(name)
    asm = R.asm
    m, r0 = asm.nrows, asm.r0
    t = TRIPLES[4]
    M = _mf(name, R.rows)
    X = _X(R, M)
    yv = q.DeviceVec(M, m)
    try:
        R.bind(X.at_need())
        yv.upload(R.y0)
        M.spmv(X.ptr, yv.ptr, *t)
        y = yv.download()
        _check_rows("%s whole" % name, R, y, R.ref(t))
        cuts = sorted({c for c in (0, 1, 64, 127, m // 3 + 1, m - 5, m) if 0 <= c <= m})
        nnz = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            S = _mf(name, (r0 + a, r0 + b))
            sv = q.DeviceVec(S, b - a)
            try:
                i = S.info()
                assert S.dim == i.nrows == b - a and i.row_offset == r0 + a
                assert S.nnz == int(asm.ia[b] - asm.ia[a]), (name, a, b)
                nnz += S.nnz
                sv.upload(R.y0[a:b])
                S.spmv(X.ptr, sv.ptr, *t)
                got = sv.download()
                assert np.array_equal(_bits(got), _bits(y[a:b])), "%s: rows [%d, %d) differ from the whole operator's" % (name, a, b)
            finally:
                sv.free()
                S.destroy()
        assert nnz == M.nnz
    finally:
        yv.free()
        X.free()
        M.destroy()


# ------------------------------------------------------------------------------------------------------ 5. deep rows --
def _heisenberg_spin1():
    """S.S on two spin-1 sites, levels l = 1 - m: three off-diagonal moves |l, l'> <-> |l - 1, l' + 1>"""
    d = 3
    M = np.zeros((9, 9), dtype=np.complex128)
    for a in range(d):
        for b in range(d):
            M[a * d + b, a * d + b] = (1 - a) * (1 - b)
            if a + 1 < d and b - 1 >= 0:
                M[(a + 1) * d + b - 1, a * d + b] = M[a * d + b, (a + 1) * d + b - 1] = 1.0
    return M


@pytest.mark.parametrize("n,d,total,dim,r0", [(24, 3, 24, 27_948_336_381, 27_000_000_000), (64, 2, 32, 1832624140942590534, 1832624140942590534 - 4096)])
def test_deep_rows_without_a_vector(n, d, total, dim, r0):
    """The handle's nnz over 4096 rows, counted on the device by k_mf_qudit_count, equals the count made here from `unrank` and the
    classes' row lengths; device memory in use stays small (a vector of either sector would not fit any device)."""
    import torch
    r1 = r0 + 4096
    if d == 3:
        pairs = [(i, (i + 1) % n, _heisenberg_spin1()) for i in range(n)]
    else:
        X = np.zeros((4, 4), dtype=np.complex128)
        X[1, 2] = X[2, 1] = 0.5
        X[1, 1] = X[2, 2] = -0.25
        X[0, 0] = X[3, 3] = 0.25
        pairs = [(i, (i + 1) % n, X) for i in range(n)] + [(0, 32, X), (63, 31, X)]
    cnt = qf.Counter(n, d, total)
    assert cnt.dim == dim
    if d == 2:
        assert all(cnt.unrank(r)[63] == 1 for r in (r0, r1 - 1))                 # bit 63 set in every word of the shard
    free0 = torch.cuda.mem_get_info()[0]
    M = q.csr_mat.qudit(n, d, total, pairs, [], rows=(r0, r1), matrix_free=True)
    try:
        used = free0 - torch.cuda.mem_get_info()[0]
        i = M.info()
        assert i.ncols == dim and i.nrows == 4096 and i.row_offset == r0 and i.kernel == _lib.KERNEL_MATRIX_FREE
        assert 0 < i.bytes_matrix < 4 << 20 and used < 64 << 20, used
        assert M.nnz == qf.count_rows(n, d, total, pairs, r0, r1)
    finally:
        M.destroy()


# ------------------------------------------------------------------------------------------------- 6. coverage gate --
def test_zz_every_instance_and_both_sides_of_every_boundary_were_exercised():
    """From the mirror alone: which instances and edges the parametrised tests above run.  No case of the table is left out."""
    assert set(MF_CASES) == set(qf.CASES) and set(GEN_CASES) == {n for n, c in qf.CASES.items() if c["dim"] <= 50_000 or c["rows"]}
    lay = qf.layout_of
    inst = {(False, bool(lay(n).tables_lds)) for n in MF_CASES} | {(True, bool(lay(n).tables_lds)) for n in DRIVER_CASES}
    assert inst == {(False, False), (False, True), (True, False), (True, True)}
    for a, b in qf.BOUNDARY_PAIRS:                                       # TLDS on and off one class apart
        assert {a, b} <= set(MF_CASES) and lay(a).tables_lds == 1 and lay(b).tables_lds == 0 and lay(b).n_cls - lay(a).n_cls == 1
        assert lay(a).lds_bytes(True) <= qf.LDS_CAP < lay(b).lds_bytes(True)
    assert {a for a, _ in qf.BOUNDARY_PAIRS} & set(DRIVER_CASES) and {b for _, b in qf.BOUNDARY_PAIRS} & set(DRIVER_CASES)
    rows = {lay(n).max_row for n in GEN_CASES}
    assert 240 in rows and 239 in rows and max(rows) == qf.MAX_ROW       # the capacity and one below; 241 is refused (test_qudit_cpu.py)
    assert any(int(np.diff(qf.reference_of(n).ia).max()) == 240 for n in GEN_CASES)
    edges = set().union(*(qf.CASES[n]["edge"] for n in MF_CASES))
    assert edges >= {"bit63", "nb64", "w64", "bits3", "top_full", "blocks", "dim1", "grid_stride", "maxk0", "diag_operator", "shared",
                     "cancelled", "no_single"}
    assert {d for d in (qf.CASES[n]["d"] for n in GEN_CASES)} == {2, 3, 4, 6, 7, 8}
    assert any(lay(n).padding for n in MF_CASES) and any(lay(n).padding == 0 for n in MF_CASES)
    assert any(lay(n).has_single == 0 for n in MF_CASES)
    for key in sorted(TOP, key=str):
        print("largest error / bound  %-40s %.3g  (%s)" % (key, TOP[key][0], TOP[key][1]))
