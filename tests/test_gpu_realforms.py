"""The all-real SpMV forms, element by element.

The library's default form of a real operator (dictionary-coded values, packed-double vectors inside the solvers) runs kernels
that qbh_spmv_dev never reaches: the row-staged Hubbard kernel (matrix-free, and as the table route of the coded Kronecker
split), the sliced and two-part coded split passes, the row kernel gathering 8-byte reals, the lane kernels k_mf_hubbard<true>
and k_mf_heis<true, NCH>.  One Lanczos continuation step exposes one SpMV of them exactly: with purpose "dnmcs", k = 1 and
np = 1, slot 0 = z, slot 1 = x (|x| = 1) and hess[1] = b1, the solver runs

    w = H x - b1 z  (fused SpMV epilogue),  a1 = <x, w>  (fused partial sums),  w -= a1 x,  b2 = |w|,  slot 0 <- w / b2

so  (H x)_i = b2 v2_i + a1 x_i + b1 z_i.  Every reconstructed element is compared with a long-double reference built from an
independent host assembly of the operator (tests/fastham.py, tests/kronsum.py) within a bound that holds for any summation
order, with or without FMA:

    |recon_i - ref_i| <= (nnz_i + 8) eps ((|H||x|)_i + |a1 x_i| + |b1 z_i|)

x has 0.25 <= |x_j| <= 1 before normalisation, so every term of every row is far above that bound: a dropped, doubled or
misplaced term cannot hide.  a1 and b2 are checked against the reference as well.  Three drivers per case: qbh_lanczos_real_dev
(packed doubles throughout), qbh_lanczos on complex vectors with zero imaginary parts (real_forms 7: packed internally) and the
same with real_forms 3 (8-byte x gathers, complex y).
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import fastham
import kronsum
import quantum_basis_amd as q
from quantum_basis_amd import _lib, lattices

pytestmark = pytest.mark.gpu

MAXIT = 4
EPS = np.finfo(np.float64).eps
C_SLACK = 8
B1 = 1.3
DRIVERS = ("real", "cplx7", "cplx3")


# ---------------------------------------------------------------------------------------------------------------- probe --
def _probe(A, x, z, b1, driver):
    """One Lanczos continuation step on x (slot 1) and z (slot 0) with hess[1] = b1: returns (v2, a1, b2)."""
    n = A.dim
    assert A.info().basis_internal == 0
    hess = np.zeros(2 * MAXIT)
    hess[1] = b1
    n_real = A.stats().n_spmv_real
    if driver == "real":
        v = A.vec(1)                                          # 16 n bytes: two slots of n doubles
        v.upload(np.ascontiguousarray(np.concatenate([z, x])).view(np.complex128))
        m = q.lanczos_real(1, 1, MAXIT, A, v, hess, "dnmcs")
        out = v.download().view(np.float64).copy()
        v.free()
        v2, xo = out[:n], out[n:]
    else:
        vv = np.zeros(2 * n, dtype=np.complex128)
        vv[:n], vv[n:] = z, x
        m = q.lanczos(1, 1, MAXIT, n, A, vv, hess, "dnmcs")
        assert not np.any(vv.imag[n:]) and (hess[2] == 0.0 or not np.any(vv.imag[:n]))     # b2 = 0 (n = 1): v2 = 0 / 0
        v2, xo = vv.real[:n].copy(), vv.real[n:].copy()
    assert m == 2
    assert np.array_equal(xo, x)                               # the step leaves its x in place
    assert A.stats().n_spmv_real > n_real, "%s: the SpMV did not run the all-real form" % driver
    return v2, hess[MAXIT + 1], hess[2]


def _check(what, ref_csr, x, z, b1, v2, a1, b2, S=None):
    """Element-wise check of the reconstruction; the message names the worst row, its (u, d) and error / bound."""
    ia, ja, val = ref_csr
    n = len(x)
    ref, absref = kronsum.row_sums(ia, ja, val, x)
    L = np.longdouble
    xl, zl = x.astype(L), z.astype(L)
    w = L(b2) * v2.astype(L) if b2 != 0.0 else np.zeros(n, dtype=L)      # n = 1: w - a1 x is exactly 0
    recon = w + L(a1) * xl + L(b1) * zl
    nnz = np.diff(ia).astype(L)
    scale = absref + np.abs(L(a1) * xl) + np.abs(L(b1) * zl)
    bound = (nnz + C_SLACK) * L(EPS) * scale
    err = np.abs(recon - ref)
    ratio = err / np.maximum(bound, L(np.finfo(np.float64).tiny))
    i = int(np.argmax(ratio))
    ud = "" if S is None else " (u, d) = (%d, %d)" % divmod(i, S)
    assert ratio[i] <= 1.0, "%s: row %d%s: |recon - ref| = %.3e, bound %.3e (ratio %.3g), ref %.17g; %d rows over" % (
        what, i, ud, float(err[i]), float(bound[i]), float(ratio[i]), float(ref[i]), int((ratio > 1).sum()))
    # a1 = <x, H x - b1 z> (any summation order: (n - 1) eps of the absolute sum, plus the rows' own error)
    wref = ref - L(b1) * zl
    a1_ref = np.dot(xl, wref)
    t_a1 = (float(nnz.max()) + C_SLACK) * EPS * float(np.dot(np.abs(xl), absref + np.abs(L(b1) * zl))) \
        + (n + C_SLACK) * EPS * float(np.dot(np.abs(xl), np.abs(wref)))
    assert abs(float(L(a1) - a1_ref)) <= t_a1, "%s: a1 = %.17g, reference %.17g (|diff| %.3e > %.3e)" % (
        what, a1, float(a1_ref), abs(float(L(a1) - a1_ref)), t_a1)
    # b2 = |H x - b1 z - a1 x| with the step's own a1
    r = wref - L(a1) * xl
    b2_ref = float(np.sqrt(np.dot(r, r)))
    t_b2 = (float(nnz.max()) + C_SLACK) * EPS * float(np.sqrt(np.dot(scale, scale))) + (n + C_SLACK) * EPS * b2_ref
    assert abs(b2 - b2_ref) <= t_b2, "%s: b2 = %.17g, reference %.17g (|diff| %.3e > %.3e)" % (what, b2, b2_ref, abs(b2 - b2_ref), t_b2)
    return recon


def _run(what, make, ref_csr, drivers=DRIVERS, S=None, seed=1, route=None):
    """make(real_forms) -> operator; every driver, with z = 0, b1 = 0 and with a random z, b1 = 1.3.  route(info) asserts the form
    the operator took.  Returns {(driver, with_beta): reconstruction}."""
    n = len(ref_csr[0]) - 1
    x = kronsum.probe_vector(n, seed)
    zr = kronsum.probe_vector(n, seed + 1000)
    out = {}
    ops = {}
    for drv in drivers:
        rf = 3 if drv == "cplx3" else 7
        if rf not in ops:
            ops[rf] = make(rf)
            if route is not None:
                route(ops[rf].info())
        A = ops[rf]
        assert A.dim == n
        for beta in (False, True):
            z, b1 = (zr, B1) if beta else (np.zeros(n), 0.0)
            v2, a1, b2 = _probe(A, x, z, b1, drv)
            out[(drv, beta)] = (_check("%s [%s, b1 = %g]" % (what, drv, b1), ref_csr, x, z, b1, v2, a1, b2, S), v2, a1, b2)
    for A in ops.values():
        A.destroy()
    return out, x, zr


def _csr(H):
    H = sp.csr_matrix(H)
    H.sort_indices()
    return H.indptr.astype(np.int64), H.indices.astype(np.int64), H.data.astype(np.float64)


def _same_rows(what, o1, o2, x, z):
    """Two probes of the same operator whose per-row sums are formed in the same order: y is the same, but a1 and b2 come from
    partial sums grouped by workgroup, and the workgroups differ, so v2 = (y - a1 x) / b2 can differ in the last bits.  What is
    left after adding a1 x + b1 z back must agree to the rounding of that axpy and scaling alone (4 eps), not to the row bound."""
    for beta in (False, True):
        r1, v1, a1, b1_ = o1[("real", beta)]
        r2, v2, a2, b2_ = o2[("real", beta)]
        L = np.longdouble
        scale = np.abs(L(b1_) * v1.astype(L)) + np.abs(L(a1) * x.astype(L)) + (np.abs(L(B1) * z.astype(L)) if beta else 0)
        d = np.abs(r1 - r2)
        i = int(np.argmax(d / np.maximum(scale, L(1e-300))))
        assert d[i] <= 4 * EPS * scale[i], "%s: row %d differs by %.3e (4 eps scale %.3e)" % (what, i, float(d[i]), float(4 * EPS * scale[i]))


# -------------------------------------------------------------------------------------------- matrix-free Hubbard --
LDS_CAP = 150 * 1024


def _mf_kernel(Nd, wu):
    """Mirror of mf_row_kernel_ok / launch_mf_hubbard (qbh_mf.hip) for real vectors: which kernel applies the operator."""
    if not (Nd >= 256 and Nd < (1 << 24) and wu <= 64):
        return "lane"
    return "row_windowed" if Nd * 8 > LDS_CAP else "row"


def _window(Nd, d, chunk, wcap):
    """[w_lo, w_hi) of k_mf_hubbard_row<true> for the chunk holding d."""
    c_lo = (d // chunk) * chunk
    c_hi = np.minimum(c_lo + chunk, Nd)
    w_lo = np.maximum(0, c_lo - (wcap - (c_hi - c_lo)) // 2)
    w_hi = w_lo + wcap
    clamp = w_hi > Nd
    w_hi = np.where(clamp, Nd, w_hi)
    w_lo = np.where(clamp, np.maximum(0, Nd - wcap), w_lo)
    return w_lo, w_hi


def _misses(Td, chunk=8192, wcap=18432):
    """Down hops whose target lies outside the LDS window of their row, with the kernel's own window formula."""
    Td = sp.csr_matrix(Td)
    Nd = Td.shape[0]
    d = np.repeat(np.arange(Nd), np.diff(Td.indptr))
    lo, hi = _window(Nd, d, chunk, wcap)
    return int(((Td.indices < lo) | (Td.indices >= hi)).sum())


_MF_CACHE = {}


def _mf_ref(L, n_up, n_dn, bonds_name, U=1.1):
    key = (L, n_up, n_dn, bonds_name, U)
    if key not in _MF_CACHE:
        bonds = _BONDS[bonds_name](L)
        H = fastham.hubbard_full(L, n_up, n_dn, bonds, t=1.0, U=U)
        _, Tu = fastham._hop_matrix(L, n_up, bonds, 1.0)
        _, Td = fastham._hop_matrix(L, n_dn, bonds, 1.0)
        _MF_CACHE.clear()                                     # one geometry at a time (host memory)
        _MF_CACHE[key] = (_csr(H), Tu, Td, bonds)
    return _MF_CACHE[key]


_BONDS = {"chain": lambda L: lattices.chain(L), "4x3": lambda L: lattices.square(4, 3)}

# (L, n_up, n_dn, kernel expected): Nd = C(L, n_dn)
MF_CASES = [
    (10, 5, 5, "lane"),              # Nd 252: below the row kernel's 256
    (11, 4, 4, "row"),               # Nd 330
    (11, 0, 4, "row"),               # no up species: one up configuration, a padding-only neighbour list
    (11, 11, 4, "row"),              # all up sites filled: the same
    (18, 1, 6, "row"),               # Nd 18564: the largest unwindowed row, 148.5 KB of LDS
    (17, 1, 7, "row_windowed"),      # Nd 19448: the smallest windowed row; three chunks, the last partial, clamped windows
    (20, 1, 6, "row_windowed"),      # Nd 38760
]


def _mf_make(L, n_up, n_dn, bonds):
    return lambda rf: q.csr_mat.hubbard(L, n_up, n_dn, bonds, t=1.0, U=1.1, opts=q.make_opts(real_forms=rf), matrix_free=True)


@pytest.mark.parametrize("case", MF_CASES, ids=["L%d_%d+%d_%s" % c for c in MF_CASES])
def test_matrix_free_hubbard_real_forms(case):
    L, n_up, n_dn, kernel = case
    ref, Tu, Td, bonds = _mf_ref(L, n_up, n_dn, "chain")
    Nd = math.comb(L, n_dn)
    assert Td.shape[0] == Nd
    wu = max(8, -(-int(np.diff(Tu.indptr).max()) // 8) * 8)     # the up table's padded width
    assert _mf_kernel(Nd, wu) == kernel
    if kernel == "row_windowed":
        assert _misses(Td) > 0, "the default window holds every down hop: the miss branch is not exercised"
    _run("mf hubbard L%d %d+%d (%s)" % case, _mf_make(L, n_up, n_dn, bonds), ref, S=Nd)


@pytest.mark.parametrize("case", [(17, 1, 7), (20, 1, 6)], ids=["L17", "L20"])
def test_matrix_free_hubbard_window_knobs(case, monkeypatch):
    """The window of the row-staged kernel is a measurement knob (QBH_DEBUG mf_chunk / mf_window): narrower windows send many more
    down hops through the miss branch, the per-row sums stay the same.  mf_row=0 turns the row-staged kernel off: the lane kernel
    k_mf_hubbard<true> applies the same operator."""
    L, n_up, n_dn = case
    ref, Tu, Td, bonds = _mf_ref(L, n_up, n_dn, "chain")
    Nd = math.comb(L, n_dn)
    make = _mf_make(L, n_up, n_dn, bonds)
    base, x, z = _run("mf L%d default window" % L, make, ref, drivers=("real",), S=Nd)
    for knob, (chunk, wcap) in (("mf_chunk=1024,mf_window=1024", (1024, 1024)), ("mf_chunk=2048,mf_window=2048", (2048, 2048)),
                                ("mf_chunk=1024,mf_window=4096", (1024, 4096))):
        assert _misses(Td, chunk, wcap) > _misses(Td)
        monkeypatch.setenv("QBH_DEBUG", knob)
        o, _, _ = _run("mf L%d %s" % (L, knob), make, ref, drivers=("real",), S=Nd)
        _same_rows("mf L%d %s against the default window" % (L, knob), base, o, x, z)
    monkeypatch.setenv("QBH_DEBUG", "mf_row=0")
    o, _, _ = _run("mf L%d lane kernel (mf_row=0)" % L, make, ref, drivers=("real", "cplx3"), S=Nd)
    _same_rows("mf L%d lane kernel against the row-staged kernel" % L, base, o, x, z)
    monkeypatch.delenv("QBH_DEBUG")


# ------------------------------------------------------------------------------------------ coded split, host arrays --
def _table_route_expected(K, S):
    """What kronc_build_sliced / kronc_table_route take for this matrix: (sliced, table)."""
    sliced = K["n_dict"] <= 255 and S <= 20 * 1024 and (S + 306) * 8 <= 159 * 1024 and K["NU"] <= 65535
    wu_pad = max(8, -(-K["wu"] // 8) * 8)
    table = sliced and S >= 256 and K["n_amp"] <= 15 and wu_pad <= 64
    return sliced, table


# (name, kronsum arguments)
KS_CASES = [
    ("S256", dict(NU=16, S=256, far=1, empty_t=3)),
    ("S255", dict(NU=16, S=255, far=1, empty_t=3)),                          # below the table kernel's 256: sliced passes
    ("S19200", dict(NU=4, S=19200, far=2)),                       # the row kernel's largest unwindowed row
    ("S19201", dict(NU=5, S=19201, far=2, empty_t=1)),                       # windowed
    ("S20046", dict(NU=3, S=20046, wu=2, far=2)),                       # the largest S whose block fits the near pass's LDS
    ("S20047", dict(NU=3, S=20047, wu=2, far=2)),                       # no coded split: the unsplit row kernel
    ("wu64", dict(NU=70, S=256, wu=64)),
    ("wu65", dict(NU=70, S=256, wu=65)),                          # wider than the kernel's neighbour list: sliced passes
    ("amp15", dict(NU=16, S=256, n_amp=15, band=4)),
    ("amp16", dict(NU=16, S=256, n_amp=16, band=4)),              # more than the table's 15 codes: sliced passes
    ("dict255", dict(NU=16, S=256, n_amp=3, n_diag=252)),
    ("dict256", dict(NU=16, S=256, n_amp=3, n_diag=253)),         # 1-byte codes without a free padding code: no split
    ("dict257", dict(NU=16, S=256, n_amp=3, n_diag=254)),         # 2-byte codes
]


def _ks_make(K, **more):
    def make(rf):
        return q.csr_mat(K["dim"], K["ia"], K["ja"], K["val"].astype(np.complex128), sym=False,
                         opts=q.make_opts(kron_minor=K["S"], kron_split=2, real_forms=rf, **more))
    return make


@pytest.mark.parametrize("name", [c[0] for c in KS_CASES])
def test_coded_split_table_route_and_fallbacks(name):
    kw = dict(KS_CASES)[name]
    K = kronsum.kronsum(seed=7, **kw)
    S = K["S"]
    sliced, table = _table_route_expected(K, S)
    if name in ("S256", "S19200", "S19201", "S20046", "wu64", "amp15", "dict255"):
        assert table
    if name in ("S255", "wu65", "amp16"):
        assert sliced and not table
    if name in ("S20047", "dict256", "dict257"):
        assert not sliced
    if table and S * 8 > LDS_CAP:
        assert _misses(sp.csr_matrix((K["Tp"][2], K["Tp"][1], K["Tp"][0]), shape=(S, S))) > 0
    ref = (K["ia"], K["ja"], K["val"])

    def route(info, rf=7):
        assert info.value_dict == K["n_dict"]
        assert info.kron_minor == (S if sliced else 0) and info.kron_sliced == (1 if sliced else 0)
        assert info.kron_table_kernel == (1 if table else 0)
        if sliced:
            assert info.kron_band == 16
    _run("kronsum %s" % name, _ks_make(K), ref, S=S, route=route)
    # the same matrix through the other forms of the split: sliced passes with T, T' kept once (kron_uniform 3), every group
    # stored (0), the two-part row-kernel form (kron_coded 1)
    for more in (dict(kron_uniform=3), dict(kron_uniform=0), dict(kron_coded=1)):
        def route2(info, more=more):
            assert info.kron_table_kernel == 0 and info.value_dict == K["n_dict"]
            if "kron_uniform" in more:
                assert info.kron_minor == (S if sliced else 0) and info.kron_sliced == (1 if sliced else 0)
            else:
                assert info.kron_minor == S and info.kron_sliced == 0
        _run("kronsum %s %s" % (name, more), _ks_make(K, **more), ref, drivers=("real",), S=S, route=route2)


# --------------------------------------------------------------------------------- row kernel, real gathers, unsplit --
def _random_real(n, density, seed, long_row=False, empty_rows=0, few_values=False):
    rng = np.random.default_rng(seed)
    m = max(1, int(density * n * n))
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    v = rng.choice(np.array([0.5, -1.0, 0.75, 2.0]), m) if few_values else rng.normal(size=m)
    M = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    if long_row and n > 8:
        M = M.tolil()
        M[n // 3, :] = rng.choice(np.array([0.5, -1.0]), n) if few_values else rng.normal(size=n)
        M = M.tocsr()
    M = M + M.T
    if empty_rows and n > 2 * empty_rows + 2:
        keep = np.ones(n)
        keep[rng.choice(n, empty_rows, replace=False)] = 0.0
        M = sp.diags(keep) @ M @ sp.diags(keep)
    diag = rng.choice(np.array([0.0, 1.1, 2.2]), n) if few_values else rng.normal(size=n)
    M = sp.csr_matrix(M + sp.diags(diag))
    M.sum_duplicates()
    M.eliminate_zeros()
    # the reference always stores the diagonal: explicit entries where it is zero
    M = sp.csr_matrix(M + sp.diags(np.full(n, 1e-300)))
    M.sort_indices()
    return M


RK_SHAPES = [
    dict(n=1, density=1.0), dict(n=2, density=0.5), dict(n=7, density=0.4), dict(n=257, density=0.05),
    dict(n=1000, density=0.05, few_values=True), dict(n=3001, density=0.002, long_row=True),
    dict(n=3001, density=0.002, long_row=True, few_values=True), dict(n=2049, density=0.003, empty_rows=40),
    dict(n=4097, density=0.01, few_values=True, empty_rows=10),
]


@pytest.mark.parametrize("npb", [0, 1024])
@pytest.mark.parametrize("shape", range(len(RK_SHAPES)))
def test_row_kernel_real_gathers_unsplit(shape, npb):
    kw = RK_SHAPES[shape]
    M = _random_real(seed=300 + shape, **kw)
    n = M.shape[0]
    ia, ja, val = _csr(M)
    if kw.get("long_row"):
        assert np.diff(ia).max() > 1024                         # longer than the kernel's LDS tile
    if kw.get("empty_rows"):
        assert (np.diff(ia) == 1).sum() >= 1                      # rows with the stored (tiny) diagonal only
    n_dict = len(np.unique(val))

    def route(info):
        assert info.kernel == _lib.KERNEL_ROWS and info.kron_minor == 0 and info.value_dict == n_dict

    def make(rf):
        return q.csr_mat(n, ia, ja, val.astype(np.complex128), sym=False,
                         opts=q.make_opts(spmv_kernel=_lib.KERNEL_ROWS, kron_split=0, nnz_per_block=npb, real_forms=rf))
    assert (n_dict > 256) == (not kw.get("few_values", False) and n > 7)
    _run("random n=%d %s npb %d dict %d" % (n, kw, npb, n_dict), make, (ia, ja, val), seed=shape + 1, route=route)


def test_row_kernel_empty_rows_without_stored_diagonal():
    """Rows with no entry at all, the diagonal included (the builders above always store it), and a trailing empty row."""
    n = 600
    M = _random_real(n, 0.01, 77)
    keep = np.ones(n)
    keep[np.random.default_rng(78).choice(n - 1, 30, replace=False)] = 0.0
    keep[n - 1] = 0.0
    M = sp.csr_matrix(sp.diags(keep) @ M @ sp.diags(keep))
    M.eliminate_zeros()
    ia, ja, val = _csr(M)
    assert (np.diff(ia) == 0).sum() == 31 and ia[-1] == ia[-2]

    def make(rf):
        return q.csr_mat(n, ia, ja, val.astype(np.complex128), sym=False, opts=q.make_opts(kron_split=0, real_forms=rf))
    _run("random n=%d with empty rows" % n, make, (ia, ja, val), seed=5)


# ------------------------------------------------------------------------------------------- matrix-free Heisenberg --
def _heis_bonds(L, uniform):
    b = lattices.chain(L) + [(i, (i + 5) % L) for i in range(0, L, 3)]
    if not uniform:
        b += [b[0], b[3], (0, L - 1)]                         # listed twice: J = 2 on those bonds (merged weights)
    return b


@pytest.mark.parametrize("L,n_dn,uniform", [(18, 3, True), (18, 3, False), (24, 3, True), (30, 2, True), (31, 3, True),
                                            (36, 2, True), (36, 3, False)])
def test_matrix_free_heisenberg_real_forms(L, n_dn, uniform):
    """k_mf_heis<true, NCH>: 18 sites -- the generic re-ranking loop; 24 / 30 / 31-36 sites -- NCH = 4 / 5 / 6 (bits 30 and up from
    the high half of the flipped pattern).  Non-uniform J (a bond listed twice) takes the per-bond diagonal and amplitudes."""
    bonds = _heis_bonds(L, uniform)
    H = fastham.heisenberg_full(L, n_dn, bonds, J=1.0)
    ref = _csr(H)
    offd = np.unique(np.abs(ref[2][ref[1] != np.repeat(np.arange(H.shape[0]), np.diff(ref[0]))]))
    assert (len(offd) == 1) == uniform

    def make(rf):
        return q.csr_mat.heisenberg(L, n_dn, bonds, J=1.0, opts=q.make_opts(real_forms=rf), matrix_free=True)
    _run("mf heisenberg L%d n_dn %d %s" % (L, n_dn, "uniform" if uniform else "non-uniform J"), make, ref, seed=L)


# ------------------------------------------------------------------------------------------------------------ sharded --
@pytest.mark.parametrize("geom", [(12, 6, 6, "4x3"), (17, 1, 7, "chain")], ids=["4x3_6+6", "L17_1+7"])
def test_sharded_matrix_free_hubbard_probe(geom):
    """5 gloo ranks on one GPU, shard boundaries inside an up-configuration row; each rank runs the probe on its slice (the
    row-staged kernel with row_begin inside a row, under the communicator's all-gather of x) and returns its v2 slice."""
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import dist_worker
    L, n_up, n_dn, bname = geom
    world = 5
    ref, Tu, Td, bonds = _mf_ref(L, n_up, n_dn, bname)
    n = len(ref[0]) - 1
    Nd = math.comb(L, n_dn)
    nblk = -(-n // world)
    assert any((r * nblk) % Nd for r in range(1, world))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(dist_worker.gpu_sharded_probe, args=(world, port, "gloo", tmp, L, n_up, n_dn, bname, B1), nprocs=world, join=True)
        for beta in (False, True):
            v2 = np.concatenate([np.load(tmp + "/v2_%d_%d.npy" % (beta, r)) for r in range(world)])
            ab = np.load(tmp + "/ab_%d.npy" % beta)
            x = kronsum.probe_vector(n, 11)
            z = kronsum.probe_vector(n, 12) if beta else np.zeros(n)
            _check("sharded mf %s [b1 = %g]" % (bname, B1 if beta else 0.0), ref, x, z, B1 if beta else 0.0, v2, ab[0], ab[1], S=Nd)
