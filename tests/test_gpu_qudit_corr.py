"""The d-level all-pair correlation kernel (qbh_corr_qudit_dev) element by element against tests/quditcorrref.py (the host
reference in longdouble, pinned by tests/test_quditcorrref.py), on random vectors that are not normalised, in the complex and the
packed-real form, with random real tables (K = 2) and every output buffer pre-filled with a sentinel.

Bound for every entry of every array:  |got - want| <= 4 (dim + n_sites + 4) 2^-53 norm2 W  (quditcorrref.bound): an entry is a
sum of at most dim terms whose moduli sum to at most W norm2, the n_sites term covers the products of up to n_sites table values,
W is the largest modulus a weight of the array can take (from the tables); `want` and norm2 come from the reference.  Entries
that must vanish exactly are compared exactly.

The launch's grid is min(tiles, CUs x workgroups per CU) workgroups of 256 x 4 rows a tile, workgroups per CU = min(4, 158 KB /
(LDS + 2 KB)) (corr_grid); (3, 15, 15) has 1,787,607 rows, more than the 4 x 256 CUs x 1024 = 1,048,576 rows of one trip on an
MI355X: test_the_large_case_takes_more_than_one_trip computes the grid from the device's CU count and asserts it.  Its vector is
random on a part of the rows (the first and last tiles, the rows around the end of the first trip, one row in 200 elsewhere) and
exactly zero on the others, so that the reference, whose cost goes with the nonzero rows, stays within seconds; the bound is
taken with the number of nonzero rows in place of dim."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import quditcorrref as ref
import quditforms as qf
import quantum_basis_amd as q
from quantum_basis_amd import _lib, lattices
from quantum_basis_amd import qudit as qd

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e300

# (d, n, total): the edge each one is here for
SHAPES = [
    (3, 1, 1),                     # dim 1, no pairs
    (3, 2, 2),                     # dim 3
    (3, 8, 8),                     # dim 1107, not a multiple of a tile
    (3, 12, 12),                   # dim 73789
    (3, 32, 2), (3, 32, 62),       # dim 528 each: 64 bits used, top field at bits 62-63, nearly empty and nearly full
    (4, 32, 3),                    # 2-bit fields with every code valid
    (5, 6, 9), (7, 5, 11),         # 3-bit fields partly used
    (8, 21, 2), (8, 21, 145),      # dim 231 each: 63 bits, level 7 in the top field
    (2, 64, 2),                    # dim 2016, two sites beyond what the spin kernel accepts
    (3, 6, 0), (3, 6, 12),         # dim 1: every aa entry off the diagonal is an exact zero
]
BIG = (3, 15, 15)
KEYS = ("norm2", "pop", "dd", "str", "aa")


def _tables(d, seed):
    rng = np.random.default_rng(seed)
    return dict(diag=rng.uniform(-1.5, 1.5, size=(2, d)), string=(rng.uniform(-1.5, 1.5, size=d), rng.uniform(-1.1, 1.1, size=d)),
                lower=np.append(0.0, rng.uniform(0.3, 1.7, size=d - 1)))


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=n) + 1j * rng.normal(size=n)) * 1.3).astype(np.complex128)        # not normalised


@functools.lru_cache(maxsize=None)
def _case(d, n, total, real):
    """(host vector, tables, reference arrays) -- computed once, shared, never modified"""
    x = _rand(qd.qudit_dim(n, d, total), 7 + 1000 * d + 100 * n + total)
    if real:
        x = np.ascontiguousarray(x.real)
    tabs = _tables(d, 31 * d + n)
    return x, tabs, ref.correlations(n, d, total, x, **tabs)


def _dev(x):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw(d, n, total, t, tabs, want=KEYS):
    real = t.dtype == torch.float64
    f = np.ascontiguousarray(tabs["diag"], dtype=np.float64)
    K = len(f)
    h, g = (np.ascontiguousarray(a, dtype=np.float64) for a in tabs["string"])
    low = np.ascontiguousarray(tabs["lower"], dtype=np.float64)
    out = {"norm2": np.full(1, SENTINEL), "pop": np.full((n, d), SENTINEL), "dd": np.full((K, K, n, n), SENTINEL),
           "str": np.full((n, n), SENTINEL), "aa": np.full((n, n), SENTINEL + 1j * SENTINEL)}
    p = {k: (_ptr(out[k]) if k in want else None) for k in out}
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_qudit_dev(n, d, total, None if real else addr, addr if real else None, K, _ptr(f), _ptr(h), _ptr(g),
                                             _ptr(low), p["norm2"], p["pop"], p["dd"], p["str"], p["aa"], None), "qbh_corr_qudit_dev")
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


def _check_mirrors(got):
    assert np.array_equal(got["aa"], got["aa"].conj().T) and np.array_equal(got["str"], got["str"].T)
    assert np.array_equal(got["dd"], got["dd"].transpose(1, 0, 3, 2))                    # <f_a(i) f_b(j)> = <f_b(j) f_a(i)>


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_n%d_q%d" % s)
def test_every_entry_against_the_reference(shape, real):
    d, n, total = shape
    x, tabs, want = _case(d, n, total, real)
    got = _raw(d, n, total, _dev(x), tabs)
    ref.compare("qudit %s %s" % (shape, "real" if real else "complex"), got, want, len(x), n, ref.weights(n, **tabs))
    _check_mirrors(got)
    if len(x) == 1:
        assert np.all(got["aa"][~np.eye(n, dtype=bool)] == 0)


def _grid(n, total, dim):
    """corr_grid for this kernel: (workgroups along x, rows of one trip)"""
    lds = (n * (total + 2) + 64 + 256 * 5) * 8
    per_cu = max(1, min(4, (158 * 1024) // (lds + 2048)))
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    gx = max(1, min((dim + 1023) // 1024, ncu * per_cu))
    return gx, gx * 1024


@functools.lru_cache(maxsize=None)
def _big_case(real):
    d, n, total = BIG
    dim = qd.qudit_dim(n, d, total)
    _, trip = _grid(n, total, dim)
    x = _rand(dim, 99)
    rng = np.random.default_rng(5)
    keep = rng.random(dim) < 1.0 / 200
    for lo, hi in ((0, 2100), (trip - 2100, trip + 2100), (dim - 2100, dim)):
        keep[max(lo, 0):min(hi, dim)] = True
    x[~keep] = 0.0
    if real:
        x = np.ascontiguousarray(x.real)
    tabs = _tables(d, 77)
    return x, tabs, ref.correlations(n, d, total, x, **tabs), int(keep.sum())


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_the_large_case_takes_more_than_one_trip(real):
    d, n, total = BIG
    dim = qd.qudit_dim(n, d, total)
    assert dim == 1787607
    gx, trip = _grid(n, total, dim)
    print("grid %d workgroups x 1024 rows = %d rows a trip, dim %d" % (gx, trip, dim))
    assert trip < dim                                                   # rows beyond one trip of the grid actually used
    x, tabs, want, nnz = _big_case(real)
    got = _raw(d, n, total, _dev(x), tabs)
    ref.compare("qudit %s %s (%d nonzero rows)" % (BIG, "real" if real else "complex", nnz), got, want, nnz, n, ref.weights(n, **tabs))
    _check_mirrors(got)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_null_groups_and_repeatability(real):
    d, n, total = 3, 8, 8
    x, tabs, _ = _case(d, n, total, real)
    t = _dev(x)
    full, again = _raw(d, n, total, t, tabs), _raw(d, n, total, t, tabs)
    assert all(_same_bits(full[k], again[k]) for k in full)                     # two calls: the same bits
    for want in [("norm2",), ("pop",), ("dd",), ("str",), ("aa",), ("norm2", "pop", "dd"), ("str", "aa"), ("dd", "aa"), ("pop", "str"), ()]:
        part = _raw(d, n, total, t, tabs, want)
        for k in full:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)                  # the other outputs keep their bits
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)  # a group that was not asked for: untouched


def test_two_levels_agree_with_the_spin_half_kernel():
    """d = 2, f = 1/2 - l, lower = {0, 1}: aa = pm, dd = zz and pop gives sz of qbh_corr_spin_dev on the same vector, within the sum of
    the two kernels' bounds (both against exact arithmetic)"""
    N, n_dn = 13, 6
    for real in (False, True):
        x = _rand(qd.qudit_dim(N, 2, n_dn), 3)
        if real:
            x = np.ascontiguousarray(x.real)
        t = _dev(x)
        s = q.spin_correlations(N, n_dn, t, real=real, normalize=False)
        c = q.qudit_correlations(N, 2, n_dn, t, diag=([0.5, -0.5],), lower=[0.0, 1.0], real=real, normalize=False)
        n2 = float(np.sum(np.abs(x.astype(np.clongdouble)) ** 2).real)
        tol = 4.0 * (len(x) + 4) * 2.0 ** -53 * n2 + ref.bound(len(x), N, n2, 1.0)
        err = {"norm2": abs(s["norm2"] - c["norm2"]), "pm": np.abs(s["pm"] - c["aa"]).max(), "zz": np.abs(s["zz"] - c["dd"][0, 0]).max(),
               "sz": np.abs(s["sz"] - c["pop"] @ np.array([0.5, -0.5])).max()}
        print("d = 2 against the spin kernel (%s): |difference| / bound  %s" % ("real" if real else "complex",
                                                                                "  ".join("%s %.3g" % (k, v / tol) for k, v in err.items())))
        assert all(v <= tol for v in err.values()), err


def test_sign_and_conjugation_of_aa_against_the_site_operator_and_dotc():
    """<S^+_i S^-_j> against moprXvec_qudit (S^-_j, then S^+_i) + dotc, a spin-1 chain, three pairs and one diagonal entry"""
    n, S, d = 8, 1, 3
    total = qd.spin_charge(n, S, 0)
    x, _, _ = _case(d, n, total, False)
    sz, sp, sm = qd.spin_matrices(S)
    lower = np.real(np.append(0.0, np.diag(sp, 1)))
    A = q.csr_mat.spin_heisenberg(n, S, 0, lattices.chain(n))
    t = _dev(x)
    mid = torch.zeros(qd.qudit_dim(n, d, total + 1), dtype=torch.complex128, device="cuda")
    y = torch.zeros(len(x), dtype=torch.complex128, device="cuda")
    got = q.qudit_correlations(n, d, total, t, lower=lower, normalize=False)
    n2 = float(np.sum(np.abs(x) ** 2))
    tol = 2.0 * ref.bound(len(x), n, n2, 2.0)                            # both routes round; lower^2 = 2
    rng = np.random.default_rng(5)
    pairs = [tuple(int(s) for s in rng.choice(n, size=2, replace=False)) for _ in range(3)] + [(0, n - 1), (n - 1, 0), (4, 4)]
    for i, j in pairs:
        ej, ei = np.zeros(n, dtype=np.complex128), np.zeros(n, dtype=np.complex128)
        ej[j], ei[i] = 1.0, 1.0
        assert q.moprXvec_qudit(n, d, total, +1, ej, sm, C.c_void_p(t.data_ptr()), C.c_void_p(mid.data_ptr())) == len(mid)
        assert q.moprXvec_qudit(n, d, total + 1, -1, ei, sp, C.c_void_p(mid.data_ptr()), C.c_void_p(y.data_ptr())) == len(x)
        val = A.dotc(C.c_void_p(t.data_ptr()), C.c_void_p(y.data_ptr()))
        print("aa[%d][%d] %r  site operators + dotc %r" % (i, j, got["aa"][i, j], val))
        assert abs(got["aa"][i, j] - val) <= tol
    A.destroy()


def _energy_by_spmv(A, x):
    v = A.vec(2)
    v.upload(x, 0)
    A.spmv(v.at(0), v.at(A.dim), 1.0, 0.0, 0.0)
    e = A.dotc(v.at(0), v.at(A.dim))
    v.free()
    return e


def test_energy_identity_for_a_random_vector():
    """<x| H |x> from the two-site expectation values equals spmv + dotc, for vectors that are no eigenvectors"""
    n, S = 8, 1
    bonds = lattices.chain(n)
    total = qd.spin_charge(n, S, 0)
    x, _, _ = _case(3, n, total, False)
    A = q.csr_mat.spin_heisenberg(n, S, 0, bonds, J=1.0)
    want = _energy_by_spmv(A, x)
    A.destroy()
    corr = q.spin_s_correlations(n, S, 0, _dev(x), normalize=False)
    got = q.energy_from_correlations(corr, bonds, J=1.0)
    n2 = float(np.sum(np.abs(x) ** 2))
    tol = 2.0 * len(bonds) * (ref.bound(len(x), n, n2, 1.0) + ref.bound(len(x), n, n2, 2.0))        # zz: W = 1, pm: W = 2; both routes round
    print("spin-1 ring 8: E from correlations %.15g, spmv + dotc %.15g, |diff| / bound %.3g" % (got, want.real, abs(got - want.real) / tol))
    assert abs(got - want.real) <= tol and abs(want.imag) <= tol
    n, nb, n_max, tt, U, mu = 6, 5, 3, 0.9, 1.1, 0.3
    bonds = lattices.chain(n)
    x = _rand(qd.qudit_dim(n, n_max + 1, nb), 21)
    A = q.csr_mat.bose_hubbard(n, nb, n_max, bonds, t=tt, U=U, mu=mu)
    want = _energy_by_spmv(A, x)
    A.destroy()
    c = q.bose_correlations(n, nb, n_max, _dev(x), normalize=False)
    i, j = np.array(bonds).T
    got = float(-tt * 2.0 * np.sum(c["obdm"][i, j].real) + 0.5 * U * np.sum(np.diag(c["nn"]) - c["dens"]) - mu * np.sum(c["dens"]))
    n2 = float(np.sum(np.abs(x) ** 2))
    weight = 2.0 * tt * len(bonds) * n_max + n * (0.5 * U * n_max * n_max + (0.5 * U + mu) * n_max)  # sum of |coefficient| W of the terms
    tol = 2.0 * ref.bound(len(x), n, n2, weight)
    print("bose-hubbard chain 6: E from correlations %.15g, spmv + dotc %.15g, |diff| / bound %.3g" % (got, want.real, abs(got - want.real) / tol))
    assert abs(got - want.real) <= tol and abs(want.imag) <= tol


def _real_gauge(v):
    """the eigenvector of a real symmetric operator with its arbitrary phase removed: the real part then holds all of it"""
    k = int(np.argmax(np.abs(v)))
    return v * (np.conj(v[k]) / abs(v[k]))


def _ground_state(L, **kw):
    A = q.csr_mat.spin_heisenberg(L, 1, 0, lattices.chain(L), **kw)
    res = q.locate_E0_lanczos(A, nev=1, ncv=1)
    A.destroy()
    return res.E0, _real_gauge(np.asarray(res.eigenvecs).reshape(-1))


def test_the_spin_one_ring_end_to_end():
    L, E0 = 12, -16.86955614
    bonds = lattices.chain(L)
    states = []
    e, psi = _ground_state(L)
    assert abs(e - E0) < 1e-8
    states += [("stored, complex", False, psi), ("stored, packed real", True, np.ascontiguousarray(psi.real))]
    e, psi_mf = _ground_state(L, matrix_free=True)
    assert abs(e - E0) < 1e-8
    states += [("matrix-free, complex", False, psi_mf), ("matrix-free, packed real", True, np.ascontiguousarray(psi_mf.real))]
    for name, real, vec in states:
        c = q.spin_s_correlations(L, 1, 0, _dev(vec), real=real)
        e_corr = q.energy_from_correlations(c, bonds)
        dist = (np.arange(L)[None, :] - np.arange(L)[:, None]) % L
        spread = max(float(np.ptp(c["ss"][dist == r])) for r in range(L))
        print("spin-1 ring 12 (%s): E %.10f, ss(1) %.10f, string(6) %.10f, sz2 %.10f, ss spread %.2e" % (
            name, e_corr, c["ss"][0, 1], c["string"][0, 6], c["sz2"][0], spread))
        assert abs(e_corr - E0) < 1e-8
        assert spread < 1e-9                                            # translation invariant
        assert abs(c["ss"][3, 3] - 2.0) < 1e-14
    # the string correlator against a dense diagonalisation at L = 8 (dim 1107)
    L = 8
    total = qd.spin_charge(L, 1, 0)
    asm = qf.assemble(L, 3, total, qd.heisenberg_terms(1, lattices.chain(L)), [], keep_terms=False)
    H = np.zeros((asm.dim, asm.dim))
    rows = np.repeat(np.arange(asm.nrows), np.diff(asm.ia))
    np.add.at(H, (rows, asm.ja), asm.val.real)
    ev, vecs = np.linalg.eigh(H)
    m = 1.0 - np.arange(3)
    dense = ref.correlations(L, 3, total, vecs[:, 0], string=(m, np.array([-1.0, 1.0, -1.0])))
    e, psi = _ground_state(L)
    # |<O>_psi - <O>_0| <= 2 |O| |psi - psi_0| <= 2 |r| / gap for a normalised psi with residual r = H psi - <H> psi, |O| <= 1
    r = H @ psi.real - (psi.real @ H @ psi.real) * psi.real
    tol = 2.0 * (np.linalg.norm(r) + np.linalg.norm(psi.imag) + abs(np.linalg.norm(psi) - 1.0)) / (ev[1] - ev[0]) + 1e-13
    c = q.spin_s_correlations(L, 1, 0, _dev(psi))
    want = np.asarray(dense["str"] / dense["norm2"], dtype=np.float64)
    print("spin-1 ring 8: E0 %.10f (dense %.10f), string(0, 6) %.12f dense %.12f, tolerance %.2e" % (e, ev[0], c["string"][0, 6], want[0, 6], tol))
    assert abs(e - ev[0]) < 1e-8
    assert abs(c["string"][0, 6] - want[0, 6]) <= tol and np.abs(c["string"] - want).max() <= tol
