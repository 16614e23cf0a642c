"""The Kondo all-pair correlation kernels (qbh_corr_kondo_dev) element by element against tests/kondocorrref.py (the host
reference in longdouble, pinned by tests/test_kondocorrref.py), on random vectors that are not normalised, in the complex and the
packed-real form, with every output buffer pre-filled with a sentinel.

Bound for every entry of every array:  |got - want| <= 4 (rows + 4) 2^-53 norm2  (kondocorrref.bound): an entry is a sum of at most
`rows` products whose moduli sum to at most norm2; every matrix element is +-1 or +-1/2.  `want` and norm2 come from the
reference.  Entries that must vanish exactly are compared exactly.

The launch's grid is min(tiles, CUs x 4) workgroups of 256 x 8 rows a tile (corr_grid; the kernel's LDS, 26,176 B, admits four
workgroups per CU); (9, 9, 0) has 5,280,932 rows, more than the 4 x 256 CUs x 2048 = 2,097,152 rows of one trip on an MI355X:
test_the_large_case_takes_more_than_one_trip computes the grid from the device's CU count and asserts it.  Its vector is random on
a part of the rows (the first and last tiles, the rows around the end of the first trip, one row in 200 elsewhere) and exactly zero
on the others, so that the reference, whose cost goes with the nonzero rows, stays within seconds; the bound is taken with the
number of nonzero rows in place of dim.

An L = 8 end-to-end case (E0 = -11.28542034 through Lanczos + CG with packed-real vectors) is not included: the L = 4 case below
covers the same route from correlations to the energy, and the large sector is covered by the energy identities."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import kondocorrref as ref
import quantum_basis_amd as q
from quantum_basis_amd import _lib, kondo, lattices

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e300
GROUPS = ("site", "nn", "zn", "zz", "hop", "ee", "ll", "le")

# (n_sites, n_elec, two_sz), dim: the edge each one is here for
SHAPES = [
    ((1, 1, 0), 2),                # the two words are coupled only by le[0][0]
    ((1, 0, 1), 1),                # dimension 1
    ((2, 0, 2), 1), ((2, 4, -2), 1),   # all pair entries off the diagonal exactly 0
    ((3, 3, 0), 56),
    ((5, 3, 2), 860),              # blocks of unequal shape; not a multiple of a tile
    ((6, 7, -1), 12432),
    ((6, 6, 0), 15184),
    ((21, 1, 20), 462),            # two blocks, bit 62 set
    ((21, 41, 20), 462),           # popcount(u) = 21 in the sign parities
    ((21, 0, 21), 1),
]
BIG = (9, 9, 0)
TILE = 256 * 8                     # rows of a tile: 256 lanes x kKcRows


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=n) + 1j * rng.normal(size=n)) * 1.3).astype(np.complex128)        # not normalised


@functools.lru_cache(maxsize=None)
def _case(shape, real):
    """(host vector, reference arrays) -- computed once, shared, never modified"""
    n, ne, tz = shape
    x = _rand(kondo.sector_dim(n, ne, tz), 7 + 1000 * n + 10 * ne + tz)
    if real:
        x = np.ascontiguousarray(x.real)
    return x, ref.correlations(n, ne, tz, x)


def _dev(x):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _addr(t):
    return C.c_void_p(t.data_ptr())


def _raw(shape, t, want=GROUPS):
    n, ne, tz = shape
    real = t.dtype == torch.float64
    z = SENTINEL + 1j * SENTINEL
    out = {"norm2": np.full(1, SENTINEL), "site": np.full((4, n), SENTINEL), "nn": np.full((4, n, n), SENTINEL), "zn": np.full((2, n, n), SENTINEL),
           "zz": np.full((n, n), SENTINEL), "hop": np.full((2, n, n), z), "ee": np.full((n, n), z), "ll": np.full((n, n), z), "le": np.full((n, n), z)}
    p = [(_ptr(out[k]) if k in want else None) for k in GROUPS]
    _lib.check(_lib.lib().qbh_corr_kondo_dev(n, ne, tz, None if real else _addr(t), _addr(t) if real else None, _ptr(out["norm2"]), *p, None),
               "qbh_corr_kondo_dev")
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


def _check_structure(got, real):
    """what the host fills: the mirrors and the diagonals"""
    n2 = got["norm2"][0]
    herm = lambda a: np.array_equal(a, np.conj(np.swapaxes(a, -1, -2)))
    assert herm(got["hop"]) and herm(got["ee"]) and herm(got["ll"]) and np.array_equal(got["zz"], got["zz"].T)
    assert np.array_equal(got["nn"][0], got["nn"][0].T) and np.array_equal(got["nn"][3], got["nn"][3].T) and np.array_equal(got["nn"][1], got["nn"][2].T)
    d = lambda a: np.diagonal(a, axis1=-2, axis2=-1)
    assert np.array_equal(d(got["hop"]), got["site"][0:2]) and np.array_equal(d(got["zz"]), np.full(len(got["zz"]), 0.25 * n2))
    assert np.array_equal(d(got["ee"]), got["site"][0] - got["site"][2]) and np.array_equal(d(got["ll"]), 0.5 * n2 + got["site"][3])
    if real:
        assert all(np.all(got[k].imag == 0) for k in ("hop", "ee", "ll", "le"))


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
@pytest.mark.parametrize("shape,dim", SHAPES, ids=lambda s: "n%d_e%d_z%d" % s if isinstance(s, tuple) else None)
def test_every_entry_against_the_reference(shape, dim, real):
    assert kondo.sector_dim(*shape) == dim
    x, want = _case(shape, real)
    got = _raw(shape, _dev(x))
    ref.compare("kondo %s %s" % (shape, "real" if real else "complex"), got, want, dim)
    _check_structure(got, real)
    if dim == 1:
        off = ~np.eye(shape[0], dtype=bool)
        assert all(np.all(got[k][..., off] == 0) for k in ("hop", "ee", "ll", "le"))


def _grid(dim):
    """corr_grid for this kernel: (workgroups along x, rows of one trip)"""
    lds = (2 * 22 * 22 + 256 * (TILE // 256 + 1)) * 8
    per_cu = max(1, min(4, (158 * 1024) // (lds + 2048)))
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    gx = max(1, min((dim + TILE - 1) // TILE, ncu * per_cu))
    return gx, gx * TILE


@functools.lru_cache(maxsize=None)
def _big_case(real):
    dim = kondo.sector_dim(*BIG)
    _, trip = _grid(dim)
    x = _rand(dim, 99)
    rng = np.random.default_rng(5)
    keep = rng.random(dim) < 1.0 / 200
    for lo, hi in ((0, TILE + 100), (trip - TILE - 100, trip + TILE + 100), (dim - TILE - 100, dim)):
        keep[max(lo, 0):min(hi, dim)] = True
    x[~keep] = 0.0
    if real:
        x = np.ascontiguousarray(x.real)
    return x, ref.correlations(*BIG, x), int(keep.sum())


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_the_large_case_takes_more_than_one_trip(real):
    dim = kondo.sector_dim(*BIG)
    assert dim == 5280932
    gx, trip = _grid(dim)
    print("grid %d workgroups x %d rows = %d rows a trip, dim %d" % (gx, TILE, trip, dim))
    assert trip < dim                                                   # rows beyond one trip of the grid actually used
    x, want, nnz = _big_case(real)
    got = _raw(BIG, _dev(x))
    ref.compare("kondo %s %s (%d nonzero rows)" % (BIG, "real" if real else "complex", nnz), got, want, nnz)
    _check_structure(got, real)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_null_groups_and_repeatability(real):
    shape = (5, 3, 2)
    x, _ = _case(shape, real)
    t = _dev(x)
    full, again = _raw(shape, t), _raw(shape, t)
    assert all(_same_bits(full[k], again[k]) for k in full)                     # two calls: the same bits
    for want in [(k,) for k in GROUPS] + [(), ("site", "nn", "zz"), ("hop", "le"), ("zn", "ee", "ll")]:
        part = _raw(shape, t, want)
        assert _same_bits(part["norm2"], full["norm2"])
        for k in GROUPS:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)                  # the other outputs keep their bits
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)  # a group that was not asked for: untouched


def _handle(n, ne, tz):
    """a handle of the sector, for dotc on its vectors"""
    return q.csr_mat.kondo(n, ne, tz, lattices.chain(n), matrix_free=True)


def test_signs_and_conjugation_against_the_site_operators_and_dotc():
    """hop, ee, ll and le for single (i, j) with i < j, i > j and i = j against <O_i psi | O_j psi> from two moprXvec_kondo results
    (the coefficient a unit vector) and dotc"""
    shape = (4, 4, 0)
    n, ne, tz = shape
    x, _ = _case(shape, False)
    t = _dev(x)
    got = _raw(shape, t)
    tol = 2.0 * ref.bound(len(x), float(np.sum(np.abs(x) ** 2)))         # both routes round
    unit = lambda k: np.eye(n, dtype=np.complex128)[k].copy()
    pairs = [(0, 1), (1, 3), (0, 3), (2, 0), (3, 1), (3, 0), (0, 0), (2, 2), (3, 3)]
    # (array, op, which coefficient set the left / right factor takes: 0 = coef_elec, 1 = coef_spin)
    checks = [(got["hop"][0], kondo.C_UP, 0, 0), (got["hop"][1], kondo.C_DN, 0, 0), (got["ee"], kondo.SPIN_MINUS, 0, 0),
              (got["ll"], kondo.SPIN_MINUS, 1, 1), (got["le"], kondo.SPIN_MINUS, 1, 0)]
    names = ["hop_up", "hop_dn", "ee", "ll", "le"]
    for name, (arr, op, left, right) in zip(names, checks):
        te, ts = kondo.mopr_target(ne, tz, op)
        H = _handle(n, te, ts)
        dim_new = kondo.sector_dim(n, te, ts)
        yl = torch.zeros(dim_new, dtype=torch.complex128, device="cuda")
        yr = torch.zeros(dim_new, dtype=torch.complex128, device="cuda")
        for i, j in pairs:
            sets = lambda which, k: (unit(k), None) if which == 0 else (None, unit(k))
            assert q.moprXvec_kondo(n, ne, tz, op, *sets(left, i), _addr(t), _addr(yl)) == (len(x), dim_new)
            assert q.moprXvec_kondo(n, ne, tz, op, *sets(right, j), _addr(t), _addr(yr)) == (len(x), dim_new)
            val = H.dotc(_addr(yl), _addr(yr))
            print("%s[%d][%d] %r  site operators + dotc %r" % (name, i, j, arr[i, j], val))
            assert abs(arr[i, j] - val) <= tol, (name, i, j)
        H.destroy()


def _energy_by_spmv(M, x):
    v = M.vec(2)
    v.upload(np.asarray(x, dtype=np.complex128), 0)
    M.spmv(v.at(0), v.at(M.dim), 1.0, 0.0, 0.0)
    e = M.dotc(v.at(0), v.at(M.dim))
    v.free()
    return e


def _random_terms(n, seed, real):
    """all-pairs Hermitian hops, random kz, kxy, bz, bxy and U; the sum of the moduli of the coefficients that meet a correlation"""
    rng = np.random.default_rng(seed)
    cplx = lambda: complex(rng.uniform(-1, 1), 0.0 if real else rng.uniform(-1, 1))
    hops, weight = [], 0.0
    for i in range(n):
        hops.append((i, i, rng.uniform(-1, 1), rng.uniform(-1, 1)))
        weight += abs(hops[-1][2]) + abs(hops[-1][3])
        for j in range(i + 1, n):
            a, b = cplx(), cplx()
            hops += [(i, j, a, b), (j, i, np.conj(a), np.conj(b))]
            weight += 2.0 * (abs(a) + abs(b))
    kz, kxy = rng.uniform(-2, 2, size=n), rng.uniform(-2, 2, size=n)
    sb = [(i, j, rng.uniform(-1, 1), rng.uniform(-1, 1)) for i in range(n) for j in range(i + 1, n)]
    U = float(rng.uniform(0.5, 2.0))
    weight += float(np.sum(np.abs(kz)) + np.sum(np.abs(kxy))) + sum(abs(b[2]) + abs(b[3]) for b in sb) + U * n
    return kondo.Terms(hops, list(kz), list(kxy), sb), U, weight


@functools.lru_cache(maxsize=None)
def _dense_big():
    return _rand(kondo.sector_dim(*BIG), 1234)


def test_dense_large_sector_flip_norm_against_the_site_operator():
    """|| sum_s (a_s S^-_s + b_s s^-_s) psi ||^2 from one moprXvec_kondo call against the quadratic form of ll, ee and le"""
    n, ne, tz = BIG
    x = _dense_big()
    t = _dev(x)
    c = q.kondo_correlations(n, ne, tz, t, normalize=False, want=("dens", "docc", "sz_local", "pm_ee", "pm_ll", "pm_le"))
    n2 = float(np.sum(np.abs(x.astype(np.clongdouble)) ** 2).real)
    te, ts = kondo.mopr_target(ne, tz, kondo.SPIN_MINUS)
    H = _handle(n, te, ts)
    y = torch.zeros(kondo.sector_dim(n, te, ts), dtype=torch.complex128, device="cuda")
    rng = np.random.default_rng(17)
    for trial in range(2):
        a = rng.normal(size=n) + 1j * rng.normal(size=n)                 # on S^-_s
        b = rng.normal(size=n) + 1j * rng.normal(size=n)                 # on s^-_s
        q.moprXvec_kondo(n, ne, tz, kondo.SPIN_MINUS, b, a, _addr(t), _addr(y))
        lhs = H.dotc(_addr(y), _addr(y))
        rhs = np.conj(a) @ c["pm_ll"] @ a + np.conj(b) @ c["pm_ee"] @ b + 2.0 * (np.conj(a) @ c["pm_le"] @ b).real
        weight = (np.sum(np.abs(a)) + np.sum(np.abs(b))) ** 2
        tol = 2.0 * weight * ref.bound(len(x), n2)
        print("flip norm %d: site operator %.15g, quadratic form %.15g, |diff| / bound %.3g" % (trial, lhs.real, rhs.real, abs(lhs.real - rhs.real) / tol))
        assert abs(lhs.real - rhs.real) <= tol and abs(rhs.imag) <= tol
    H.destroy()


def test_dense_large_sector_energy_identity_complex_and_real():
    """<x| H |x> from the correlations equals spmv + dotc of the matrix-free operator: complex terms and vector, then real terms
    with the packed-real vector, which also agrees with the complex route on the same numbers"""
    n, ne, tz = BIG
    x = _dense_big()
    n2 = float(np.sum(np.abs(x.astype(np.clongdouble)) ** 2).real)
    T, U, weight = _random_terms(n, 23, real=False)
    M = q.csr_mat.kondo(n, ne, tz, None, U=U, terms=T, matrix_free=True)
    want = _energy_by_spmv(M, x)
    M.destroy()
    got = q.kondo_energy_from_correlations(q.kondo_correlations(n, ne, tz, _dev(x), normalize=False), T, U=U)
    tol = 2.0 * weight * ref.bound(len(x), n2)
    print("complex: E from correlations %.15g, spmv + dotc %.15g, |diff| / bound %.3g" % (got, want.real, abs(got - want.real) / tol))
    assert abs(got - want.real) <= tol and abs(want.imag) <= tol
    xr = np.ascontiguousarray(x.real)
    n2 = float(np.sum(xr.astype(np.longdouble) ** 2))
    T, U, weight = _random_terms(n, 29, real=True)
    M = q.csr_mat.kondo(n, ne, tz, None, U=U, terms=T, matrix_free=True)
    want = _energy_by_spmv(M, xr)
    M.destroy()
    got_r = q.kondo_energy_from_correlations(q.kondo_correlations(n, ne, tz, _dev(xr), real=True, normalize=False), T, U=U)
    got_c = q.kondo_energy_from_correlations(q.kondo_correlations(n, ne, tz, _dev(xr.astype(np.complex128)), normalize=False), T, U=U)
    tol = 2.0 * weight * ref.bound(len(x), n2)
    print("real: E from correlations %.15g (packed real) %.15g (complex route), spmv + dotc %.15g, |diff| / bound %.3g %.3g" % (
        got_r, got_c, want.real, abs(got_r - want.real) / tol, abs(got_r - got_c) / tol))
    assert abs(got_r - want.real) <= tol and abs(got_r - got_c) <= tol and abs(want.imag) <= tol


def test_the_reference_chain_end_to_end():
    """the reference's L = 4 chain (periodic, t = 1, J_K = 4, n_elec = 4): ground state by a dense eigh of the downloaded operator,
    its energy from the correlations, S_tot^2 = 0 and the same Kondo singlet <S_i . s_i> on every site"""
    with open(os.path.join(os.path.dirname(__file__), "golden", "kondo_reference_answers.json")) as f:
        gold = json.load(f)["chain_L4_all_sz"]
    L, ne = gold["L"], gold["n_elec"]
    bonds = lattices.chain(L)
    A = q.csr_mat.kondo(L, ne, 0, bonds, t=gold["t"], J_K=gold["J_K"])
    assert A.dim == 346
    ia, ja, val = A.download()
    A.destroy()
    H = np.zeros((346, 346), dtype=np.complex128)
    np.add.at(H, (np.repeat(np.arange(346), np.diff(ia)), ja), val)
    assert np.abs(H.imag).max() == 0 and np.abs(H - H.T).max() == 0
    ev, vecs = np.linalg.eigh(H.real)
    psi = vecs[:, 0]
    T = kondo.terms(L, bonds, t=gold["t"], J_K=gold["J_K"])
    for real in (False, True):
        c = q.kondo_correlations(L, ne, 0, _dev(psi if real else psi.astype(np.complex128)), real=real)
        e = q.kondo_energy_from_correlations(c, T)
        singlet = np.diag(c["ss_le"])
        print("Kondo chain L = 4, J_K = 4 (%s): E %.10f (eigh %.10f), <S_i . s_i> %s, S_tot^2 %.3e, <S_0 . S_1> %.10f, docc %.10f" % (
            "packed real" if real else "complex", e, ev[0], np.array2string(singlet, precision=12), c["total_spin"], c["ss_ll"][0, 1], c["docc"][0]))
        assert abs(e - gold["E0"]) < 1e-8 and abs(e - ev[0]) < 1e-10
        # S_tot^2 sums 3 N^2 <S . S> entries, each of up to five raw ones (S_tot^2 psi = 0: second order in the eigenvector's error)
        assert abs(c["total_spin"]) <= 15 * L * L * ref.bound(346, 1.0)
        assert np.ptp(singlet) < 1e-12                                   # equal on all sites
        assert abs(c["norm2"] - 1.0) < 1e-13
