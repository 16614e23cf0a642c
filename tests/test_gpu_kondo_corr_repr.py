"""qbh_corr_kondo_repr_dev (all-pair correlations of a Kondo-lattice momentum-sector state) entry by entry against
tests/kondocorrreprref.py (the longdouble reference from representatives, pinned on the CPU by tests/test_kondocorrreprref.py against
unfolded states), on random vectors that are not normalised and carry garbage at the zero-norm representatives, complex and -- at
real characters -- packed-real, with every output buffer pre-filled with a sentinel.

Bound for every entry of every array:  |got - want| <= (dim |G| + C_ROUND) 2^-53 A,  A = the sum of the absolute values of the
terms of the entry (from the reference), C_ROUND = 10 derived in the reference's docstring.  Entries with A = 0 must vanish exactly.
The numbers of representatives and of zero-norm representatives below were computed on the CPU with kondoops.Momentum.

Worst |got - want| / bound per group over all entry-by-entry cases (complex and packed real), as measured:
    norm2 0.037  site 0.035  nn 0.035  zn 0.035  zz 0.037  hop 0.035  ee 0.035  ll 0.035  le 0.0029
(the largest ones at the sectors of one and four representatives; 0.0084 at most from 36 representatives on)"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import kondocorrref as kc
import kondocorrreprref as kr
import kondoops as ko
import quantum_basis_amd as q
from quantum_basis_amd import _lib, kondo

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e300
KEYS = kr.KEYS
GROUPS = KEYS[1:]
WHO = "qbh_corr_kondo_repr_dev"
U53 = 2.0 ** -53

CASES = {
    # name: (n_sites, n_elec, two_sz, (perms, turns), real characters, representatives, zero-norm representatives or None)
    "ring4_2_k0": (4, 2, 0, kr.ring(4, 0), True, 36, None),
    "ring4_2_k1": (4, 2, 0, kr.ring(4, 1), False, 36, None),
    "ring4_4_k2": (4, 4, 0, kr.ring(4, 2), True, 90, None),
    "ring6_6_k0": (6, 6, 0, kr.ring(6, 0), True, 2544, 20),
    "ring6_6_k1": (6, 6, 0, kr.ring(6, 1), False, 2544, 6),
    "ring6_6_k3": (6, 6, 0, kr.ring(6, 3), True, 2544, 0),
    "ring6_4_z2_k2": (6, 4, 2, kr.ring(6, 2), False, 1129, None),
    "torus3x2_k00": (6, 3, 1, kr.torus(3, 2, 0, 0), True, 595, None),          # two generators
    "torus3x2_k11": (6, 3, 1, kr.torus(3, 2, 1, 1), False, 595, None),
    "dihedral6_trivial": (6, 4, 0, kr.dihedral(6, False), True, 714, 36),
    "dihedral6_sign": (6, 4, 0, kr.dihedral(6, True), True, 714, 12),          # classes that are their own mirror
    "no_symmetry": (5, 3, 0, kr.identity(5), True, 1100, None),                # n_trans = 1: 10 classes, 25 ordered orbits, 5 site orbits
    "ring6_empty_band": (6, 0, 0, kr.ring(6, 0), True, 4, None),               # hop, ee, le exactly 0
    "ring6_full_band": (6, 12, 0, kr.ring(6, 0), True, 4, None),
    "ring6_one_dead": (6, 6, 12, kr.ring(6, 0), True, 1, 1),                   # the only representative has zero norm: all outputs 0
    "ring6_one_live": (6, 6, 12, kr.ring(6, 3), True, 1, 0),
    "ring10_2_k3": (10, 2, 0, kr.ring(10, 3), False, 4420, None),
    "ring12_2_z2_k5": (12, 2, 2, kr.ring(12, 5), False, 17326, None),          # 12 elements, complex
    "torus4x4_k12": (16, 2, 12, kr.torus(4, 4, 1, 2), False, 6240, None),      # 16 elements, 48-bit words
    "ring21_k4": (21, 1, -18, kr.ring(21, 4), False, 231, None),               # s in bits 42 .. 62; 50,752 B of tables: 1024 lanes
    "ring21_dihedral_sign": (21, 1, -18, kr.dihedral(21, True), True, 121, 11),      # 42 elements
    "ring8_8_k4": (8, 8, 0, kr.ring(8, 4), None, 92442, None),                 # complex only; several workgroups per CU
}
IDS = sorted(CASES)
REAL_IDS = [n for n in IDS if CASES[n][4]]
WORST = {}                                                   # group -> worst ratio over the entry-by-entry cases that have run


def _chars(turns):
    """the characters handed to the library: the exact ones rounded to double"""
    return ko.chars_of(turns)


@functools.lru_cache(maxsize=None)
def _case(name, real):
    """(host vector, reference) -- computed once, shared, never modified"""
    n, ne, tz, (perms, turns) = CASES[name][:4]
    dim = ko.Momentum(ko.Sector(n, ne, tz), perms, turns).dim
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = ((rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 1.3).astype(np.complex128)
    if real:
        x = np.ascontiguousarray(x.real)
    x.setflags(write=False)
    return x, kr.kondo_repr(n, ne, tz, perms, turns, x, chars=_chars(turns))


def _dev(x):
    t = torch.from_numpy(np.array(x)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _addr(t):
    return C.c_void_p(t.data_ptr())


def _raw_args(N, ne, tz, perms, chars, t, want=KEYS):
    real = t.dtype == torch.float64
    p, c = np.ascontiguousarray(perms, dtype=np.int32), np.ascontiguousarray(chars, dtype=np.complex128)
    z = SENTINEL + 1j * SENTINEL
    out = {"norm2": np.full(1, SENTINEL), "site": np.full((4, N), SENTINEL), "nn": np.full((4, N, N), SENTINEL),
           "zn": np.full((2, N, N), SENTINEL), "zz": np.full((N, N), SENTINEL), "hop": np.full((2, N, N), z), "ee": np.full((N, N), z),
           "ll": np.full((N, N), z), "le": np.full((N, N), z)}
    a = [(_ptr(out[k]) if k in want else None) for k in GROUPS]
    dim = C.c_int64(-1)
    _lib.check(_lib.lib().qbh_corr_kondo_repr_dev(N, ne, tz, len(p), _ptr(p), _ptr(c), None if real else _addr(t),
                                                  _addr(t) if real else None, _ptr(out["norm2"]), *a, C.byref(dim), None), WHO)
    out["dim"] = dim.value
    return out


def _raw(name, t, want=KEYS):
    n, ne, tz, (perms, turns) = CASES[name][:4]
    return _raw_args(n, ne, tz, perms, _chars(turns), t, want)


def _full_call(n, ne, tz, t):
    """qbh_corr_kondo_dev on a full-sector vector"""
    real = t.dtype == torch.float64
    z = SENTINEL + 1j * SENTINEL
    out = {"norm2": np.full(1, SENTINEL), "site": np.full((4, n), SENTINEL), "nn": np.full((4, n, n), SENTINEL), "zn": np.full((2, n, n), SENTINEL),
           "zz": np.full((n, n), SENTINEL), "hop": np.full((2, n, n), z), "ee": np.full((n, n), z), "ll": np.full((n, n), z), "le": np.full((n, n), z)}
    _lib.check(_lib.lib().qbh_corr_kondo_dev(n, ne, tz, None if real else _addr(t), _addr(t) if real else None, _ptr(out["norm2"]),
                                             *[_ptr(out[k]) for k in GROUPS], None), "qbh_corr_kondo_dev")
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
    assert np.array_equal(d(got["nn"][0]), got["site"][0]) and np.array_equal(d(got["nn"][1]), got["site"][2])
    if real:
        assert all(np.all(got[k].imag == 0) for k in ("hop", "ee", "ll", "le"))


def _entry_by_entry(name, real):
    n, ne, tz, (perms, turns), _, dim, n_zero = CASES[name]
    x, ref = _case(name, real)
    assert ref["dim"] == dim == len(x)                       # the counts computed on the CPU
    if n_zero is not None:
        assert int(ref["zero"].sum()) == n_zero
    got = _raw(name, _dev(x))
    assert got["dim"] == dim
    worst = kr.compare("%s %s" % (name, "packed real" if real else "complex"), got, ref, len(perms))
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("worst so far  %s" % "  ".join("%s %.3g" % kv for kv in WORST.items()))
    _check_structure(got, real)
    return got


@pytest.mark.parametrize("name", IDS)
def test_every_entry_against_the_reference_complex(name):
    got = _entry_by_entry(name, False)
    zero = lambda a: np.all(np.ascontiguousarray(a).view(np.float64) == 0)
    off = ~np.eye(CASES[name][0], dtype=bool)
    if name in ("ring6_empty_band", "ring6_full_band"):      # nothing can hop, no electron spin can turn
        assert zero(got["hop"][:, off]) and zero(got["ee"][off]) and zero(got["le"])
    if name == "ring6_one_dead":
        assert all(zero(got[k]) for k in KEYS)
    if name == "ring6_one_live":
        n2 = got["norm2"][0]                                 # all six sites hold an up electron, all local spins are up
        assert n2 > 0 and np.allclose(got["site"][0], n2, rtol=1e-15, atol=0) and np.allclose(got["site"][3], 0.5 * n2, rtol=1e-15, atol=0)


@pytest.mark.parametrize("name", REAL_IDS)
def test_every_entry_against_the_reference_packed_real(name):
    got = _entry_by_entry(name, True)
    assert all(np.array_equal(got[k], np.swapaxes(got[k], -1, -2)) for k in ("hop", "ee", "ll"))


def test_packed_real_needs_real_characters():
    x, _ = _case("ring6_6_k1", True)
    with pytest.raises(_lib.QbhError) as e:
        _raw("ring6_6_k1", _dev(x))
    assert e.value.code == -1 and "real characters" in str(e.value)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_no_symmetry_equals_the_full_space_call(real):
    """n_trans = 1: the representatives are the whole sector in its own order, so qbh_corr_kondo_dev measures the same vector.
    Within the sum of both bounds."""
    n, ne, tz, (perms, turns) = CASES["no_symmetry"][:4]
    x, ref = _case("no_symmetry", real)
    assert kondo.sector_dim(n, ne, tz) == len(x)
    t = _dev(x)
    a, b = _raw("no_symmetry", t), _full_call(n, ne, tz, t)
    for k in KEYS:
        tol = kr.tolerance(ref, 1, k) + kc.bound(len(x), float(ref["norm2"]))
        err = np.abs(np.asarray(a[k]) - np.asarray(b[k]).reshape(np.asarray(a[k]).shape))
        print("%s: worst |sector call - full call| / (sum of both bounds) %.3g" % (k, float(np.max(err / tol))))
        assert np.all(err <= tol), k


@pytest.mark.parametrize("name,real", [("ring6_6_k1", False), ("dihedral6_sign", True), ("ring21_k4", False), ("no_symmetry", True)])
def test_null_groups_and_repeatability(name, real):
    x, _ = _case(name, real)
    t = _dev(x)
    full, again = _raw(name, t), _raw(name, t)
    assert all(_same_bits(full[k], again[k]) for k in KEYS)                     # two calls: the same bits
    wants = [("norm2", g) for g in GROUPS] + [tuple(k for k in KEYS if k != g) for g in GROUPS] + [("norm2",), ("norm2", "zn", "le")]
    for want in wants:                                                          # each group alone, each group left out
        part = _raw(name, t, want)
        for k in KEYS:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)                  # a NULL group changes no other output
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)  # ... and is not written
        assert part["dim"] == full["dim"]


@pytest.mark.parametrize("name", ["ring6_6_k0", "dihedral6_trivial", "dihedral6_sign"])
def test_entries_at_zero_norm_representatives_are_never_read(name):
    x, ref = _case(name, False)
    zero = ref["zero"]
    assert zero.any()
    clean = np.array(x)
    clean[zero] = 0.0
    loud = np.array(x)
    loud[zero] = np.nan * (1 + 1j)
    a, b, c = _raw(name, _dev(x)), _raw(name, _dev(clean)), _raw(name, _dev(loud))
    assert all(_same_bits(a[k], b[k]) and _same_bits(a[k], c[k]) for k in KEYS)
    assert all(np.all(np.isfinite(c[k].view(np.float64))) for k in KEYS)


# ---- the energy identity: <x| H |x> from the correlations against spmv + dotc of qbh_mf_kondo_repr ----
def _chain_terms(L):
    """hops, anisotropic kz / kxy and local-spin bonds to the first and second neighbours, as test_anisotropic_couplings_and_local_
    spin_bonds of tests/test_gpu_kondo_repr_mf.py; returns the terms and the sum of the moduli of their coefficients"""
    bonds = ko.chain(L)
    sb = [(i, (i + 1) % L, 0.4, 0.9) for i in range(L)] + [(i, (i + 2) % L, 0.2, -0.3) for i in range(L)]
    T = kondo.Terms(kondo.hop_terms(bonds, 1.0), [0.7] * L, [1.9] * L, sb)
    weight = sum(abs(h[2]) + abs(h[3]) for h in T.hops) + L * (0.7 + 1.9) + sum(abs(b[2]) + abs(b[3]) for b in sb)
    return T, float(weight)


def _energy_identity(L, ne, tz, m, x, U=1.3):
    """(E from the raw correlations, Re dotc(x, H x), the bound, the raw correlations).  x must vanish at the zero-norm
    representatives: their decoupled rows keep a diagonal of their own, which enters dotc and no correlation.  Bound: the energy sums `weight` worth
    of entries, each within (dim |G| + C_ROUND) 2^-53 A with A <= norm2; on the other side a row of the matrix-free apply is a sum
    of at most kKondoMaxRow = 160 products (4 (160 + 4) 2^-53 weight |x_i| per row, tests/test_gpu_kondo_repr_mf.py) and dotc a
    sum of dim products ((dim + 8) 2^-53)."""
    perms, turns = ko.chain_group(L, m)
    T, weight = _chain_terms(L)
    weight += U * L
    M = q.csr_mat.kondo_repr(L, ne, tz, None, perms, _chars(turns), U=U, terms=T, fake_pos=0.0, matrix_free=True)
    assert M.dim == len(x)
    v = M.vec(2)
    v.upload(np.asarray(x, dtype=np.complex128), 0)
    M.spmv(v.at(0), v.at(M.dim), 1.0, 0.0, 0.0)
    want = M.dotc(v.at(0), v.at(M.dim))
    c = q.kondo_repr_correlations(L, ne, tz, perms, _chars(turns), v.at(0), normalize=False)
    v.free()
    M.destroy()
    got = q.kondo_energy_from_correlations(c, T, U=U)
    tol = weight * c["norm2"] * U53 * ((len(x) * len(perms) + kr.C_ROUND) + 4 * (160 + 4) + (len(x) + 8))
    return got, want, tol, c


@pytest.mark.parametrize("m", range(6))
def test_energy_identity_at_every_momentum_of_ring_6(m):
    perms, turns = ko.chain_group(6, m)
    mo = ko.Momentum(ko.Sector(6, 6, 0), perms, turns)
    assert mo.dim == 2544
    rng = np.random.default_rng(600 + m)
    x = (rng.normal(size=2544) + 1j * rng.normal(size=2544)) * 1.3
    x[mo.zero] = 0.0
    got, want, tol, _ = _energy_identity(6, 6, 0, m, x)
    print("ring 6, k = %d: E from correlations %.15g, dotc(x, Hx) %.15g %+.3gi, |diff| / bound %.3g" % (
        m, got, want.real, want.imag, abs(got - want.real) / tol))
    assert abs(got - want.real) <= tol and abs(want.imag) <= tol


def test_more_representatives_than_one_trip_of_the_resident_grid():
    """Chain L = 10, n_elec = 8, S^z = 0, k = 0 (the case of tests/test_gpu_kondo_repr_mf.py): about 2.6e6 representatives, more
    than CUs x 4 x 256, so every lane walks its grid-stride loop several times.  No longdouble reference at this size: the sum
    rules of the sector, <S_tot^2> >= 0 and the energy identity."""
    L, ne, tz = 10, 8, 0
    perms, turns = ko.chain_group(L, 0)
    M = q.csr_mat.kondo_repr(L, ne, tz, None, perms, _chars(turns), terms=_chain_terms(L)[0], fake_pos=0.0, matrix_free=True)
    dim = M.dim
    M.destroy()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2.5e6 < dim < 2.8e6 and dim > cus * 4 * 256
    rng = np.random.default_rng(1008)
    x = (rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 1.3
    got, want, tol, c = _energy_identity(L, ne, tz, 0, x)
    n2 = c["norm2"]
    # every representative of this sector is live (norm2 is the whole weight of x), so no decoupled row enters dotc
    assert c["dim"] == dim and abs(n2 - float(np.sum(np.abs(x) ** 2))) <= (dim + kr.C_ROUND) * U53 * n2
    print("ring 10 (8, 0), k = 0: dim %d, E from correlations %.15g, dotc(x, Hx) %.15g, |diff| / bound %.3g" % (
        dim, got, want.real, abs(got - want.real) / tol))
    assert abs(got - want.real) <= tol and abs(want.imag) <= tol
    entry = (dim * L + kr.C_ROUND) * U53 * n2                                    # the bound of one entry with A <= norm2
    n_tot, sz_tot = float(np.sum(c["dens"])), float(np.sum(c["sz_local"]) + np.sum(c["sz_elec"]))
    print("sum rules: sum n / norm2 - n_elec = %.3g, sum S^z / norm2 - S^z = %.3g, <S_tot^2> / norm2 = %.6g" % (
        n_tot / n2 - ne, sz_tot / n2 - 0.5 * tz, c["total_spin"] / n2))
    assert abs(n_tot - ne * n2) <= 2 * L * entry and abs(sz_tot - 0.5 * tz * n2) <= 3 * L * entry
    assert c["total_spin"] >= 0.0


def test_sector_ground_state_against_the_full_space_call():
    """The ground state of the chain model (t = 1, J_K = 1.1) in the sector k = pi of ring 6 (6, 0) by Lanczos and CG, measured
    in the sector, against qbh_corr_kondo_dev on the state unfolded on the host (kondoops.Momentum.expand, rounded to double).
    Within both bounds; the 4 (.. + 4) of the full call's bound also holds the rounding of the unfolded vector and of the
    characters to double (3 x 2^-53 norm2)."""
    n, ne, tz, (perms, turns) = CASES["ring6_6_k3"][:4]
    T = kondo.terms(n, ko.chain(n), 1.0, 1.1)
    M = q.csr_mat.kondo_repr(n, ne, tz, None, perms, _chars(turns), terms=T, fake_pos=100.0)      # the stored sector operator
    dim, maxit = M.dim, 400
    assert dim == 2544
    hess = np.zeros(2 * maxit)
    v = np.zeros(2 * dim, dtype=np.complex128)
    v[:dim] = q.vec_randomize(M, seed=1)
    steps = q.lanczos(0, maxit - 1, maxit, dim, M, v, hess, "sr_val0")
    e0 = q.hess_eigen(hess, maxit, steps, "sr")[0][0]
    vs = [np.array(q.vec_randomize(M, seed=1))] + [np.zeros(dim, dtype=np.complex128) for _ in range(3)]
    q.eigenvec_CG(dim, 1000, 0, M, e0, *vs)
    M.destroy()
    psi = vs[0]
    mo = ko.Momentum(ko.Sector(n, ne, tz), perms, turns)
    assert not mo.zero.any()
    full = mo.expand(psi.astype(kr.CLD)).astype(np.complex128)
    a, b = _raw("ring6_6_k3", _dev(psi)), _full_call(n, ne, tz, _dev(full))
    ref = kr.kondo_repr(n, ne, tz, perms, turns, psi, chars=_chars(turns))
    e = q.kondo_energy_from_correlations({"hop": a["hop"], "docc": a["site"][2], "zz_le": 0.5 * (a["zn"][0] - a["zn"][1]), "pm_le": a["le"],
                                          "zz_ll": a["zz"], "pm_ll": a["ll"]}, T) / a["norm2"][0]
    print("ground state of ring 6 at k = pi: E0 %.12f (Lanczos), %.12f (correlations)" % (e0, e))
    assert abs(e - e0) < 1e-8
    for k in KEYS:
        tol = kr.tolerance(ref, len(perms), k) + kc.bound(len(full), float(ref["norm2"]))
        err = np.abs(np.asarray(a[k]) - np.asarray(b[k]).reshape(np.asarray(a[k]).shape))
        print("%s: worst |sector call - full call on the unfolded state| / (sum of both bounds) %.3g" % (k, float(np.max(err / tol))))
        assert np.all(err <= tol), k


def test_python_wrapper():
    name = "ring6_6_k1"
    n, ne, tz, (perms, turns) = CASES[name][:4]
    x, ref = _case(name, False)
    t = _dev(x)
    raw = q.kondo_repr_correlations(n, ne, tz, perms, _chars(turns), t, normalize=False)
    nrm = q.kondo_repr_correlations(n, ne, tz, perms, _chars(turns), t)
    low = _raw(name, t)
    assert raw["dim"] == nrm["dim"] == 2544 and raw["norm2"] == nrm["norm2"] == low["norm2"][0]
    assert _same_bits(raw["dens"], low["site"][:2]) and _same_bits(raw["docc"], low["site"][2]) and _same_bits(raw["sz_local"], low["site"][3])
    for k, l in (("nn", "nn"), ("zn", "zn"), ("zz_ll", "zz"), ("hop", "hop"), ("pm_ee", "ee"), ("pm_ll", "ll"), ("pm_le", "le")):
        assert _same_bits(raw[k], low[l]) and _same_bits(nrm[k], low[l] / low["norm2"][0]), k
    for k in ("sz_elec", "zz_le", "zz_ee", "ss_ll", "ss_ee", "ss_le", "total_spin"):
        assert k in raw and k in nrm
    assert np.array_equal(raw["ss_le"], 0.5 * (raw["zn"][0] - raw["zn"][1]) + raw["pm_le"].real)
    assert np.ptp(np.diag(nrm["ss_le"])) == 0.0              # one site orbit on a ring: the same bits on every site
    assert nrm["total_spin"] >= 0.0
    part = q.kondo_repr_correlations(n, ne, tz, perms, _chars(turns), t, normalize=False, want=("pm_le", "zn"))
    assert set(part) == {"norm2", "dim", "pm_le", "zn", "zz_le", "ss_le"} and _same_bits(part["pm_le"], raw["pm_le"])
    with pytest.raises(ValueError):
        q.kondo_repr_correlations(n, ne, tz, perms, _chars(turns), t, want=("flip",))
    # the host helpers take the arrays as they are
    nk = q.momentum_distribution(nrm["hop"], np.arange(n), 2 * np.pi * np.arange(n) / n)
    assert nk.shape == (2, n) and abs(float(np.sum(nk)) - ne) < 1e-9
    sq = q.structure_factor(nrm["ss_ll"], np.arange(n), 2 * np.pi * np.arange(n) / n)
    assert sq.shape == (n,) and np.all(sq > -1e-12)
    # packed real at a real character, and a norm of zero cannot be normalised
    xr, _ = _case("ring6_6_k3", True)
    perms3, turns3 = CASES["ring6_6_k3"][3]
    rr = q.kondo_repr_correlations(n, ne, tz, perms3, _chars(turns3), _dev(xr), real=True)
    assert np.all(rr["pm_le"].imag == 0) and np.all(rr["hop"].imag == 0)
    xd, _ = _case("ring6_one_dead", False)
    pd, td = CASES["ring6_one_dead"][3]
    with pytest.raises(ValueError):
        q.kondo_repr_correlations(6, 6, 12, pd, _chars(td), _dev(xd))
    assert q.kondo_repr_correlations(6, 6, 12, pd, _chars(td), _dev(xd), normalize=False)["norm2"] == 0.0
