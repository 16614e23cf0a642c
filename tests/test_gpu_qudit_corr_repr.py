"""qbh_corr_qudit_repr_dev (all-pair correlations and string order of a d-level momentum-sector state) entry by entry against
tests/quditcorrreprref.py (the longdouble reference from representatives, pinned on the CPU by tests/test_quditcorrreprref.py against
unfolded states), on random vectors that are not normalised and carry garbage at the zero-norm representatives, complex and -- at
real characters -- packed-real, with every output buffer pre-filled with a sentinel.

Bound for every entry of norm2, pop, dd, str and aa:  |got - want| <= (dim |G| + n_sites + 10) 2^-53 A,  A = the sum of the absolute
values of the terms of the entry (from the reference; the constant is derived in the reference's docstring).  Entries with A = 0
must vanish exactly, and so must every imaginary part of a packed-real call."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import corrreprref
import quantum_basis_amd as q
import quditcorrref
import quditcorrreprref as qr
from quantum_basis_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e300
KEYS = qr.KEYS
WHO = "qbh_corr_qudit_repr_dev"


def _tables(d, K, kind="plain"):
    """(diag [K][d] or None, (h, g), lower).  plain: nothing vanishes; zeros: g has a zero and negative entries, lower a zero entry;
    spin: S^z, the den Nijs-Rommelse string and S^+ of spin (d - 1) / 2 (d odd)"""
    rng = np.random.default_rng(1000 + 10 * d + K)
    diag = rng.uniform(-1.5, 1.5, size=(K, d)) if K else None
    if kind == "spin":
        m = (d - 1) / 2.0 - np.arange(d)
        diag = np.concatenate([m[None, :], diag[1:]]) if K else None
        return diag, (m, np.where(np.arange(d) % 2 == ((d - 1) // 2) % 2, 1.0, -1.0)), np.append(0.0, np.sqrt((d - np.arange(1, d)) * np.arange(1, d)))
    h = rng.uniform(0.5, 1.5, size=d) * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    g = rng.uniform(0.6, 1.3, size=d) * np.where(np.arange(d) % 3 == 1, -1.0, 1.0)
    lower = np.append(0.0, rng.uniform(0.5, 1.5, size=d - 1))
    if kind == "zeros":
        g[d // 2] = 0.0
        g[0] = -abs(g[0])
        lower[d - 1] = 0.0
    return diag, (h, g), lower


CASES = {
    # name: (n_sites, d, total, (perms, chars), n_diag, tables)
    "trivial_d3": (6, 3, 6, qr.identity(6), 2, "plain"),
    "dihedral6_minus": (6, 3, 6, qr.dihedral(6, True), 2, "spin"),            # every class its own mirror; zero-norm representatives
    "dihedral8_minus_d4": (8, 4, 9, qr.dihedral(8, True), 1, "plain"),
    "dihedral6_plus": (6, 3, 5, qr.dihedral(6, False), 2, "plain"),
    "cells4x2_k1": (8, 3, 8, qr.cells_chain(4, 2, 1), 2, "plain"),            # rotations by two sites: two site orbits
    "cells4x2_k2": (8, 3, 7, qr.cells_chain(4, 2, 2), 1, "spin"),
    "cells3x3_k1": (9, 3, 8, qr.cells_chain(3, 3, 1), 2, "plain"),            # cells of three sites
    "torus3x2_k11": (6, 3, 6, qr.torus(3, 2, 1, 1), 2, "plain"),              # strings whose images are not intervals
    "torus3x2_k00": (6, 3, 6, qr.torus(3, 2, 0, 0), 4, "spin"),
    "torus4x2_k11": (8, 3, 8, qr.torus(4, 2, 1, 1), 2, "plain"),
    "torus4x2_k20": (8, 3, 7, qr.torus(4, 2, 2, 0), 0, "plain"),
    "ring7_d4_k2": (7, 4, 10, qr.ring(7, 2), 2, "plain"),                     # 2-bit fields full
    "ring6_d4_k3": (6, 4, 9, qr.ring(6, 3), 4, "zeros"),
    "ring6_d5_k1": (6, 5, 11, qr.ring(6, 1), 2, "plain"),                     # 3-bit fields with unused codes
    "ring6_d5_k0": (6, 5, 12, qr.ring(6, 0), 1, "spin"),
    "ring5_d8_k1": (5, 8, 17, qr.ring(5, 1), 2, "plain"),
    "ring5_d8_k0": (5, 8, 18, qr.ring(5, 0), 4, "zeros"),
    "ring8_zeros": (8, 3, 8, qr.ring(8, 0), 2, "zeros"),                      # a zero and negative entries in g, a zero in lower
    "ring8_K0": (8, 3, 8, qr.ring(8, 1), 0, "plain"),                         # n_diag = 0, 1 and 4
    "ring8_K1": (8, 3, 8, qr.ring(8, 3), 1, "plain"),
    "ring8_K4": (8, 3, 8, qr.ring(8, 4), 4, "plain"),
    "ring8_K3": (8, 3, 7, qr.ring(8, 2), 3, "plain"),
    "ring64_d2_bit63": (64, 2, 2, qr.ring(64, 5), 1, "plain"),                # 360 KB of translation tables: read from global memory
    "ring64_d2_bit63_k0": (64, 2, 2, qr.ring(64, 0), 2, "plain"),
    "ring32_d4_bit63": (32, 4, 2, qr.ring(32, 16), 1, "plain"),               # 180 KB of tables: global memory as well
    "ring21_d8_bit63": (21, 8, 2, qr.ring(21, 0), 2, "plain"),                # 118 KB of tables in LDS: one workgroup of 1024 lanes
    "ring21_d8_bit63_k4": (21, 8, 2, qr.ring(21, 4), 1, "plain"),
    "trivial64_d2": (64, 2, 2, qr.identity(64), 4, "plain"),                  # 2016 classes of every kind: several passes of each
    "trivial21_d8": (21, 8, 3, qr.identity(21), 2, "plain"),
    "one_site": (1, 3, 2, qr.identity(1), 2, "plain"),
    "dim1": (6, 3, 0, qr.ring(6, 0), 2, "plain"),
}
for _L in (6, 8):
    for _k in range(_L):
        for _t, _tag in ((_L, "sz0"), (1, "t1"), (2 * _L - 1, "tmax")):
            CASES["spin1_ring%d_%s_k%d" % (_L, _tag, _k)] = (_L, 3, _t, qr.ring(_L, _k), 1, "spin")
IDS = sorted(CASES)
REAL_IDS = [n for n in IDS if np.all(np.abs(np.asarray(CASES[n][3][1]).imag) == 0)]


def _args(name):
    n, d, total, (perms, chars), K, kind = CASES[name]
    diag, string, lower = _tables(d, K, kind)
    return n, d, total, perms, chars, diag, string, lower


@functools.lru_cache(maxsize=None)
def _case(name, real):
    """(host vector, reference) -- computed once, shared, never modified"""
    n, d, total, perms, chars, diag, string, lower = _args(name)
    S = qr.sector(n, d, total, perms, chars)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = ((rng.normal(size=S.dim) + 1j * rng.normal(size=S.dim)) * 1.3).astype(np.complex128)
    if real:
        x = np.ascontiguousarray(x.real)
    x.setflags(write=False)
    return x, qr.qudit_repr(n, d, total, perms, chars, x, diag=diag, string=string, lower=lower)


def _dev(x):
    t = torch.from_numpy(np.array(x)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw(name, t, want=KEYS):
    return _raw_args(*_args(name), t, want)


def _raw_args(N, d, total, perms, chars, diag, string, lower, t, want=KEYS):
    real = t.dtype == torch.float64
    p, c = np.ascontiguousarray(perms, dtype=np.int32), np.ascontiguousarray(chars, dtype=np.complex128)
    f = None if diag is None else np.ascontiguousarray(diag, dtype=np.float64)
    K = 0 if f is None else len(f)
    h, g = (np.ascontiguousarray(v, dtype=np.float64) for v in string)
    low = np.ascontiguousarray(lower, dtype=np.float64)
    out = {"norm2": np.full(1, SENTINEL), "pop": np.full((N, d), SENTINEL), "dd": np.full((K, K, N, N), SENTINEL),
           "str": np.full((N, N), SENTINEL), "aa": np.full((N, N), SENTINEL + 1j * SENTINEL)}
    a = {k: (_ptr(out[k]) if k in want and (k != "dd" or K) else None) for k in out}
    dim = C.c_int64(-1)
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_qudit_repr_dev(N, d, total, len(p), _ptr(p), _ptr(c), None if real else addr, addr if real else None,
                                                  K, _ptr(f), _ptr(h), _ptr(g), _ptr(low), a["norm2"], a["pop"], a["dd"], a["str"],
                                                  a["aa"], C.byref(dim), None), WHO)
    out["dim"] = dim.value
    return out


def _keys(ref):
    return [k for k in KEYS if k in ref]


@pytest.mark.parametrize("name", IDS)
def test_every_entry_against_the_reference_complex(name):
    x, ref = _case(name, False)
    got = _raw(name, _dev(x))
    assert got["dim"] == ref["dim"] == len(x)
    n, n_trans = CASES[name][0], len(CASES[name][3][0])
    qr.compare(name + " complex", got, ref, n_trans, n, _keys(ref))
    assert np.array_equal(got["aa"], got["aa"].conj().T) and np.array_equal(got["str"], got["str"].T)
    if "dd" in ref:
        assert np.array_equal(got["dd"], got["dd"].transpose(1, 0, 3, 2))


@pytest.mark.parametrize("name", REAL_IDS)
def test_every_entry_against_the_reference_packed_real(name):
    x, ref = _case(name, True)
    got = _raw(name, _dev(x))
    assert got["dim"] == ref["dim"]
    qr.compare(name + " packed real", got, ref, len(CASES[name][3][0]), CASES[name][0], _keys(ref))
    assert np.all(got["aa"].imag == 0) and np.array_equal(got["aa"], got["aa"].T)


def test_packed_real_needs_real_characters():
    x, _ = _case("spin1_ring6_sz0_k1", True)
    with pytest.raises(_lib.QbhError) as e:
        _raw("spin1_ring6_sz0_k1", _dev(x))
    assert e.value.code == -1 and "real characters" in str(e.value)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


@pytest.mark.parametrize("name,real", [("spin1_ring8_sz0_k1", False), ("torus4x2_k11", False), ("ring64_d2_bit63_k0", True),
                                       ("ring21_d8_bit63_k4", False), ("trivial21_d8", True)])
def test_null_groups_and_repeatability(name, real):
    x, _ = _case(name, real)
    t = _dev(x)
    full, again = _raw(name, t), _raw(name, t)
    assert all(_same_bits(full[k], again[k]) for k in KEYS)                     # two calls: the same bits
    every = set(KEYS)
    for want in [every - {k} for k in KEYS] + [{k} for k in KEYS] + [{"norm2", "pop", "dd"}, {"str", "aa"}, {"dd", "aa"}, set()]:
        part = _raw(name, t, want)
        for k in KEYS:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)                  # a NULL group changes no other output
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)  # ... and is not written
        assert part["dim"] == full["dim"]


@pytest.mark.parametrize("name", ["dihedral6_minus", "dihedral8_minus_d4", "spin1_ring6_sz0_k1", "cells4x2_k1"])
def test_entries_at_zero_norm_representatives_are_never_read(name):
    x, ref = _case(name, False)
    zero = ref["zero"]
    assert zero.any()
    clean = np.array(x)
    clean[zero] = 0.0
    loud = np.array(x)
    loud[zero] = np.nan * (1 + 1j)
    a, b, c = _raw(name, _dev(x)), _raw(name, _dev(clean)), _raw(name, _dev(loud))
    assert all(np.all(np.isfinite(c[k].view(np.float64))) for k in KEYS)         # NaN at the zero-norm rows: every output still finite
    assert all(_same_bits(a[k], b[k]) and _same_bits(a[k], c[k]) for k in KEYS)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_no_symmetry_equals_the_full_space_call(real):
    """n_trans = 1: the representatives are the whole sector in generator order, and the call must agree with qbh_corr_qudit_dev on
    the same vector within the two calls' bounds added (that call's: quditcorrref.bound)"""
    name = "trivial_d3"
    n, d, total, perms, chars, diag, string, lower = _args(name)
    x, ref = _case(name, real)
    t = _dev(x)
    got = _raw(name, t)
    K = len(diag)
    full = {"norm2": np.zeros(1), "pop": np.zeros((n, d)), "dd": np.zeros((K, K, n, n)), "str": np.zeros((n, n)),
            "aa": np.zeros((n, n), dtype=np.complex128)}
    addr = C.c_void_p(t.data_ptr())
    f, h, g, low = (np.ascontiguousarray(v, dtype=np.float64) for v in (diag, string[0], string[1], lower))
    _lib.check(_lib.lib().qbh_corr_qudit_dev(n, d, total, None if real else addr, addr if real else None, K, _ptr(f), _ptr(h), _ptr(g),
                                             _ptr(low), _ptr(full["norm2"]), _ptr(full["pop"]), _ptr(full["dd"]), _ptr(full["str"]),
                                             _ptr(full["aa"]), None), "qbh_corr_qudit_dev")
    W = quditcorrref.weights(n, diag, string, lower)
    for k in KEYS:
        tol = qr.tolerance(ref, 1, n, k) + quditcorrref.bound(ref["dim"], n, ref["norm2"], W[k])
        err = np.abs(got[k].reshape(np.shape(tol)) - full[k].reshape(np.shape(tol)))
        print("trivial group %s %s: worst |sector call - full-space call| / (sum of bounds) %.3g" % ("real" if real else "complex", k,
                                                                                                     float(np.max(err / tol))))
        assert np.all(err <= tol), k


@pytest.mark.parametrize("n,n_dn,sym,real", [(10, 5, qr.ring(10, 1), False), (10, 4, qr.ring(10, 5), True), (8, 4, qr.dihedral(8, True), True),
                                             (8, 3, qr.torus(4, 2, 1, 1), False)])
def test_two_levels_equal_the_spin_half_sector_call(n, n_dn, sym, real):
    """d = 2, level 1 = bit set = spin down, lower = {0, 1}, diag = (S^z,): aa against pm, dd against zz and pop against sz of
    qbh_corr_spin_repr_dev on the same vector, within the two calls' bounds added ((dim |G| + 8) 2^-53 A for that call)"""
    perms, chars = sym
    S = qr.sector(n, 2, n_dn, perms, chars)
    rng = np.random.default_rng(n * 100 + n_dn)
    x = (rng.normal(size=S.dim) + 1j * rng.normal(size=S.dim)) * 1.1
    if real:
        x = np.ascontiguousarray(x.real)
    m = np.array([0.5, -0.5])
    ref = qr.qudit_repr(n, 2, n_dn, perms, chars, x, diag=(m,), string=(m, m), lower=(0.0, 1.0))
    sref = corrreprref.spin_repr(n, n_dn, perms, chars, x)
    t = _dev(x)
    got = _raw_args(n, 2, n_dn, perms, chars, m[None, :], (m, m), (0.0, 1.0), t)
    spin = q.spin_repr_correlations(n, n_dn, perms, chars, t, real=real, normalize=False)
    G = len(perms)
    qr.compare("d = 2 %d sites" % n, got, ref, G, n, _keys(ref))
    scale = (S.dim * G + 8) * 2.0 ** -53
    for mine, theirs, key, skey in ((got["aa"], spin["pm"], "aa", "pm"), (got["dd"][0, 0], spin["zz"], "dd", "zz"),
                                    (got["pop"] @ m, spin["sz"], None, "sz")):
        tol = scale * np.asarray(sref["A"][skey]).astype(np.float64)
        tol = tol + (qr.tolerance(ref, G, n, key).reshape(np.shape(tol)) if key else (qr.tolerance(ref, G, n, "pop") @ np.abs(m)))
        assert np.all(np.abs(mine - theirs) <= tol), skey
    assert got["norm2"][0] == spin["norm2"] or abs(got["norm2"][0] - spin["norm2"]) <= 2 * scale * spin["norm2"]


def test_more_representatives_than_one_trip_of_the_grid():
    """the spin-1 ring of 16 sites at S^z = 0, k = 0: 324,862 representatives -- more than the 262,144 lanes of the resident grid
    (four workgroups of 256 lanes on each of 256 CUs), so lanes walk their grid-stride loop twice.  The vector is nonzero on one
    row in sixteen, spread over the whole range, and the reference is limited to norm2, pop and three classes of each kind (string
    lengths 1, 4 and 8; the pair class r = 8 is its own mirror) to stay within seconds."""
    n, d, total = 16, 3, 16
    perms, chars = qr.ring(n, 0)
    diag, string, lower = _tables(d, 2, "spin")
    S = qr.sector(n, d, total, perms, chars)
    assert S.dim > 4 * 256 * 256
    rng = np.random.default_rng(16)
    x = np.zeros(S.dim)
    pick = rng.permutation(S.dim)[:S.dim // 16]
    x[pick] = rng.normal(size=len(pick)) * 1.3
    x[[0, S.dim - 1, 4 * 256 * 256, 4 * 256 * 256 + 1]] = [0.7, -1.1, 0.9, 1.2]
    ref = qr.qudit_repr(n, d, total, perms, chars, x, diag=diag, string=string, lower=lower, entries=[(0, 1), (3, 7), (2, 10)])
    for real in (True, False):
        got = _raw_args(n, d, total, perms, chars, diag, string, lower, _dev(x if real else x.astype(np.complex128)))
        assert got["dim"] == S.dim
        qr.compare("spin-1 ring 16 %s" % ("real" if real else "complex"), got, ref, n, n)
        assert np.all(got["aa"].imag == 0)


def test_python_wrappers_raw_normalised_and_derived():
    name = "spin1_ring8_sz0_k1"
    n, d, total, perms, chars, diag, string, lower = _args(name)
    x, ref = _case(name, False)
    t = _dev(x)
    raw = q.qudit_repr_correlations(n, d, total, perms, chars, t, diag=diag, string=string, lower=lower, normalize=False)
    nrm = q.qudit_repr_correlations(n, d, total, perms, chars, t, diag=diag, string=string, lower=lower)
    got = _raw(name, t)
    assert raw["dim"] == nrm["dim"] == ref["dim"] and raw["norm2"] == got["norm2"][0]
    assert all(_same_bits(raw[k], got[k]) for k in ("pop", "dd", "str", "aa"))
    assert np.allclose(nrm["aa"] * raw["norm2"], raw["aa"], rtol=1e-15)
    part = q.qudit_repr_correlations(n, d, total, perms, chars, t, normalize=False)
    assert set(part) == {"norm2", "pop", "dim"} and _same_bits(part["pop"], raw["pop"])
    # the spin-1 tables of this case are those of spin_s_repr_correlations: the same bits, and <S.S> = zz + Re pm
    sp = q.spin_s_repr_correlations(n, 1, 0, perms, chars, t, normalize=False)
    assert sp["dim"] == ref["dim"] and _same_bits(sp["zz"], raw["dd"][0, 0]) and _same_bits(sp["pm"], raw["aa"])
    assert _same_bits(sp["string"], raw["str"]) and np.allclose(np.diag(sp["ss"]), 2.0 * raw["norm2"])
    assert q.energy_from_correlations(sp, [(i, (i + 1) % n) for i in range(n)]) == pytest.approx(float(n * (raw["dd"][0, 0, 0, 1] + raw["aa"][0, 1].real)))
    bo = q.bose_repr_correlations(n, total, d - 1, perms, chars, t)
    assert bo["dim"] == ref["dim"] and np.allclose(np.sum(bo["dens"]), total, atol=1e-12)
    nk = q.momentum_distribution(bo["obdm"], np.arange(n), 2 * np.pi * np.arange(n) / n)
    assert np.allclose(np.sum(nk), np.trace(bo["obdm"]).real, atol=1e-10)     # a random vector has weight at n_max: the trace is not N_b


def test_ground_state_of_a_sector_shows_the_haldane_string_order():
    """spin-1 Heisenberg ring of 8 sites: the ground state (S^z = 0, k = 0) from the momentum sector's operator; <S.S> of nearest
    neighbours gives the energy, and the den Nijs-Rommelse string correlator at the largest distance stays finite and negative
    while the spin correlation has decayed below it"""
    n = 8
    perms, chars = qr.ring(n, 0)
    bonds = [(i, (i + 1) % n) for i in range(n)]
    H = q.csr_mat.spin_heisenberg_repr(n, 1, 0, bonds, perms, chars)
    try:
        r = q.locate_E0_lanczos(H, nev=1, ncv=1)
        c = q.spin_s_repr_correlations(n, 1, 0, perms, chars, _dev(r.eigenvecs))
        assert c["dim"] == H.dim
    finally:
        H.destroy()
    assert q.energy_from_correlations(c, bonds) == pytest.approx(r.E0, abs=1e-8)
    assert abs(r.E0 / n + 1.41712) < 1e-4                                       # the known energy per site of the 8-site ring
    assert c["string"][0, 4] < -0.3 and abs(c["zz"][0, 4]) < abs(c["string"][0, 4])
