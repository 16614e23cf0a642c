"""qbh_corr_hubbard_repr_dev (all-pair correlations of a two-species fermion momentum-sector state) entry by entry against
tests/corrhubreprref.py (the longdouble reference from representatives, pinned on the CPU by tests/test_corrhubreprref.py against
unfolded states), on random vectors that are not normalised and carry garbage at the zero-norm representatives, complex and -- at
real characters -- packed-real, with every output buffer pre-filled with a sentinel.

Bound for every entry of norm2, dens, nn, hop and flip:  |got - want| <= (dim |G| + C_ROUND) 2^-53 A,  A = the sum of the absolute
values of the terms of the entry (from the reference), C_ROUND = 10 derived in the reference's docstring.  Entries with A = 0 must
vanish exactly."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch

import corrhubreprref as hr
import quantum_basis_amd as q
import secforms
from quantum_basis_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e300
KEYS = hr.KEYS
WHO = "qbh_corr_hubbard_repr_dev"

CASES = {
    # name: (n_sites, n_up, n_dn, (perms, chars), no_double, real characters)
    "ring6_k0": (6, 2, 2, hr.ring(6, 0), False, True),
    "ring6_k1": (6, 2, 2, hr.ring(6, 1), False, False),               # three zero-norm representatives
    "ring6_k3": (6, 2, 2, hr.ring(6, 3), False, True),
    "ring4_2+0_k0": (4, 2, 0, hr.ring(4, 0), False, True),            # {0, 2} is dead through the sign of T^2 alone
    "ring4_2+0_k1": (4, 2, 0, hr.ring(4, 1), False, False),
    "torus3x2_k00": (6, 2, 1, hr.torus(3, 2, 0, 0), False, True),
    "torus3x2_k11": (6, 2, 1, hr.torus(3, 2, 1, 1), False, False),
    "dihedral6_trivial": (6, 2, 2, hr.dihedral(6, False), False, True),      # classes that are their own mirror
    "dihedral6_sign": (6, 2, 2, hr.dihedral(6, True), False, True),
    "no_symmetry": (5, 2, 1, hr.identity(5), False, True),            # n_trans = 1: ten classes, five site orbits
    "ring6_3+0_k0": (6, 3, 0, hr.ring(6, 0), False, True),            # one species empty
    "ring6_3+0_k2": (6, 3, 0, hr.ring(6, 2), False, False),
    "ring6_tj_k0": (6, 2, 2, hr.ring(6, 0), True, True),              # no_double
    "ring6_tj_k1": (6, 2, 2, hr.ring(6, 1), True, False),
    "4x3_4+3_k11": (12, 4, 3, hr.torus(4, 3, 1, 1), False, False),    # complex characters, 108,900 words
    "4x4_4+2_k22": (16, 4, 2, hr.torus(4, 4, 2, 2), False, True),     # 32-bit words, 54 chunks of the directory
    "4x4_4+2_k13": (16, 4, 2, hr.torus(4, 4, 1, 3), False, False),
    "13x1_6+2_k5": (13, 6, 2, hr.ring(13, 5), False, False),
    "ring10_4+3_dihedral_sign": (10, 4, 3, hr.dihedral(10, True), False, True),      # 20 group elements
    "ring31_2+1_k3": (31, 2, 1, hr.ring(31, 3), False, False),        # dim 465, words to bit 61; tables of 93 KB: 1024 lanes
    "4x5_2+2_k20": (20, 2, 2, hr.torus(4, 5, 2, 0), False, True),     # dim 1810
    "ring31_2+1_dihedral": (31, 2, 1, hr.dihedral(31, True), False, True),   # 62 x 6 chunks = 186 KB of tables: read from global memory
    "dim1": (6, 0, 0, hr.ring(6, 0), False, True),
}
for _kx in range(4):
    for _ky in range(2):
        CASES["4x2_k%d%d" % (_kx, _ky)] = (8, 4, 4, hr.torus(4, 2, _kx, _ky), False, (_kx % 2 == 0))
IDS = sorted(CASES)
REAL_IDS = [n for n in IDS if CASES[n][5]]


@functools.lru_cache(maxsize=None)
def _case(name, real):
    """(host vector, reference) -- computed once, shared, never modified"""
    n, nu, nd, (perms, chars), nod, _ = CASES[name]
    S = hr.sector(n, nu, nd, perms, chars, nod)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = ((rng.normal(size=S.dim) + 1j * rng.normal(size=S.dim)) * 1.3).astype(np.complex128)
    if real:
        x = np.ascontiguousarray(x.real)
    x.setflags(write=False)
    return x, hr.hubbard_repr(n, nu, nd, perms, chars, x, nod)


def _dev(x):
    t = torch.from_numpy(np.array(x)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw(name, t, want=KEYS):
    n, nu, nd, (perms, chars), nod, _ = CASES[name]
    return _raw_args(n, nu, nd, perms, chars, t, want, nod)


def _raw_args(N, nu, nd, perms, chars, t, want=KEYS, no_double=False):
    real = t.dtype == torch.float64
    p, c = np.ascontiguousarray(perms, dtype=np.int32), np.ascontiguousarray(chars, dtype=np.complex128)
    out = {"norm2": np.full(1, SENTINEL), "dens": np.full((2, N), SENTINEL), "nn": np.full((4, N, N), SENTINEL),
           "hop": np.full((2, N, N), SENTINEL + 1j * SENTINEL), "flip": np.full((N, N), SENTINEL + 1j * SENTINEL)}
    a = {k: (_ptr(out[k]) if k in want else None) for k in out}
    dim = C.c_int64(-1)
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_hubbard_repr_dev(N, nu, nd, int(no_double), len(p), _ptr(p), _ptr(c), None if real else addr,
                                                    addr if real else None, a["norm2"], a["dens"], a["nn"], a["hop"], a["flip"],
                                                    C.byref(dim), None), WHO)
    out["dim"] = dim.value
    return out


def _tolerance(ref, n_trans, key):
    return (ref["dim"] * n_trans + hr.C_ROUND) * 2.0 ** -53 * np.asarray(ref["A"][key]).astype(np.float64)


def _compare(label, got, ref, n_trans):
    worst = {}
    for k in KEYS:
        w = np.asarray(ref[k])
        g = np.asarray(got[k]).reshape(w.shape)
        err = np.abs(g.astype(w.dtype) - w).astype(np.float64)
        tol = _tolerance(ref, n_trans, k)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))     # exact zeros stay exact
        worst[k] = float(np.max(ratio))
    print("%s dim %d |G| %d: worst |got - want| / bound  %s" % (label, ref["dim"], n_trans, "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k in KEYS:
        assert worst[k] <= 1.0, (label, k, worst[k])


@pytest.mark.parametrize("name", IDS)
def test_every_entry_against_the_reference_complex(name):
    x, ref = _case(name, False)
    got = _raw(name, _dev(x))
    assert got["dim"] == ref["dim"] == len(x)
    _compare(name + " complex", got, ref, len(CASES[name][3][0]))
    assert np.array_equal(got["hop"], got["hop"].conj().transpose(0, 2, 1)) and np.array_equal(got["flip"], got["flip"].conj().T)
    assert np.array_equal(got["nn"][1], got["nn"][2].T) and np.array_equal(got["nn"][0], got["nn"][0].T)
    assert np.array_equal(got["nn"][3], got["nn"][3].T)
    assert np.array_equal(np.diagonal(got["hop"], axis1=1, axis2=2).real, got["dens"])


@pytest.mark.parametrize("name", REAL_IDS)
def test_every_entry_against_the_reference_packed_real(name):
    x, ref = _case(name, True)
    got = _raw(name, _dev(x))
    assert got["dim"] == ref["dim"]
    _compare(name + " packed real", got, ref, len(CASES[name][3][0]))
    assert np.all(got["hop"].imag == 0) and np.all(got["flip"].imag == 0) and np.array_equal(got["flip"], got["flip"].T)


def test_packed_real_needs_real_characters():
    x, _ = _case("ring6_k1", True)
    with pytest.raises(_lib.QbhError) as e:
        _raw("ring6_k1", _dev(x))
    assert e.value.code == -1 and "real characters" in str(e.value)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


@pytest.mark.parametrize("name,real", [("4x2_k10", False), ("4x2_k20", True), ("ring31_2+1_dihedral", False), ("ring31_2+1_k3", False)])
def test_null_groups_and_repeatability(name, real):
    x, _ = _case(name, real)
    t = _dev(x)
    full, again = _raw(name, t), _raw(name, t)
    assert all(_same_bits(full[k], again[k]) for k in KEYS)                     # two calls: the same bits
    for want in [("norm2",), ("dens",), ("nn",), ("hop",), ("flip",), ("norm2", "dens", "nn"), ("hop", "flip"), ("nn", "flip"),
                 ("norm2", "hop"), ()]:
        part = _raw(name, t, want)
        for k in KEYS:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)                  # a NULL group changes no other output
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)  # ... and is not written
        assert part["dim"] == full["dim"]


@pytest.mark.parametrize("name", ["ring6_k1", "ring4_2+0_k0", "4x2_k11", "dihedral6_sign"])
def test_entries_at_zero_norm_representatives_are_never_read(name):
    x, ref = _case(name, False)
    zero = ref["zero"]
    assert zero.any()
    clean = np.array(x)
    clean[zero] = 0.0
    loud = np.array(x)
    loud[zero] = 1e150 * (1 + 1j)                                               # finite, and ruinous if it were read
    a, b, c = _raw(name, _dev(x)), _raw(name, _dev(clean)), _raw(name, _dev(loud))
    assert all(_same_bits(a[k], b[k]) and _same_bits(a[k], c[k]) for k in KEYS)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_no_symmetry_equals_the_full_space_call(real):
    """n_trans = 1 at 12 sites with 5 + 5: the representatives are the whole space, 627,264 rows -- more than one trip of the resident
    grid (tables of 4 KB: four workgroups of 256 lanes on each of the 256 CUs, 262,144 rows), so every lane walks its grid-stride
    loop two or three times.  The call must agree with qbh_corr_hubbard_dev on the same vector moved to that call's order (row =
    rank(u) C(n, n_dn) + rank(d); the sector's words are down-major) within that call's own bound (tests/test_gpu_corr.py:
    4 (dim + 4) 2^-53 norm2)."""
    N, nu, nd = 12, 5, 5
    dim = math.comb(N, nu) * math.comb(N, nd)
    rng = np.random.default_rng(1205)
    x = (rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 1.3
    if real:
        x = np.ascontiguousarray(x.real)
    perms, chars = hr.identity(N)
    got = _raw_args(N, nu, nd, perms, chars, _dev(x))
    assert got["dim"] == dim
    t = _dev(hr.to_generator_order(N, nu, nd, x))
    full = {"norm2": np.zeros(1), "dens": np.zeros((2, N)), "nn": np.zeros((4, N, N)), "hop": np.zeros((2, N, N), dtype=np.complex128),
            "flip": np.zeros((N, N), dtype=np.complex128)}
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_hubbard_dev(N, nu, nd, None if real else addr, addr if real else None, _ptr(full["norm2"]),
                                               _ptr(full["dens"]), _ptr(full["nn"]), _ptr(full["hop"]), _ptr(full["flip"]), None),
               "qbh_corr_hubbard_dev")
    bound = 4.0 * (dim + 4) * 2.0 ** -53 * float(full["norm2"][0])
    worst = {k: float(np.max(np.abs(got[k] - full[k]))) / bound for k in KEYS}
    print("N %d %d+%d %s: worst |sector call - full-space call| / bound  %s" % (N, nu, nd, "real" if real else "complex", worst))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_source_handle_in_orbit_order():
    """a device vector of a hubbard_repr_mf handle is kept orbit by orbit (info().basis_internal = BASIS_SECTOR_ORBIT): named with
    its handle it gives the bits of the call on the ascending vector, handed over bare it is another vector"""
    name = "4x2_k10"
    n, nu, nd, (perms, chars), _, _ = CASES[name]
    x, _ = _case(name, False)
    t = _dev(x)
    want = q.hubbard_repr_correlations(n, nu, nd, perms, chars, t, normalize=False)
    M = q.csr_mat.hubbard_repr_mf(n, nu, nd, secforms.operator("4x2_4+4", "plain")["bonds"], perms, chars)
    try:
        assert M.info().basis_internal == _lib.BASIS_SECTOR_ORBIT and M.dim == len(x)
        v = M.vec(1)
        try:
            M.to_internal(v.ptr, C.c_void_p(t.data_ptr()))
            M.sync()
            got = q.hubbard_repr_correlations(n, nu, nd, perms, chars, v, source=M, normalize=False)
            bare = q.hubbard_repr_correlations(n, nu, nd, perms, chars, v, normalize=False)
        finally:
            v.free()
    finally:
        M.destroy()
    assert got["dim"] == want["dim"] and got["norm2"] == want["norm2"]
    assert all(_same_bits(got[k], want[k]) for k in ("dens", "nn", "hop", "flip", "ss"))
    assert not _same_bits(bare["hop"], want["hop"])


@pytest.mark.parametrize("name", ["4x2_k10", "ring10_4+3_dihedral_sign", "4x3_4+3_k11"])
def test_entries_against_the_translation_averaged_sector_operator(name):
    """three entries of each group against measure_repr_static_hubbard on the same vector (zero at the zero-norm rows, whose fake
    diagonal is no part of an observable).  Both routes sum the same at most dim |G| terms, each with about C_ROUND roundings (the
    operator's stored value, its product with x and the product of the dot), so they differ by at most twice the entry's bound."""
    n, nu, nd, (perms, chars), _, _ = CASES[name]
    x, ref = _case(name, False)
    x = np.array(x)
    x[ref["zero"]] = 0.0
    t = _dev(x)
    got = _raw(name, t)
    addr = C.c_void_p(t.data_ptr())
    G = len(perms)
    pairs = [(0, 1), (2, n - 1), (n // 2, 0)]
    for (i, j) in pairs:
        for s in (0, 1):
            m = q.measure_repr_static_hubbard(n, nu, nd, perms, chars, addr, one_body=[(i, j, 1.0 - s, float(s))])
            assert abs(m - got["hop"][s, i, j]) <= 2 * _tolerance(ref, G, "hop")[s, i, j] + 1e-300, (name, "hop", s, i, j)
        for ab in range(4):
            v = [0.0] * 4
            v[ab] = 1.0
            m = q.measure_repr_static_hubbard(n, nu, nd, perms, chars, addr, two_body=[(i, j, *v)])
            assert abs(m - got["nn"][ab, i, j]) <= 2 * _tolerance(ref, G, "nn")[ab, i, j] + 1e-300, (name, "nn", ab, i, j)
        m = q.measure_repr_static_hubbard(n, nu, nd, perms, chars, addr, spin_exchange=[(i, j, 1.0)])
        tol = 2 * (_tolerance(ref, G, "flip")[i, j] + _tolerance(ref, G, "flip")[j, i])
        assert abs(m - (got["flip"][i, j] + got["flip"][j, i])) <= tol + 1e-300, (name, "flip", i, j)
    m = q.measure_repr_static_hubbard(n, nu, nd, perms, chars, addr, two_body=[(3, 3, 0.0, 1.0, 0.0, 0.0)])
    assert abs(m - got["nn"][1, 3, 3]) <= 2 * _tolerance(ref, G, "nn")[1, 3, 3]


@pytest.mark.parametrize("case,ik,variant", [("4x3_4+3", 2, "plain"), ("4x3_4+3", 2, "peierls"), ("4x2_4+4", 3, "plain")])
def test_energy_identity(case, ik, variant):
    """sum_terms (a_up hop[0][i][j] + a_dn hop[1][i][j]) + U sum_i nn_ud[i][i] = <psi| H psi> (spmv + dotc of csr_mat.hubbard_repr)
    for a random vector that vanishes at the zero-norm rows, on the same absolute scale: the bounds of the entries that enter,
    weighted with |amplitude|, twice (the product H psi and the dot product sum the same terms in another order).  The peierls
    variant has complex amplitudes of the down species."""
    spec, op = secforms.CASES[case], secforms.operator(case, variant)
    n, nu, nd = op["n"], spec["nu"], spec["nd"]
    perms, chars = secforms.symmetry(case, ik)
    perms, chars = np.asarray(perms, dtype=np.int32), np.asarray(chars, dtype=np.complex128)
    S = hr.sector(n, nu, nd, perms, chars)
    rng = np.random.default_rng(77 + ik)
    x = (rng.normal(size=S.dim) + 1j * rng.normal(size=S.dim)) * 0.9
    x[S.zero] = 0.0
    ref = hr.hubbard_repr(n, nu, nd, perms, chars, x)
    got = _raw_args(n, nu, nd, perms, chars, _dev(x))
    G = len(perms)
    e_corr, tol = 0.0 + 0.0j, 0.0
    t_hop = _tolerance(ref, G, "hop")
    for (i, j, au, ad) in op["terms"]:
        e_corr += au * got["hop"][0, i, j] + ad * got["hop"][1, i, j]
        tol += abs(au) * t_hop[0, i, j] + abs(ad) * t_hop[1, i, j]
    e_corr += op["U"] * np.trace(got["nn"][1])
    tol += abs(op["U"]) * float(np.trace(_tolerance(ref, G, "nn")[1]))
    tol *= 2.0
    H = q.csr_mat.hubbard_repr(n, nu, nd, None, perms, chars, U=op["U"], terms=op["terms"])
    try:
        assert H.dim == len(x)
        v = H.vec(2)
        try:
            v.upload(x)
            H.spmv(v.at(0), v.at(H.dim))
            e_op = H.dotc(v.at(0), v.at(H.dim))
        finally:
            v.free()
    finally:
        H.destroy()
    print("%s k %d %s: <H> from correlations %.15g%+.3gi, from H psi %.15g, difference %.3g, bound %.3g"
          % (case, ik, variant, e_corr.real, e_corr.imag, e_op.real, abs(e_corr - e_op), tol))
    assert abs(e_corr - e_op) <= tol
    if variant == "plain":
        bonds = op["bonds"]
        assert q.energy_from_correlations(got, bonds, t=1.0, U=op["U"]) == pytest.approx(e_corr.real, rel=1e-13)


def test_ground_state_of_the_sector_equals_the_full_space_ground_state():
    """4x2 with 4 + 4 at U = 1.1: the ground state of the full space (dense diagonalisation at dim 4900: non-degenerate, gap above
    1e-3) lies at k = (0, 0).  nn and ss from the sector's eigenvector through hubbard_repr_correlations against
    hubbard_correlations on the dense eigenvector of the whole (4, 4) space, to 1e-9: the accuracy the sector's solver is asked for."""
    import scipy.linalg
    import fastham
    from quantum_basis_amd import lattices
    n, nu, nd, U = 8, 4, 4, 1.1
    bonds = lattices.square(4, 2)
    Hf = np.asarray(fastham.hubbard_full(n, nu, nd, bonds, t=1.0, U=U).todense()).real        # row = rank(u) C(n, nd) + rank(d)
    assert Hf.shape == (4900, 4900)
    w, vecs = scipy.linalg.eigh(Hf, subset_by_index=[0, 1])
    assert abs(w[0] + 14.07605866) < 1e-8 and w[1] - w[0] > 1e-3                              # unique ground state
    perms, shifts = lattices.translations(4, 2)
    chars = lattices.characters(shifts, (0, 0), (4, 2))
    Hk = q.csr_mat.hubbard_repr(n, nu, nd, bonds, perms, chars, t=1.0, U=U)
    try:
        rk = q.locate_E0_lanczos(Hk, nev=1, ncv=1)
        assert abs(rk.E0 - w[0]) < 1e-9
        ck = q.hubbard_repr_correlations(n, nu, nd, perms, chars, _dev(rk.eigenvecs))
        assert ck["dim"] == Hk.dim == 628
    finally:
        Hk.destroy()
    cf = q.hubbard_correlations(n, nu, nd, _dev(vecs[:, 0].astype(np.complex128)))
    for k in ("nn", "ss", "docc", "szsz"):
        assert np.max(np.abs(ck[k] - cf[k])) < 1e-9, k
    assert q.energy_from_correlations(ck, bonds, t=1.0, U=U) == pytest.approx(w[0], abs=1e-8)
    nk = q.momentum_distribution(ck["hop"], [(x, y) for y in range(2) for x in range(4)],
                                 [(2 * np.pi * kx / 4, np.pi * ky) for kx in range(4) for ky in range(2)])
    assert nk.shape == (2, 8) and np.allclose(nk.sum(axis=1), [nu, nd], atol=1e-8) and np.all(nk > -1e-9) and np.all(nk < 1 + 1e-9)


def test_python_wrapper_raw_and_normalised():
    name = "torus3x2_k11"
    n, nu, nd, (perms, chars), _, _ = CASES[name]
    x, ref = _case(name, False)
    t = _dev(x)
    raw = q.hubbard_repr_correlations(n, nu, nd, perms, chars, t, normalize=False)
    nrm = q.hubbard_repr_correlations(n, nu, nd, perms, chars, t)
    got = _raw(name, t)
    assert raw["dim"] == nrm["dim"] == ref["dim"] and raw["norm2"] == got["norm2"][0]
    assert all(_same_bits(raw[k], got[k]) for k in ("dens", "nn", "hop", "flip"))
    assert np.allclose(nrm["ss"] * raw["norm2"], raw["ss"], rtol=1e-15) and np.array_equal(raw["docc"], np.diag(raw["nn"][1]))
    part = q.hubbard_repr_correlations(n, nu, nd, perms, chars, t, normalize=False, want=("hop",))
    assert set(part) == {"norm2", "hop", "dim"} and _same_bits(part["hop"], raw["hop"])
    tj = q.hubbard_repr_correlations(6, 2, 2, *CASES["ring6_tj_k0"][3], _dev(_case("ring6_tj_k0", False)[0]), normalize=False, no_double=True)
    assert tj["dim"] == 16 and np.all(tj["docc"] == 0.0)
