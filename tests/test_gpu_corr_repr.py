"""qbh_corr_spin_repr_dev (all-pair correlations of a spin-1/2 momentum-sector state) entry by entry against tests/corrreprref.py
(the longdouble reference from representatives, pinned on the CPU by tests/test_corrreprref.py against unfolded states), on random
vectors that are not normalised and carry garbage at the zero-norm representatives, complex and -- at real characters --
packed-real, with every output buffer pre-filled with a sentinel.

Bound for every entry of sz, zz, pm and norm2:  |got - want| <= (dim |G| + 8) 2^-53 A,  A = the sum of the absolute values of the
terms of the entry (from the reference): any order of summation over at most dim |G| terms, each a product with a few roundings.
Entries with A = 0 must vanish exactly."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch

import corrreprref as rr
import quantum_basis_amd as q
from quantum_basis_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e300
KEYS = ("norm2", "sz", "zz", "pm")
ONE = (np.arange(7, dtype=np.int32)[None, :], np.ones(1, dtype=np.complex128))

CASES = {
    # name: (n_sites, n_dn, (perms, chars), real characters)
    "chain8_k1": (8, 4, rr.chain(8, 1), False),                       # two zero-norm representatives
    "chain8_k4": (8, 4, rr.chain(8, 4), True),
    "cells4x2_k1": (8, 3, rr.cells_chain(4, 2, 1), False),            # 16 ordered pair classes
    "cells4x2_k2": (8, 3, rr.cells_chain(4, 2, 2), True),
    "torus3x2_k11": (6, 2, rr.torus(3, 2, 1, 1), False),              # one zero-norm representative, dim 3
    "no_symmetry": (7, 3, ONE, True),                                 # n_trans = 1: 21 classes, three pair passes
    "chain16_k0": (16, 8, rr.chain(16, 0), True),                     # 12,870 words: four chunks of the directory
    "chain16_k3": (16, 8, rr.chain(16, 3), False),
    "chain16_k8": (16, 8, rr.chain(16, 8), True),
    "chain20_k0": (20, 10, rr.chain(20, 0), True),                    # 46 chunks of the directory, ten workgroups of 1024 lanes
    "chain40_dn2": (40, 2, rr.chain(40, 7), False),                   # words beyond 32 bits; tables of 143 KB in LDS, 1024 lanes
    "chain40_dn2_k20": (40, 2, rr.chain(40, 20), True),
    "chain62_dn2": (62, 2, rr.chain(62, 5), False),                   # 62 x 11 chunks = 349 KB of tables: read from global memory
    "chain62_dn2_k0": (62, 2, rr.chain(62, 0), True),
    "torus4x4_k12": (16, 8, rr.torus(4, 4, 1, 2), False),
    "torus4x4_k20": (16, 8, rr.torus(4, 4, 2, 0), True),
    "kagome2x2_k10": (12, 6, rr.torus(2, 2, 1, 0, n_sub=3), True),    # three sublattices, four translations
    "torus4x4_x_only_k1": (16, 7, rr.torus(4, 4, 1, 0, only_x=True), False),      # a subgroup: the action on the sites is not transitive
    "dim1": (6, 0, rr.chain(6, 0), True),
}
IDS = sorted(CASES)
REAL_IDS = [n for n in IDS if CASES[n][3]]


@functools.lru_cache(maxsize=None)
def _case(name, real):
    """(host vector, reference) -- computed once, shared, never modified"""
    N, n_dn, (perms, chars), _ = CASES[name]
    S = rr.sector(N, n_dn, perms, chars)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = ((rng.normal(size=S.dim) + 1j * rng.normal(size=S.dim)) * 1.3).astype(np.complex128)
    if real:
        x = np.ascontiguousarray(x.real)
    x.setflags(write=False)
    return x, rr.spin_repr(N, n_dn, perms, chars, x)


def _dev(x):
    t = torch.from_numpy(np.array(x)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw(name, t, want=KEYS):
    N, n_dn, (perms, chars), _ = CASES[name]
    return _raw_args(N, n_dn, perms, chars, t, want)


def _raw_args(N, n_dn, perms, chars, t, want=KEYS):
    real = t.dtype == torch.float64
    p, c = np.ascontiguousarray(perms, dtype=np.int32), np.ascontiguousarray(chars, dtype=np.complex128)
    out = {"norm2": np.full(1, SENTINEL), "sz": np.full(N, SENTINEL), "zz": np.full((N, N), SENTINEL),
           "pm": np.full((N, N), SENTINEL + 1j * SENTINEL)}
    a = {k: (_ptr(out[k]) if k in want else None) for k in out}
    dim = C.c_int64(-1)
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_spin_repr_dev(N, n_dn, len(p), _ptr(p), _ptr(c), None if real else addr, addr if real else None,
                                                 a["norm2"], a["sz"], a["zz"], a["pm"], C.byref(dim), None), "qbh_corr_spin_repr_dev")
    out["dim"] = dim.value
    return out


def _tolerance(ref, n_trans, key):
    return (ref["dim"] * n_trans + 8) * 2.0 ** -53 * np.asarray(ref["A"][key]).astype(np.float64)


def _compare(label, got, ref, n_trans):
    worst = {}
    for k in KEYS:
        w = np.asarray(ref[k])
        g = np.asarray(got[k]).reshape(w.shape)
        err = np.abs(g.astype(w.dtype) - w).astype(np.float64)
        tol = _tolerance(ref, n_trans, k)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
        worst[k] = float(np.max(ratio))
    print("%s dim %d |G| %d: worst |got - want| / bound  %s" % (label, ref["dim"], n_trans, "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k in KEYS:
        assert worst[k] <= 1.0, (label, k, worst[k])


@pytest.mark.parametrize("name", IDS)
def test_every_entry_against_the_reference_complex(name):
    x, ref = _case(name, False)
    got = _raw(name, _dev(x))
    assert got["dim"] == ref["dim"] == len(x)
    _compare(name + " complex", got, ref, len(CASES[name][2][0]))
    assert np.array_equal(got["pm"], got["pm"].conj().T) and np.array_equal(got["zz"], got["zz"].T)


@pytest.mark.parametrize("name", REAL_IDS)
def test_every_entry_against_the_reference_packed_real(name):
    x, ref = _case(name, True)
    got = _raw(name, _dev(x))
    assert got["dim"] == ref["dim"]
    _compare(name + " packed real", got, ref, len(CASES[name][2][0]))
    assert np.all(got["pm"].imag == 0) and np.array_equal(got["pm"], got["pm"].T)


def test_packed_real_needs_real_characters():
    x, _ = _case("chain8_k1", True)
    with pytest.raises(_lib.QbhError) as e:
        _raw("chain8_k1", _dev(x))
    assert e.value.code == -1 and "real characters" in str(e.value)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


@pytest.mark.parametrize("name,real", [("chain16_k3", False), ("chain16_k8", True), ("chain62_dn2", False)])
def test_null_groups_and_repeatability(name, real):
    x, _ = _case(name, real)
    t = _dev(x)
    full, again = _raw(name, t), _raw(name, t)
    assert all(_same_bits(full[k], again[k]) for k in KEYS)                     # two calls: the same bits
    for want in [("norm2",), ("sz",), ("zz",), ("pm",), ("norm2", "sz", "zz"), ("norm2", "pm"), ("zz", "pm"), ()]:
        part = _raw(name, t, want)
        for k in KEYS:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)                  # a NULL group changes no other output
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)  # ... and is not written
        assert part["dim"] == full["dim"]


@pytest.mark.parametrize("name", ["chain8_k1", "chain16_k3", "torus3x2_k11"])
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


# (30, 6): 593,775 rows, more than the resident grid holds at once -- every lane walks its grid-stride loop two or three times
@pytest.mark.parametrize("shape", [(7, 3), (30, 6)], ids=lambda s: "N%d_dn%d" % s)
@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_no_symmetry_equals_the_full_space_call(shape, real):
    """n_trans = 1: the representatives are the whole sector, and the call must agree with qbh_corr_spin_dev on the same vector
    within that call's own bound (tests/test_gpu_corr.py: 4 (dim + 4) 2^-53 norm2)."""
    N, n_dn = shape
    dim = math.comb(N, n_dn)
    rng = np.random.default_rng(31 * N + n_dn)
    x = (rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 1.3
    t = _dev(np.ascontiguousarray(x.real) if real else x)
    got = _raw_args(N, n_dn, np.arange(N, dtype=np.int32)[None, :], np.ones(1, dtype=np.complex128), t)
    assert got["dim"] == dim
    full = {"norm2": np.zeros(1), "sz": np.zeros(N), "zz": np.zeros((N, N)), "pm": np.zeros((N, N), dtype=np.complex128)}
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_spin_dev(N, n_dn, None if real else addr, addr if real else None, _ptr(full["norm2"]), _ptr(full["sz"]),
                                            _ptr(full["zz"]), _ptr(full["pm"]), None), "qbh_corr_spin_dev")
    bound = 4.0 * (dim + 4) * 2.0 ** -53 * float(full["norm2"][0])
    worst = {k: float(np.max(np.abs(got[k] - full[k]))) / bound for k in KEYS}
    print("N %d n_dn %d %s: worst |sector call - full-space call| / bound  %s" % (N, n_dn, "real" if real else "complex", worst))
    assert all(v <= 1.0 for v in worst.values()), worst


def _bonds_chain(n):
    return [(i, (i + 1) % n) for i in range(n)]


@pytest.mark.parametrize("name,bonds", [("chain16_k3", _bonds_chain(16)), ("chain8_k1", _bonds_chain(8)),
                                        ("torus4x4_k12", [(x + 4 * y, (x + 1) % 4 + 4 * y) for x in range(4) for y in range(4)] +
                                         [(x + 4 * y, x + 4 * ((y + 1) % 4)) for x in range(4) for y in range(4)])])
def test_energy_identity(name, bonds):
    """J sum_bonds (zz + Re pm) = <psi| H psi> for a random vector that vanishes at the zero-norm rows (their fake diagonal is
    no part of the Hamiltonian), on the same absolute scale: the bounds of the entries that enter, twice (the product H psi and
    the dot product sum the same terms in another order)."""
    N, n_dn, (perms, chars), _ = CASES[name]
    J = 0.7
    x, ref = _case(name, False)
    x = np.array(x)
    x[ref["zero"]] = 0.0
    got = _raw(name, _dev(x))
    b = np.asarray(bonds)
    e_corr = J * float(np.sum(got["zz"][b[:, 0], b[:, 1]] + got["pm"][b[:, 0], b[:, 1]].real))
    H = q.csr_mat.heisenberg_repr(N, n_dn, bonds, perms, chars, J=J)
    assert H.dim == len(x)
    v = H.vec(2)
    try:
        v.upload(x)
        H.spmv(v.at(0), v.at(H.dim))
        e_op = H.dotc(v.at(0), v.at(H.dim))
    finally:
        v.free()
    n_trans = len(perms)
    tol = 2.0 * J * float(np.sum(_tolerance(ref, n_trans, "zz")[b[:, 0], b[:, 1]] + _tolerance(ref, n_trans, "pm")[b[:, 0], b[:, 1]]))
    print("%s: <H> from correlations %.15g, from H psi %.15g, difference %.3g, bound %.3g" % (name, e_corr, e_op.real, abs(e_corr - e_op.real), tol))
    assert abs(e_corr - e_op.real) <= tol and abs(e_op.imag) <= tol
    assert q.energy_from_correlations(got, bonds, J=J) == pytest.approx(e_corr, rel=1e-15)


def test_ground_state_of_the_sector_equals_the_full_space_ground_state():
    """chain 16: the ground state lies at k = 0.  ss(r) from the sector's eigenvector through spin_repr_correlations against
    spin_correlations on the eigenvector of the whole S^z = 0 space, to 1e-9: the accuracy both solvers are asked for."""
    N, n_dn = 16, 8
    perms, chars = rr.chain(N, 0)
    bonds = _bonds_chain(N)
    Hk = q.csr_mat.heisenberg_repr(N, n_dn, bonds, perms, chars)
    rk = q.locate_E0_lanczos(Hk, nev=1, ncv=1)
    Hf = q.csr_mat.heisenberg(N, n_dn, bonds)
    rf = q.locate_E0_lanczos(Hf, nev=1, ncv=1)
    assert abs(rk.E0 - rf.E0) < 1e-9
    ck = q.spin_repr_correlations(N, n_dn, perms, chars, _dev(rk.eigenvecs))
    cf = q.spin_correlations(N, n_dn, _dev(rf.eigenvecs))
    assert ck["dim"] == Hk.dim
    assert np.max(np.abs(ck["ss"] - cf["ss"])) < 1e-9
    assert q.energy_from_correlations(ck, bonds) == pytest.approx(rk.E0, abs=1e-9)
    ss_r = ck["ss"][0]
    assert np.allclose(ss_r[1:], ss_r[1:][::-1], atol=1e-12)                    # ss(r) = ss(N - r)
    s_q = q.structure_factor(ck["ss"], np.arange(N, dtype=float), 2 * np.pi * np.arange(N) / N)
    assert s_q.shape == (N,) and abs(s_q[0]) < 1e-8 and np.argmax(s_q) == N // 2      # a singlet, antiferromagnetic


def test_python_wrapper_raw_and_normalised():
    name = "cells4x2_k1"
    N, n_dn, (perms, chars), _ = CASES[name]
    x, ref = _case(name, False)
    t = _dev(x)
    raw = q.spin_repr_correlations(N, n_dn, perms, chars, t, normalize=False)
    nrm = q.spin_repr_correlations(N, n_dn, perms, chars, t)
    got = _raw(name, t)
    assert raw["dim"] == ref["dim"] and raw["norm2"] == got["norm2"][0]
    assert all(_same_bits(raw[k], got[k]) for k in ("sz", "zz", "pm"))
    assert np.allclose(nrm["ss"] * raw["norm2"], raw["ss"], rtol=1e-15) and np.allclose(np.diag(nrm["ss"]), 0.75)
    assert q.structure_factor(nrm["ss"], np.arange(N, dtype=float), [0.0, np.pi]).shape == (2,)
