"""The all-pair correlation kernels (qbh_corr_spin_dev, qbh_corr_hubbard_dev) element by element against tests/corrref.py (the
host reference in longdouble, pinned by tests/test_corrref.py), on random vectors that are not normalised, in the complex and the
packed-real form, with every output buffer pre-filled with a sentinel.

Bound for every entry of every array:  |got - want| <= 4 (dim + 4) 2^-53 norm2.  Each entry is a sum of at most dim terms whose
absolute values sum to at most norm2 (Cauchy-Schwarz; every weight has modulus <= 1), the factor 4 covers the complex products;
`want` and norm2 come from the reference.  Entries that must be exactly zero are compared exactly."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import corrref
import helpers
import quantum_basis_amd as q
from quantum_basis_amd import _lib, lattices

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e300

# 32 sites: the last shape with 32-bit patterns (six chunks, bit 31); 33: the first with 64-bit ones; (12, 6): dim 924 is no
# multiple of the rows a lane steps through (8 or 4), so the last lane of the tile runs past the sector
SPIN_SHAPES = [(2, 1), (5, 2), (7, 3), (9, 4), (13, 6), (16, 8), (24, 2), (30, 3), (36, 3), (40, 2), (6, 0), (6, 6), (32, 2), (33, 2), (12, 6)]
HUB_SHAPES = [(2, 1, 1), (3, 2, 1), (5, 2, 3), (6, 3, 3), (8, 4, 4), (8, 1, 7), (8, 0, 3), (12, 2, 2), (20, 1, 2)]


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=n) + 1j * rng.normal(size=n)) * 1.3).astype(np.complex128)        # not normalised


def _bound(dim, norm2):
    return 4.0 * (dim + 4) * 2.0 ** -53 * float(norm2)


@functools.lru_cache(maxsize=None)
def _spin_case(N, n_dn, real):
    """(host vector, reference arrays) -- computed once, shared, never modified"""
    x = _rand(math.comb(N, n_dn), 7 + 100 * N + n_dn)
    if real:
        x = np.ascontiguousarray(x.real)
    return x, corrref.spin(N, n_dn, x)


@functools.lru_cache(maxsize=None)
def _hub_case(N, n_up, n_dn, real):
    x = _rand(math.comb(N, n_up) * math.comb(N, n_dn), 11 + 1000 * N + 10 * n_up + n_dn)
    if real:
        x = np.ascontiguousarray(x.real)
    return x, corrref.hubbard(N, n_up, n_dn, x)


def _dev(x):
    """the host vector on the device (complex128, or float64 = the packed real parts), in the generators' order"""
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw_spin(N, n_dn, t, want=("norm2", "sz", "zz", "pm")):
    real = t.dtype == torch.float64
    out = {"norm2": np.full(1, SENTINEL), "sz": np.full(N, SENTINEL), "zz": np.full((N, N), SENTINEL),
           "pm": np.full((N, N), SENTINEL + 1j * SENTINEL)}
    p = {k: (_ptr(out[k]) if k in want else None) for k in out}
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_spin_dev(N, n_dn, None if real else addr, addr if real else None, p["norm2"], p["sz"], p["zz"], p["pm"],
                                            None), "qbh_corr_spin_dev")
    return out


def _raw_hub(N, n_up, n_dn, t, want=("norm2", "dens", "nn", "hop", "flip")):
    real = t.dtype == torch.float64
    out = {"norm2": np.full(1, SENTINEL), "dens": np.full((2, N), SENTINEL), "nn": np.full((4, N, N), SENTINEL),
           "hop": np.full((2, N, N), SENTINEL + 1j * SENTINEL), "flip": np.full((N, N), SENTINEL + 1j * SENTINEL)}
    p = {k: (_ptr(out[k]) if k in want else None) for k in out}
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_hubbard_dev(N, n_up, n_dn, None if real else addr, addr if real else None, p["norm2"], p["dens"], p["nn"],
                                               p["hop"], p["flip"], None), "qbh_corr_hubbard_dev")
    return out


def _compare(label, got, ref, dim, keys):
    tol = _bound(dim, ref["norm2"])
    worst = {}
    for k in keys:
        g = np.asarray(got[k]).reshape(np.asarray(ref[k]).shape) if k != "norm2" else np.asarray(got[k]).reshape(())
        w = np.asarray(ref[k])
        err = np.abs(g.astype(w.dtype) - w).astype(np.float64)
        worst[k] = float(err.max() / tol)
    print("%s dim %d: worst |got - want| / bound  %s" % (label, dim, "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k in keys:
        g = np.asarray(got[k]).reshape(np.asarray(ref[k]).shape) if k != "norm2" else np.asarray(got[k]).reshape(())
        w = np.asarray(ref[k])
        assert worst[k] <= 1.0, (label, k, worst[k])
        zero = (w == 0)
        assert np.all(g[zero] == 0), (label, k, "an entry that must vanish exactly does not")
        if np.iscomplexobj(w):                                     # ... and so does a part of an entry
            assert np.all(g.real[w.real == 0] == 0) and np.all(g.imag[w.imag == 0] == 0), (label, k)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
@pytest.mark.parametrize("shape", SPIN_SHAPES, ids=lambda s: "N%d_dn%d" % s)
def test_spin_every_entry_against_the_reference(shape, real):
    N, n_dn = shape
    x, ref = _spin_case(N, n_dn, real)
    got = _raw_spin(N, n_dn, _dev(x))
    _compare("spin %s %s" % (shape, "real" if real else "complex"), got, ref, len(x), ("norm2", "sz", "zz", "pm"))
    assert np.array_equal(got["pm"], got["pm"].conj().T) and np.array_equal(got["zz"], got["zz"].T)     # the mirrored halves


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
@pytest.mark.parametrize("shape", HUB_SHAPES, ids=lambda s: "N%d_up%d_dn%d" % s)
def test_hubbard_every_entry_against_the_reference(shape, real):
    N, n_up, n_dn = shape
    x, ref = _hub_case(N, n_up, n_dn, real)
    got = _raw_hub(N, n_up, n_dn, _dev(x))
    _compare("hubbard %s %s" % (shape, "real" if real else "complex"), got, ref, len(x), ("norm2", "dens", "nn", "hop", "flip"))
    assert np.array_equal(got["flip"], got["flip"].conj().T)
    assert all(np.array_equal(got["hop"][s], got["hop"][s].conj().T) for s in (0, 1))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_spin_null_groups_and_repeatability(real):
    N, n_dn = 13, 6
    x, _ = _spin_case(N, n_dn, real)
    t = _dev(x)
    full, again = _raw_spin(N, n_dn, t), _raw_spin(N, n_dn, t)
    assert all(_same_bits(full[k], again[k]) for k in full)                     # two calls: the same bits
    for want in [("norm2",), ("sz",), ("zz",), ("pm",), ("norm2", "sz", "zz"), ("norm2", "pm"), ("zz", "pm"), ()]:
        part = _raw_spin(N, n_dn, t, want)
        for k in full:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)                  # the other outputs keep their bits
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)  # a group that was not asked for: untouched


@pytest.mark.parametrize("real", [False, True], ids=["complex", "packed_real"])
def test_hubbard_null_groups_and_repeatability(real):
    N, n_up, n_dn = 8, 4, 4
    x, _ = _hub_case(N, n_up, n_dn, real)
    t = _dev(x)
    full, again = _raw_hub(N, n_up, n_dn, t), _raw_hub(N, n_up, n_dn, t)
    assert all(_same_bits(full[k], again[k]) for k in full)
    for want in [("norm2",), ("dens",), ("nn",), ("hop",), ("flip",), ("norm2", "dens", "nn"), ("hop", "flip"), ("nn", "flip"), ()]:
        part = _raw_hub(N, n_up, n_dn, t, want)
        for k in full:
            if k in want:
                assert _same_bits(part[k], full[k]), (want, k)
            else:
                assert np.all(part[k].view(np.float64) == SENTINEL), (want, k)


def test_sign_convention_is_the_one_of_the_term_list_operator():
    """<S^+_i S^-_j>, <c+_{i,up} c_{j,up}> and the fermion spin flip against qbh_mopr_terms_dev + dotc, three random pairs each"""
    rng = np.random.default_rng(5)
    # spin (13, 6)
    N, n_dn = 13, 6
    x, ref = _spin_case(N, n_dn, False)
    A = q.csr_mat.heisenberg(N, n_dn, lattices.chain(N))
    t, y = _dev(x), torch.empty(len(x), dtype=torch.complex128, device="cuda")
    got = _raw_spin(N, n_dn, t)
    tol = _bound(len(x), ref["norm2"])
    for _ in range(3):
        i, j = (int(s) for s in rng.choice(N, size=2, replace=False))
        q.moprXvec_terms("spin", N, n_dn, 0, [(1.0, [("S+", i), ("S-", j)])], C.c_void_p(t.data_ptr()), C.c_void_p(y.data_ptr()))
        val = A.dotc(C.c_void_p(t.data_ptr()), C.c_void_p(y.data_ptr()))
        print("spin pm[%d][%d] %r  terms + dotc %r" % (i, j, got["pm"][i, j], val))
        assert abs(got["pm"][i, j] - val) <= tol
    A.destroy()
    # fermions (8, 4, 4)
    N, n_up, n_dn = 8, 4, 4
    x, ref = _hub_case(N, n_up, n_dn, False)
    A = q.csr_mat.hubbard(N, n_up, n_dn, lattices.square(4, 2))
    t, y = _dev(x), torch.empty(len(x), dtype=torch.complex128, device="cuda")
    got = _raw_hub(N, n_up, n_dn, t)
    tol = _bound(len(x), ref["norm2"])
    for _ in range(3):
        i, j = (int(s) for s in rng.choice(N, size=2, replace=False))
        for name, terms, mine in (("hop_up", [("c+", i, 0), ("c", j, 0)], got["hop"][0][i, j]),
                                  ("hop_dn", [("c+", i, 1), ("c", j, 1)], got["hop"][1][i, j]),
                                  ("flip", [("c+", i, 0), ("c", i, 1), ("c+", j, 1), ("c", j, 0)], got["flip"][i, j])):
            q.moprXvec_terms("fermion", N, n_up, n_dn, [(1.0, terms)], C.c_void_p(t.data_ptr()), C.c_void_p(y.data_ptr()))
            val = A.dotc(C.c_void_p(t.data_ptr()), C.c_void_p(y.data_ptr()))
            print("fermion %s[%d][%d] %r  terms + dotc %r" % (name, i, j, mine, val))
            assert abs(mine - val) <= tol
    A.destroy()


def _energy_by_spmv(A, x):
    v = A.vec(2)
    v.upload(x, 0)
    A.spmv(v.at(0), v.at(A.dim), 1.0, 0.0, 0.0)
    e = A.dotc(v.at(0), v.at(A.dim))
    v.free()
    return e


def test_energy_identity_for_a_random_vector():
    """<x| H |x> from the two-site expectation values equals spmv + dotc, for a vector that is no eigenvector"""
    N, n_dn = 13, 6
    bonds = lattices.chain(N)                                           # ring
    x, ref = _spin_case(N, n_dn, False)
    A = q.csr_mat.heisenberg(N, n_dn, bonds, J=1.0)
    want = _energy_by_spmv(A, x)
    A.destroy()
    corr = q.spin_correlations(N, n_dn, _dev(x), normalize=False)
    got = q.energy_from_correlations(corr, bonds, J=1.0)
    tol = _bound(len(x), ref["norm2"]) * len(bonds)
    print("heisenberg ring 13: E from correlations %.15g, spmv + dotc %.15g, |diff| / bound %.3g" % (got, want.real, abs(got - want.real) / tol))
    assert abs(got - want.real) <= tol and abs(want.imag) <= tol
    N, n_up, n_dn = 8, 4, 4
    bonds = lattices.square(4, 2)                                       # 4 x 2 torus, real hops
    x, ref = _hub_case(N, n_up, n_dn, False)
    A = q.csr_mat.hubbard(N, n_up, n_dn, bonds, t=1.0, U=1.1)
    want = _energy_by_spmv(A, x)
    A.destroy()
    corr = q.hubbard_correlations(N, n_up, n_dn, _dev(x), normalize=False)
    got = q.energy_from_correlations(corr, bonds, t=1.0, U=1.1)
    tol = _bound(len(x), ref["norm2"]) * len(bonds)
    print("hubbard 4x2: E from correlations %.15g, spmv + dotc %.15g, |diff| / bound %.3g" % (got, want.real, abs(got - want.real) / tol))
    assert abs(got - want.real) <= tol and abs(want.imag) <= tol


def _real_gauge(v):
    """the eigenvector of a real symmetric operator with its arbitrary phase removed: the real part then holds all of it"""
    k = int(np.argmax(np.abs(v)))
    return v * (np.conj(v[k]) / abs(v[k]))


def test_the_references_asserted_correlators_end_to_end():
    k = helpers.known()["chain16_full"]
    L, n_dn = 16, 8
    A = q.csr_mat.heisenberg(L, n_dn, lattices.chain(L))
    res = q.locate_E0_lanczos(A, nev=1, ncv=1)
    A.destroy()
    assert abs(res.E0 - k["E0"]) < k["tol"]
    psi = _real_gauge(res.eigenvecs)
    for real, vec in ((False, psi), (True, np.ascontiguousarray(psi.real))):
        c = q.spin_correlations(L, n_dn, _dev(vec), real=real)
        print("chain16 %s: zz01 %.12f zz02 %.12f pm01 %.12f norm2 %.15f" % ("real" if real else "complex", c["zz"][0, 1], c["zz"][0, 2],
                                                                           c["pm"][0, 1].real, c["norm2"]))
        assert abs(c["zz"][0, 1] - k["Sz0Sz1"]) < k["tol"]
        assert abs(c["zz"][0, 2] - k["Sz0Sz2"]) < k["tol"]
        assert abs(c["pm"][0, 1] - k["Sp0Sm1"]) < k["tol"]
        assert abs(q.energy_from_correlations(c, lattices.chain(L)) - k["E0"]) < k["tol"]
        assert abs(c["ss"][3, 3] - 0.75) < 1e-15 and abs(c["ss"][0, 1] - (c["zz"][0, 1] + c["pm"][0, 1].real)) < 1e-15
    k = helpers.known()["hubbard_4x2"]
    A = q.csr_mat.hubbard(8, 4, 4, lattices.square(4, 2), t=1.0, U=1.1)
    res = q.locate_E0_lanczos(A, nev=1, ncv=1)
    A.destroy()
    assert abs(res.E0 - k["E0"]) < k["tol"]
    psi = _real_gauge(res.eigenvecs)
    for real, vec in ((False, psi), (True, np.ascontiguousarray(psi.real))):
        c = q.hubbard_correlations(8, 4, 4, _dev(vec), real=real)
        print("hubbard 4x2 %s: hop[up][1][5] %.12f norm2 %.15f" % ("real" if real else "complex", c["hop"][0][1, 5].real, c["norm2"]))
        assert abs(c["hop"][0][1, 5] - k["cupdg1cup5"]) < k["tol"]
        assert abs(q.energy_from_correlations(c, lattices.square(4, 2), t=1.0, U=1.1) - k["E0"]) < k["tol"]
        assert np.allclose(c["docc"], np.diag(c["nn"][1])) and abs(c["nn_total"].sum() - 64.0) < 1e-10


def test_a_vector_in_a_handles_internal_order_is_translated_through_source():
    n, k, h = 16, 8, 8
    K = q.csr_mat.heisenberg(n, k, lattices.chain(n), J=1.0,
                             opts=q.make_opts(kron_split=2, basis_kind=_lib.BASIS_SPIN_SECTOR, n_sites=n, n_up=h, n_dn=k, value_dict=0,
                                              real_fast_path=0))
    assert K.info().basis_internal != 0
    x, _ = _spin_case(n, k, False)
    v = K.vec(1)
    v.upload(x)                                                         # translated into the handle's order
    got = q.spin_correlations(n, k, v, source=K, normalize=False)
    want = q.spin_correlations(n, k, _dev(x), normalize=False)
    wrong = q.spin_correlations(n, k, v, normalize=False)               # without `source` the handle's order is taken for the generators'
    for key in ("sz", "zz", "pm", "ss"):
        assert _same_bits(got[key], want[key]), key
    assert got["norm2"] == want["norm2"] and not _same_bits(wrong["zz"], want["zz"])
    with pytest.raises(ValueError):
        q.spin_correlations(n, k, v, real=True, source=K)
    v.free()
    K.destroy()
