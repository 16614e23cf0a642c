"""Pins tests/kondocorrref.py, the host reference of the Kondo all-pair correlations, against operators built independently of it:
Jordan-Wigner products of 2 x 2 factors (Kronecker products over the 3n two-level modes up_0 .. up_{n-1}, dn_0 .. dn_{n-1},
spin_0 .. spin_{n-1}; mode k is bit k of the word) on the FULL 8^n space, multiplied there and then restricted to the sector.
The Kronecker products are scipy.sparse.kron of the same factors np.kron would take (8^4 = 4096 is too wide for dense products).
Also pins the faults that compare() must reject.  No device."""
import copy
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp

import kondocorrref as kr
from quantum_basis_amd import kondo

I2 = sp.identity(2, format="csr")
Z = sp.csr_matrix(np.diag([1.0, -1.0]))
LOWER = sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]]))          # |0><1|: removes the particle / turns the local spin up
SZ = sp.csr_matrix(np.diag([0.5, -0.5]))                            # bit clear = local spin up


def mode_op(n_modes, k, m, string):
    """m on mode k, Z on the modes below it when `string`; the first Kronecker factor is the most significant bit"""
    out = sp.identity(1, format="csr")
    for q in range(n_modes - 1, -1, -1):
        out = sp.kron(out, m if q == k else (Z if (string and q < k) else I2), format="csr")
    return out


@lru_cache(maxsize=4)
def full_ops(n):
    M = 3 * n
    c = [[mode_op(M, sp_ * n + i, LOWER, True) for i in range(n)] for sp_ in (0, 1)]        # c_{i,up}, c_{i,dn}
    cd = [[a.T.tocsr() for a in row] for row in c]
    num = [[(cd[s][i] @ c[s][i]).tocsr() for i in range(n)] for s in (0, 1)]
    Sp = [mode_op(M, 2 * n + i, LOWER, False) for i in range(n)]                            # S^+_i
    Sm = [a.T.tocsr() for a in Sp]
    Sz = [mode_op(M, 2 * n + i, SZ, False) for i in range(n)]
    ep = [(cd[0][i] @ c[1][i]).tocsr() for i in range(n)]                                   # s^+_i = c^dag_up c_dn
    em = [(cd[1][i] @ c[0][i]).tocsr() for i in range(n)]
    return c, cd, num, Sp, Sm, Sz, ep, em


def dense_correlations(n, n_elec, two_sz, psi):
    c, cd, num, Sp, Sm, Sz, ep, em = full_ops(n)
    w = kondo.words(n, n_elec, two_sz).astype(np.int64)
    full = np.zeros(8 ** n, dtype=np.complex128)
    full[w] = psi

    def ev(O):
        return np.vdot(full, O @ full)

    R = range(n)
    out = {"norm2": np.vdot(psi, psi).real}
    out["site"] = np.array([[ev(num[0][i]).real for i in R], [ev(num[1][i]).real for i in R], [ev(num[0][i] @ num[1][i]).real for i in R],
                            [ev(Sz[i]).real for i in R]])
    out["nn"] = np.array([[[ev(num[a][i] @ num[b][j]).real for j in R] for i in R] for a in (0, 1) for b in (0, 1)])
    out["zn"] = np.array([[[ev(Sz[i] @ num[s][j]).real for j in R] for i in R] for s in (0, 1)])
    out["zz"] = np.array([[ev(Sz[i] @ Sz[j]).real for j in R] for i in R])
    out["hop"] = np.array([[[ev(cd[s][i] @ c[s][j]) for j in R] for i in R] for s in (0, 1)])
    out["ee"] = np.array([[ev(ep[i] @ em[j]) for j in R] for i in R])
    out["ll"] = np.array([[ev(Sp[i] @ Sm[j]) for j in R] for i in R])
    out["le"] = np.array([[ev(Sp[i] @ em[j]) for j in R] for i in R])
    return out


def all_sectors(n):
    return [(ne, tz) for ne in range(2 * n + 1) for tz in range(-2 * n, 2 * n + 1) if kondo.sector_dim(n, ne, tz) > 0]


def rand_vec(dim, seed, real=False):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(dim) if real else rng.standard_normal(dim) + 1j * rng.standard_normal(dim)


def check_sector(n, ne, tz, seed):
    dim = kondo.sector_dim(n, ne, tz)
    for real in (False, True):
        psi = rand_vec(dim, seed + real, real)
        ref = kr.correlations(n, ne, tz, psi)
        dense = dense_correlations(n, ne, tz, psi)
        tol = kr.bound(dim, ref["norm2"]) + 64 * 2.0 ** -53 * float(ref["norm2"])           # + the dense product's own rounding
        for k in kr.KEYS:
            err = np.max(np.abs(np.asarray(ref[k]).astype(np.complex128) - dense[k]))
            assert err <= tol, (n, ne, tz, real, k, err, tol)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_reference_matches_jordan_wigner_every_sector(n):
    sectors = all_sectors(n)
    assert sum(kondo.sector_dim(n, ne, tz) for ne, tz in sectors) == 8 ** n
    for k, (ne, tz) in enumerate(sectors):
        check_sector(n, ne, tz, 100 * n + k)


def test_reference_matches_jordan_wigner_4_4_0():
    assert kondo.sector_dim(4, 4, 0) == 346
    check_sector(4, 4, 0, 7)


def test_reference_symmetries():
    n, ne, tz = 3, 4, 1
    assert kondo.sector_dim(n, ne, tz) == 39
    psi = rand_vec(kondo.sector_dim(n, ne, tz), 3)
    r = kr.correlations(n, ne, tz, psi)
    for k in ("ee", "ll"):
        assert np.max(np.abs(r[k] - np.conj(r[k].T))) < 1e-15 * float(r["norm2"])
    assert np.max(np.abs(r["hop"] - np.conj(np.transpose(r["hop"], (0, 2, 1))))) < 1e-15 * float(r["norm2"])
    assert np.max(np.abs(r["le"] - np.conj(r["le"].T))) > 1e-3 * float(r["norm2"])          # le is NOT Hermitian
    assert np.allclose(np.diag(r["zz"]).astype(float), 0.25 * float(r["norm2"]))
    assert np.allclose(np.diag(r["ll"]).real.astype(float), (0.5 * r["norm2"] + r["site"][3]).astype(float))
    assert np.allclose(np.diag(r["ee"]).real.astype(float), (r["site"][0] - r["site"][2]).astype(float))


# ---- the faults compare() must reject ----
@pytest.fixture(scope="module")
def case():
    n, ne, tz = 3, 3, 0
    dim = kondo.sector_dim(n, ne, tz)
    psi = rand_vec(dim, 11)
    ref = kr.correlations(n, ne, tz, psi)
    got = {k: np.asarray(v).astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in ref.items()}
    return dim, ref, got


def test_compare_accepts_the_rounded_reference(case):
    dim, ref, got = case
    kr.compare("rounded", got, ref, dim)


def rejects(case, mutate):
    dim, ref, got = case
    bad = copy.deepcopy(got)
    mutate(bad, kr.bound(dim, ref["norm2"]))
    with pytest.raises(AssertionError):
        kr.compare("fault", bad, ref, dim)


def test_compare_rejects_le_transposed(case):
    def f(bad, tol):
        bad["le"] = bad["le"].T.copy()
    rejects(case, f)


def test_compare_rejects_conjugated_hop(case):
    def f(bad, tol):
        bad["hop"] = np.conj(bad["hop"])
    rejects(case, f)


@pytest.mark.parametrize("key,at", [("ee", (0, 1)), ("hop", (1, 0, 2)), ("le", (1, 1)), ("ll", (2, 0)), ("zn", (0, 1, 2)), ("site", (3, 1))])
def test_compare_rejects_one_flipped_sign(case, key, at):
    def f(bad, tol):
        bad[key][at] = -bad[key][at]
    rejects(case, f)


@pytest.mark.parametrize("key,at", [("norm2", ()), ("site", (0, 0)), ("nn", (1, 0, 1)), ("zn", (1, 2, 2)), ("zz", (0, 2)), ("hop", (0, 0, 1)),
                                    ("ee", (1, 2)), ("ll", (0, 1)), ("le", (2, 0))])
def test_compare_rejects_twice_the_bound(case, key, at):
    def f(bad, tol):
        if at == ():
            bad[key] = bad[key] + 2.0 * tol
        else:
            bad[key][at] = bad[key][at] + 2.0 * tol
    rejects(case, f)


def test_compare_rejects_a_nonzero_where_a_zero_belongs():
    # (2, 0, 2): one word, every pair entry off the diagonal vanishes exactly
    psi = np.array([0.6 - 0.3j])
    ref = kr.correlations(2, 0, 2, psi)
    got = {k: np.asarray(v).astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in ref.items()}
    kr.compare("one word", got, ref, 1)
    assert ref["ll"][0, 1] == 0 and ref["hop"][0, 0, 1] == 0
    for key, at in (("ll", (0, 1)), ("hop", (0, 0, 1)), ("le", (0, 0))):
        bad = copy.deepcopy(got)
        bad[key][at] = 1e-30                                    # far inside the bound, but not zero
        with pytest.raises(AssertionError):
            kr.compare("fault", bad, ref, 1)
    bad = copy.deepcopy(got)
    bad["ee"][0, 0] = bad["ee"][0, 0] + 1e-30j                  # an imaginary part on a real diagonal
    with pytest.raises(AssertionError):
        kr.compare("fault", bad, ref, 1)
