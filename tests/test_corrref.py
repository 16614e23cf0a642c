"""Pins tests/corrref.py (the host reference of the all-pair correlations): every sector is embedded in the full 2^N (spin) or 4^N
(fermion) space, where the site operators are Kronecker products (with Jordan-Wigner strings for the fermions), and every array
must agree to 1e-13 on random complex vectors; the sum rules of the sector hold.  CPU only."""
import functools

import numpy as np
import pytest

import corrref

TOL = 1e-13


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)) * 1.7       # not normalised


def _site_op(local, pos, n, below=None):
    """kron over positions n-1 .. 0 (position p is bit p of the index): `local` at pos, `below` on every position under it"""
    ident = np.eye(2)
    m = np.ones((1, 1))
    for p in range(n - 1, -1, -1):
        m = np.kron(m, local if p == pos else (below if (below is not None and p < pos) else ident))
    return m


SPIN_SHAPES = [(1, 0), (1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (6, 0), (6, 6), (7, 3), (8, 4), (8, 1)]


@pytest.mark.parametrize("shape", SPIN_SHAPES)
def test_spin_reference_against_kronecker_operators(shape):
    N, n_dn = shape
    pat = corrref.patterns(N, n_dn)
    psi = _rand(len(pat), 100 * N + n_dn)
    full = np.zeros(2 ** N, dtype=np.complex128)
    full[pat.astype(np.int64)] = psi                                  # local index 0 = up, 1 = down: the index IS the pattern
    sz_l, sp_l = np.diag([0.5, -0.5]), np.array([[0.0, 1.0], [0.0, 0.0]])      # S^+ takes down (1) to up (0)
    Sz = [_site_op(sz_l, i, N) for i in range(N)]
    Sp = [_site_op(sp_l, i, N) for i in range(N)]
    got = corrref.spin(N, n_dn, psi)
    assert abs(got["norm2"] - np.vdot(psi, psi).real) <= TOL * float(got["norm2"])
    scale = float(got["norm2"])
    for i in range(N):
        assert abs(got["sz"][i] - np.vdot(full, Sz[i] @ full)) <= TOL * scale
        for j in range(N):
            assert abs(got["zz"][i, j] - np.vdot(full, Sz[i] @ (Sz[j] @ full))) <= TOL * scale
            assert abs(got["pm"][i, j] - np.vdot(full, Sp[i] @ (Sp[j].T @ full))) <= TOL * scale
    # sum rules
    assert abs(got["zz"].sum() - (N / 2 - n_dn) ** 2 * got["norm2"]) <= TOL * scale * N * N
    assert abs(got["sz"].sum() - (N / 2 - n_dn) * got["norm2"]) <= TOL * scale * N
    assert np.abs(got["pm"] - got["pm"].conj().T).max() <= TOL * scale
    assert np.abs(got["zz"] - got["zz"].T).max() <= TOL * scale
    assert np.abs(np.diag(got["zz"]) - got["norm2"] / 4).max() <= TOL * scale
    assert np.abs(np.diag(got["pm"]) - (got["norm2"] / 2 + got["sz"])).max() <= TOL * scale


HUB_SHAPES = [(1, 1, 0), (2, 1, 1), (2, 2, 1), (3, 2, 1), (3, 1, 1), (4, 2, 2), (4, 1, 3), (4, 0, 2), (4, 3, 3), (4, 4, 1)]


@functools.lru_cache(maxsize=None)
def _fermi_ops(N):
    """c+_o for the 2N orbitals o = site + species * N with the Jordan-Wigner string on the orbitals BELOW o"""
    ad, z = np.array([[0.0, 0.0], [1.0, 0.0]]), np.diag([1.0, -1.0])
    return [_site_op(ad, o, 2 * N, below=z) for o in range(2 * N)]


@pytest.mark.parametrize("shape", HUB_SHAPES)
def test_hubbard_reference_against_jordan_wigner_operators(shape):
    N, n_up, n_dn = shape
    B = corrref.HubbardBasis(N, n_up, n_dn)
    psi = _rand(len(B.words), 1000 * N + 10 * n_up + n_dn)
    full = np.zeros(4 ** N, dtype=np.complex128)
    full[B.words.astype(np.int64)] = psi
    Cd = _fermi_ops(N)

    def ev(*ops):                                                       # <full| ops[0] ops[1] ... |full>
        v = full
        for m in reversed(ops):
            v = m @ v
        return np.vdot(full, v)

    got = corrref.hubbard(N, n_up, n_dn, psi)
    scale = float(got["norm2"])
    assert abs(got["norm2"] - np.vdot(psi, psi).real) <= TOL * scale
    n_op = [[Cd[i + s * N] @ Cd[i + s * N].T for i in range(N)] for s in (0, 1)]
    for i in range(N):
        for s in (0, 1):
            assert abs(got["dens"][s, i] - ev(n_op[s][i])) <= TOL * scale
        for j in range(N):
            for a in (0, 1):
                for b in (0, 1):
                    assert abs(got["nn"][2 * a + b, i, j] - ev(n_op[a][i], n_op[b][j])) <= TOL * scale
            for s in (0, 1):
                assert abs(got["hop"][s, i, j] - ev(Cd[i + s * N], Cd[j + s * N].T)) <= TOL * scale
            assert abs(got["flip"][i, j] - ev(Cd[i], Cd[i + N].T, Cd[j + N], Cd[j].T)) <= TOL * scale
    # sum rules
    for s, n_s in ((0, n_up), (1, n_dn)):
        assert abs(got["dens"][s].sum() - n_s * got["norm2"]) <= TOL * scale * N
        assert abs(np.trace(got["hop"][s]) - n_s * got["norm2"]) <= TOL * scale * N
        assert np.abs(got["hop"][s] - got["hop"][s].conj().T).max() <= TOL * scale
    assert np.abs(got["flip"] - got["flip"].conj().T).max() <= TOL * scale
    assert abs(got["nn"].sum() - (n_up + n_dn) ** 2 * got["norm2"]) <= TOL * scale * N * N
    assert np.abs(np.diag(got["flip"]) - (got["dens"][0] - np.diag(got["nn"][1]))).max() <= TOL * scale


def test_the_elementary_operators_anticommute():
    """A four-factor chain through intermediate words outside the sector: for a != b, c+_a c_b c+_b c_a = n_a (1 - n_b), so adding
    n_a n_b gives n_a -- every sign of the chain has to cancel."""
    N, n_up, n_dn = 4, 2, 1
    B = corrref.HubbardBasis(N, n_up, n_dn)
    psi = _rand(len(B.words), 5)
    for a in range(N):
        for b in range(N):
            if a == b:
                continue
            lhs = corrref.hubbard_expect(B, psi, [(1, a, 0), (2, b, 0), (1, b, 0), (2, a, 0)]) + \
                corrref.hubbard_expect(B, psi, [(0, a, 0), (0, b, 0)])
            assert abs(lhs - corrref.hubbard_expect(B, psi, [(0, a, 0)])) <= TOL * float(np.vdot(psi, psi).real)
