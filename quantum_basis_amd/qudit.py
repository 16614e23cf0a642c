"""Local operators and term tables for sites with d levels (qbh_gen_qudit, qbh_mopr_qudit_dev).  Pure numpy, no device.

Level convention (include/qbhip.h, qbh_gen_qudit): site s holds a level l in [0, d) whose charge is l.
    spin S:              d = 2S + 1, l = S - m (l = 0 is m = +S), so the charge of a sector is n S - S^z_total
    bosons, n <= n_max:  d = n_max + 1, l = n
A pair term is a d^2 x d^2 matrix M with M[l'_i d + l'_j, l_i d + l_j] = <l'_i l'_j|M|l_i l_j>, i.e. np.kron(A_i, B_j) for a
product A_i B_j; a single-site term is the diagonal of a local operator (one value per level).
"""
from fractions import Fraction

import numpy as np


def _two_s(S):
    two = Fraction(S).limit_denominator(2) * 2
    if two.denominator != 1 or two < 1:
        raise ValueError("S must be a positive multiple of 1/2, got %r" % (S,))
    return int(two)


def spin_matrices(S):
    """(S^z, S^+, S^-) of spin S as (2S+1) x (2S+1) complex matrices in the level basis l = S - m."""
    d = _two_s(S) + 1
    Sv = (d - 1) / 2.0
    m = Sv - np.arange(d)
    sz = np.diag(m).astype(np.complex128)
    sp = np.zeros((d, d), dtype=np.complex128)
    for l in range(1, d):                       # S^+ |m> = sqrt(S(S+1) - m(m+1)) |m+1>, and m+1 is level l-1
        sp[l - 1, l] = np.sqrt(Sv * (Sv + 1) - m[l] * (m[l] + 1))
    return sz, sp, sp.T.copy()


def boson_matrices(n_max):
    """(b, b^dag, n) truncated to at most n_max bosons, levels l = n."""
    d = n_max + 1
    b = np.zeros((d, d), dtype=np.complex128)
    for n in range(1, d):
        b[n - 1, n] = np.sqrt(n)
    return b, b.T.copy(), np.diag(np.arange(d)).astype(np.complex128)


def _bond_list(bonds):
    return [(int(i), int(j)) for i, j in np.asarray(bonds, dtype=np.int64).reshape(-1, 2)]


def heisenberg_terms(S, bonds, J=1.0, Jz=None, K=0.0):
    """Pair terms of  sum_<ij> [ J/2 (S+_i S-_j + S-_i S+_j) + Jz S^z_i S^z_j + K (S_i . S_j)^2 ]  (Jz = J by default):
    a list of (i, j, M), one per bond."""
    Jz = J if Jz is None else Jz
    sz, sp, sm = spin_matrices(S)
    exch = 0.5 * (np.kron(sp, sm) + np.kron(sm, sp))
    zz = np.kron(sz, sz)
    M = J * exch + Jz * zz
    if K != 0.0:
        ss = exch + zz
        M = M + K * (ss @ ss)
    return [(i, j, M.copy()) for i, j in _bond_list(bonds)]


def single_ion(S, n_sites, D):
    """Single-site terms of  D sum_s (S^z_s)^2:  a list of (s, diag)."""
    sz = spin_matrices(S)[0]
    dg = D * np.real(np.diag(sz)) ** 2
    return [(s, dg.copy()) for s in range(n_sites)]


def bose_hubbard_terms(n_max, bonds, t, U, mu=0.0):
    """-t sum_<ij> (b+_i b_j + h.c.) + U/2 sum_s n_s (n_s - 1) - mu sum_s n_s  as (pairs, singles); the single-site terms
    cover every site named by a bond."""
    b, bd, _ = boson_matrices(n_max)
    M = -t * (np.kron(bd, b) + np.kron(b, bd))
    bl = _bond_list(bonds)
    n = np.arange(n_max + 1, dtype=np.float64)
    dg = 0.5 * U * n * (n - 1) - mu * n
    sites = sorted({s for ij in bl for s in ij})
    return [(i, j, M.copy()) for i, j in bl], [(s, dg.copy()) for s in sites]


def qudit_dim(n_sites, d, total):
    """Number of words of n_sites levels in [0, d) whose levels sum to total (the sector dimension; exact integer)."""
    if n_sites < 0 or d < 1:
        raise ValueError("n_sites >= 0 and d >= 1")
    cnt = [1] + [0] * max(total, 0)
    for _ in range(n_sites):
        cnt = [sum(cnt[q - l] for l in range(min(d - 1, q) + 1)) for q in range(len(cnt))]
    return cnt[total] if 0 <= total < len(cnt) else 0


def spin_charge(n_sites, S, two_sz):
    """The charge total = n S - S^z of the sector with 2 S^z = two_sz (ValueError when it is not an integer in range)."""
    two_s = _two_s(S)
    num = n_sites * two_s - two_sz
    if num % 2 or num < 0 or num > 2 * n_sites * two_s:
        raise ValueError("2 S^z = %d is not a sector of %d spins %s" % (two_sz, n_sites, S))
    return num // 2
