"""Basis and term lists of the Kondo lattice model (qbh_gen_kondo, qbh_mf_kondo, qbh_gen_kondo_repr).  Pure numpy, no device.

Every site carries a conduction-electron orbital and a localized spin-1/2.  A basis word is three n-bit fields

    w = u | d << n | s << 2n        u, d: sites occupied by an up / down electron;  s: sites whose local spin is DOWN

and the sector (n_elec, two_sz) holds the words with popcount(u) + popcount(d) = n_elec and
(popcount(u) - popcount(d)) + (n - 2 popcount(s)) = two_sz, in ascending order of w.  popcount(s) = m fixes the electron
numbers, so the sector is a union of blocks (n_up, n_dn, m): sector_blocks.

The operator (include/qbhip.h, qbh_gen_kondo) is given by a Terms tuple:
    hops    [(i, j, amp_up, amp_dn), ...]   amp * c+_i c_j per species (i == j: a number operator)
    kz, kxy [n_sites] each                  kz S^z_i s^z_i + kxy/2 (S+_i s-_i + S-_i s+_i), s = the electron's spin on site i
    sbonds  [(i, j, bz, bxy), ...]          bz S^z_i S^z_j + bxy/2 (S+_i S-_j + S-_i S+_j) between local spins
and U sum_i n_up n_dn, passed separately.
"""
from collections import namedtuple
from functools import lru_cache
from math import comb

import numpy as np

MAX_SITES = 21

Terms = namedtuple("Terms", "hops kz kxy sbonds")

# the operators between sectors (qbh_mopr_kondo_dev, qbh_mopr_kondo_repr_dev): sum_s coef[s] O_s
C_UP, C_DN, CDAG_UP, CDAG_DN, SPIN_PLUS, SPIN_MINUS = range(6)
_MOPR_SHIFT = {C_UP: (-1, -1), C_DN: (-1, 1), CDAG_UP: (1, 1), CDAG_DN: (1, -1), SPIN_PLUS: (0, 2), SPIN_MINUS: (0, -2)}


def mopr_target(n_elec, two_sz, op):
    """(n_elec_new, two_sz_new) of the sector the operator `op` takes the sector (n_elec, two_sz) to."""
    de, ds = _MOPR_SHIFT[int(op)]
    return n_elec + de, two_sz + ds


def sector_blocks(n_sites, n_elec, two_sz):
    """[(n_up, n_dn, m), ...] for every number m of down local spins that the sector admits, m ascending."""
    twice_up0 = n_elec + two_sz - n_sites            # 2 n_up = n_elec + two_sz - n + 2 m
    if twice_up0 % 2:
        return []
    out = []
    for m in range(n_sites + 1):
        n_up = twice_up0 // 2 + m
        n_dn = n_elec - n_up
        if 0 <= n_up <= n_sites and 0 <= n_dn <= n_sites:
            out.append((n_up, n_dn, m))
    return out


def sector_dim(n_sites, n_elec, two_sz):
    """Number of words of the sector (n = n_elec, two_sz = 0: the Franel numbers sum_m C(n, m)^3)."""
    return sum(comb(n_sites, m) * comb(n_sites, n_up) * comb(n_sites, n_dn) for (n_up, n_dn, m) in sector_blocks(n_sites, n_elec, two_sz))


def _patterns(n_sites):
    """patterns[k] = the n-bit integers with k set bits, ascending"""
    a = np.arange(1 << n_sites, dtype=np.uint64)
    pc = np.zeros(a.size, dtype=np.int64)
    for b in range(n_sites):
        pc += ((a >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return [a[pc == k] for k in range(n_sites + 1)]


def words(n_sites, n_elec, two_sz):
    """The words of the sector, ascending (uint64): row i of csr_mat.kondo is words(...)[i]."""
    assert 1 <= n_sites <= MAX_SITES
    blocks = {m: (n_up, n_dn) for (n_up, n_dn, m) in sector_blocks(n_sites, n_elec, two_sz)}
    pat = _patterns(n_sites)
    n = np.uint64(n_sites)
    out = []
    for s in range(1 << n_sites):
        m = bin(s).count("1")
        if m not in blocks:
            continue
        n_up, n_dn = blocks[m]
        ud = (pat[n_dn][:, None] << n) | pat[n_up][None, :]
        out.append(ud.reshape(-1) | (np.uint64(s) << (n + n)))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint64)


@lru_cache(maxsize=16)
def _rank_table(n_sites, n_elec, two_sz):
    """(blocks, A): blocks[m] = (n_up, n_dn) and A[p][c] = sum_j C(p, j) w(c + j) with w(m) = C(n, n_up(m)) C(n, n_dn(m))
    (0 where the sector has no block m): the words whose s field agrees with a given one above bit p, holds 0 at p and has c
    ones above p (the table of the device's ranking, qbh_kondo.hpp)."""
    assert 1 <= n_sites <= MAX_SITES
    blocks = {m: (n_up, n_dn) for (n_up, n_dn, m) in sector_blocks(n_sites, n_elec, two_sz)}
    w = [comb(n_sites, blocks[m][0]) * comb(n_sites, blocks[m][1]) if m in blocks else 0 for m in range(n_sites + 1)]
    A = [[sum(comb(p, j) * w[c + j] for j in range(p + 1) if c + j <= n_sites) for c in range(n_sites + 1)] for p in range(n_sites + 1)]
    return blocks, A


def _colex_rank(bits):
    r, k = 0, 0
    p = 0
    while bits:
        if bits & 1:
            k += 1
            r += comb(p, k)
        bits >>= 1
        p += 1
    return r


def _colex_unrank(n_sites, k, r):
    bits, p = 0, n_sites - 1
    while k >= 1:
        while comb(p, k) > r:
            p -= 1
        bits |= 1 << p
        r -= comb(p, k)
        p -= 1
        k -= 1
    return bits


def unrank(n_sites, n_elec, two_sz, r):
    """(u, d, s) of the word with index r in the sector, without enumerating it: words(...)[r] == u | d << n | s << 2n."""
    blocks, A = _rank_table(n_sites, n_elec, two_sz)
    r = int(r)
    assert 0 <= r < sector_dim(n_sites, n_elec, two_sz)
    s, c = 0, 0
    for p in range(n_sites - 1, -1, -1):
        if r >= A[p][c]:
            s |= 1 << p
            r -= A[p][c]
            c += 1
    n_up, n_dn = blocks[c]
    cu = comb(n_sites, n_up)
    return _colex_unrank(n_sites, n_up, r % cu), _colex_unrank(n_sites, n_dn, r // cu), s


def rank(n_sites, n_elec, two_sz, u, d, s):
    """Index in the sector of the word u | d << n | s << 2n (which must belong to it): the inverse of unrank."""
    blocks, A = _rank_table(n_sites, n_elec, two_sz)
    u, d, s = int(u), int(d), int(s)
    m = bin(s).count("1")
    assert m in blocks and (bin(u).count("1"), bin(d).count("1")) == blocks[m] and max(u, d, s) < 1 << n_sites
    r, c = 0, 0
    for p in range(n_sites - 1, -1, -1):
        if (s >> p) & 1:
            r += A[p][c]
            c += 1
    return r + _colex_rank(d) * comb(n_sites, blocks[m][0]) + _colex_rank(u)


def fields(w, n_sites):
    """(u, d, s) of a word or an array of words"""
    w = np.asarray(w, dtype=np.uint64)
    m = np.uint64((1 << n_sites) - 1)
    n = np.uint64(n_sites)
    return w & m, (w >> n) & m, w >> (n + n)


def hop_terms(bonds, t=1.0):
    """-t (c+_i c_j + c+_j c_i) for both species on every bond (a bond listed twice counts twice)"""
    out = []
    for (i, j) in np.asarray(bonds, dtype=np.int64).reshape(-1, 2):
        out.append((int(i), int(j), -t, -t))
        out.append((int(j), int(i), -t, -t))
    return out


def exchange_terms(bonds, J):
    """isotropic J S_i . S_j between the local spins on every bond"""
    return [(int(i), int(j), J, J) for (i, j) in np.asarray(bonds, dtype=np.int64).reshape(-1, 2)]


def terms(n_sites, bonds, t=1.0, J_K=1.1, J_RKKY=0.0):
    """The Kondo lattice model of the reference's examples: hops -t both ways on every bond, J_K S_i . s_i on every site,
    J_RKKY S_i . S_j between the local spins on every bond."""
    return Terms(hop_terms(bonds, t), [J_K] * n_sites, [J_K] * n_sites, exchange_terms(bonds, J_RKKY) if J_RKKY != 0.0 else [])


def local_singlet_terms(n_sites, site):
    """Terms of the observable S_i . s_i on one site (no hops): apply it with spmv and take dotc for <S_i . s_i>."""
    k = [0.0] * n_sites
    k[site] = 1.0
    return Terms([], k, list(k), [])
