"""Independent host reference for the all-pair static correlations (qbh_corr_spin_dev / qbh_corr_hubbard_dev), written from the
operator definitions: every elementary operator acts on the bit patterns of the colex-ordered basis states with explicit bit
operations and fermion signs, and every expectation value is summed in longdouble / clongdouble.  Nothing here shares a formula
with the kernels (no 'between' masks, no chunk tables, no D_ij shortcut); tests/test_corrref.py pins it against Kronecker-product
operators in the full 2^N / 4^N space.

Conventions (those of qbh_gen_heisenberg / qbh_gen_hubbard / qbh_mopr_terms_dev):
  spin-1/2   basis state = pattern of the DOWN spins, rank = colexicographic = ascending pattern
  fermions   orbital o = site + species * N (species 0 = up, 1 = down), word w = u | d << N, |w> = prod_{o ascending} c+_o |0>,
             c+_o |w> = (-1)^(occupied orbitals below o) |w + o>; row = rank(u) * C(N, n_dn) + rank(d)
All values are raw bilinear forms <psi| O |psi>: nothing is divided by <psi|psi>."""
import functools
import itertools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble


@functools.lru_cache(maxsize=None)
def patterns(n_sites, n):
    """Ascending bit patterns with n bits set among n_sites (uint64, read-only): the colex order."""
    out = [sum(1 << b for b in c) for c in itertools.combinations(range(n_sites), n)]
    a = np.array(sorted(out), dtype=np.uint64)
    a.setflags(write=False)
    return a


def _popcount(x):
    x = x.copy()
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def _expect(psi, src_alive, amp, target_index):
    """sum over the live source states s of conj(psi[target(s)]) * amp(s) * psi[s], in clongdouble"""
    if not src_alive.any():
        return CLD(0)
    p = psi.astype(CLD)
    return np.sum(np.conj(p[target_index[src_alive]]) * amp[src_alive].astype(LD) * p[src_alive])


# ------------------------------------------------------------------------------------------------------------ spin-1/2 --
def _spin_apply(w, amp, alive, kind, site):
    """one of S^z (0), S^+ (1: down -> up), S^- (2: up -> down) at `site` on the patterns w (bit set = down)"""
    bit = np.uint64(1 << site)
    down = (w & bit) != 0
    if kind == 0:
        return w, amp * np.where(down, -0.5, 0.5), alive
    if kind == 1:
        return np.where(down, w ^ bit, w), amp, alive & down
    return np.where(down, w, w ^ bit), amp, alive & ~down


def spin_expect(n_sites, n_dn, psi, ops):
    """<psi| O_0 O_1 ... |psi> for ops = [(kind, site), ...], O_0 the leftmost factor (the rightmost acts first); the product must
    return to the sector."""
    pat = patterns(n_sites, n_dn)
    w, amp, alive = pat.copy(), np.ones(len(pat)), np.ones(len(pat), dtype=bool)
    for kind, site in reversed(list(ops)):
        w, amp, alive = _spin_apply(w, amp, alive, kind, site)
    idx = np.searchsorted(pat, w)
    idx = np.where(alive, idx, 0)
    assert np.all(pat[idx[alive]] == w[alive])
    return _expect(np.asarray(psi), alive, amp, idx)


def spin(n_sites, n_dn, psi):
    """dict(norm2, sz[N], zz[N][N], pm[N][N]) of a vector of the (n_sites, n_dn) sector"""
    N = n_sites
    psi = np.asarray(psi)
    out = {"norm2": np.sum(np.abs(psi.astype(CLD)) ** 2).real.astype(LD), "sz": np.zeros(N, dtype=LD), "zz": np.zeros((N, N), dtype=LD),
           "pm": np.zeros((N, N), dtype=CLD)}
    for i in range(N):
        out["sz"][i] = spin_expect(N, n_dn, psi, [(0, i)]).real
        for j in range(N):
            out["zz"][i, j] = spin_expect(N, n_dn, psi, [(0, i), (0, j)]).real
            out["pm"][i, j] = spin_expect(N, n_dn, psi, [(1, i), (2, j)])
    return out


# ------------------------------------------------------------------------------------------------- two-species fermions --
def _fermi_apply(w, amp, alive, kind, orb):
    """one of n_o (0), c+_o (1), c_o (2) on the words w"""
    bit = np.uint64(1 << orb)
    occ = (w & bit) != 0
    if kind == 0:
        return w, amp, alive & occ
    sign = np.where(_popcount(w & np.uint64((1 << orb) - 1)) % 2 == 1, -1.0, 1.0)
    ok = ~occ if kind == 1 else occ
    return np.where(ok, w ^ bit, w), amp * sign, alive & ok


class HubbardBasis:
    def __init__(self, n_sites, n_up, n_dn):
        self.N = n_sites
        self.cu, self.cd = patterns(n_sites, n_up), patterns(n_sites, n_dn)
        self.words = (self.cu[:, None] | (self.cd[None, :] << np.uint64(n_sites))).reshape(-1)       # row = ru * Nd + rd

    def index(self, w, alive):
        N = self.N
        u, d = w & np.uint64((1 << N) - 1), w >> np.uint64(N)
        ru, rd = np.searchsorted(self.cu, u), np.searchsorted(self.cd, d)
        ru, rd = np.where(alive, ru, 0), np.where(alive, rd, 0)
        assert np.all(self.cu[ru[alive]] == u[alive]) and np.all(self.cd[rd[alive]] == d[alive])
        return ru * len(self.cd) + rd


def hubbard_expect(basis, psi, ops):
    """<psi| O_0 O_1 ... |psi> for ops = [(kind, site, species), ...], O_0 the leftmost factor"""
    w = basis.words.copy()
    amp, alive = np.ones(len(w)), np.ones(len(w), dtype=bool)
    for kind, site, sp in reversed(list(ops)):
        w, amp, alive = _fermi_apply(w, amp, alive, kind, site + sp * basis.N)
    return _expect(np.asarray(psi), alive, amp, basis.index(w, alive))


def hubbard(n_sites, n_up, n_dn, psi):
    """dict(norm2, dens[2][N], nn[4][N][N] (uu, ud, du, dd), hop[2][N][N], flip[N][N])"""
    N = n_sites
    B = HubbardBasis(N, n_up, n_dn)
    psi = np.asarray(psi)
    out = {"norm2": np.sum(np.abs(psi.astype(CLD)) ** 2).real.astype(LD), "dens": np.zeros((2, N), dtype=LD),
           "nn": np.zeros((4, N, N), dtype=LD), "hop": np.zeros((2, N, N), dtype=CLD), "flip": np.zeros((N, N), dtype=CLD)}
    for i in range(N):
        for s in (0, 1):
            out["dens"][s, i] = hubbard_expect(B, psi, [(0, i, s)]).real
        for j in range(N):
            for a in (0, 1):
                for b in (0, 1):
                    out["nn"][2 * a + b, i, j] = hubbard_expect(B, psi, [(0, i, a), (0, j, b)]).real
            for s in (0, 1):
                out["hop"][s, i, j] = hubbard_expect(B, psi, [(1, i, s), (2, j, s)])
            out["flip"][i, j] = hubbard_expect(B, psi, [(1, i, 0), (2, i, 1), (1, j, 1), (2, j, 0)])
    return out
