"""Independent host reference for the all-pair static correlations of a spin-1/2 MOMENTUM-SECTOR state (qbh_corr_spin_repr_dev),
in numpy longdouble, written from the formulas of the call with their sums over the translations g left in place (no pair
classes, no Hermiticity, no site orbits), plus the explicit route that pins it: unfold the state to the full space and evaluate
the operator definitions of tests/corrref.py there (tests/test_corrreprref.py).

Conventions (those of qbh_gen_heisenberg_repr): bit set = spin down; G = the n_trans site permutations perms[g][s]; a
translation carries the spin of site s to site perms[g][s]; the basis is ALL orbit representatives (the smallest word of every
orbit), ascending, a representative whose character sum over its stabiliser vanishes has zero norm and is ignored; the
momentum state of representative a is the normalised sum_g chi(g) T_g |a>.

Every value comes with A = the sum of the absolute values of the terms it is a sum of (the scale of its rounding error):
  norm2     sum_a |psi_a|^2                                                                       A = norm2
  sz[i]     sum_a |psi_a|^2 (1/|G|) sum_g s_{g(i)}(a)                                             A = norm2 / 2
  zz[i][j]  sum_a |psi_a|^2 (1/|G|) sum_g s_{g(i)}(a) s_{g(j)}(a)                                 A = norm2 / 4
  pm[i][j]  (1/|G|) sum_a sum_{g: a has g(i) up, g(j) down} conj(psi_a) conj(chi(g*)) sqrt(|S_b|/|S_a|) psi_b
            diagonal: sum_a |psi_a|^2 (1/|G|) sum_g (1/2 + s_{g(i)}(a)), the terms being the 1/2 and the s: A = norm2
"""
import functools

import numpy as np

import corrref

LD, CLD = np.longdouble, np.clongdouble
FAULTS = ("chi_not_conjugated", "no_sqrt", "zero_norm_counted")


# ------------------------------------------------------------------------------------------------------------ lattices --
def chain(n, k):
    """(perms, chars) of the n translations of a ring at momentum 2 pi k / n"""
    perms = np.array([[(s + g) % n for s in range(n)] for g in range(n)], dtype=np.int32)
    return perms, _chars([k * g / n for g in range(n)])


def cells_chain(n_cells, n_sub, k):
    """a ring of n_cells cells of n_sub sites (site = cell * n_sub + sublattice): n_cells translations"""
    n = n_cells * n_sub
    perms = np.array([[(s + g * n_sub) % n for s in range(n)] for g in range(n_cells)], dtype=np.int32)
    return perms, _chars([k * g / n_cells for g in range(n_cells)])


def torus(lx, ly, kx, ky, n_sub=1, only_x=False):
    """lx x ly cells of n_sub sites (site = (x + lx * y) * n_sub + sublattice) under all translations, or those along x only"""
    perms, phase = [], []
    for ty in range(1 if only_x else ly):
        for tx in range(lx):
            perms.append([(((x + tx) % lx) + lx * ((y + ty) % ly)) * n_sub + b for y in range(ly) for x in range(lx) for b in range(n_sub)])
            phase.append(kx * tx / lx + ky * ty / ly)
    return np.array(perms, dtype=np.int32), _chars(phase)


def _chars(turns):
    """exp(-2 pi i t) with the exact values where t is a multiple of 1/4 (real characters are exactly real)"""
    out = []
    for t in turns:
        q = (4 * t) % 4
        if abs(q - round(q)) < 1e-12:
            out.append([1, -1j, -1, 1j][int(round(q)) % 4])
        else:
            out.append(np.exp(-2j * np.pi * t))
    return np.array(out, dtype=np.complex128)


# -------------------------------------------------------------------------------------------------------------- basis --
def translate(words, perm):
    """images of the uint64 words under the site permutation perm"""
    out = np.zeros_like(words)
    for s, img in enumerate(perm):
        out |= ((words >> np.uint64(s)) & np.uint64(1)) << np.uint64(int(img))
    return out


class Sector:
    """the representatives of the (n_sites, n_dn) words under perms, and for every word its representative and translation"""

    def __init__(self, n_sites, n_dn, perms, chars):
        self.N, self.n_dn = n_sites, n_dn
        self.perms, self.chars = np.asarray(perms), np.asarray(chars, dtype=np.complex128)
        self.G = len(self.perms)
        pat = corrref.patterns(n_sites, n_dn)
        best, gstar = pat.copy(), np.zeros(len(pat), dtype=np.int64)
        nstab, chisum = np.zeros(len(pat), dtype=np.int64), np.zeros(len(pat), dtype=np.complex128)
        for g in range(self.G):
            img = translate(pat, self.perms[g])
            less = img < best                                    # the first translation that reaches the smallest image
            best, gstar = np.where(less, img, best), np.where(less, g, gstar)
            same = img == pat
            nstab += same
            chisum += np.where(same, self.chars[g], 0)
        is_rep = best == pat
        self.pat = pat
        self.reps = pat[is_rep]                                  # ascending
        self.nstab = nstab[is_rep]
        self.zero = (np.abs(chisum[is_rep]) ** 2 < 1e-20)
        self.rep_of = np.searchsorted(self.reps, best)           # per word: the position of its representative
        self.gstar = gstar
        self.dim = len(self.reps)


@functools.lru_cache(maxsize=None)
def _sector_cached(n_sites, n_dn, perms_bytes, chars_bytes, n_trans):
    perms = np.frombuffer(perms_bytes, dtype=np.int32).reshape(n_trans, n_sites)
    return Sector(n_sites, n_dn, perms, np.frombuffer(chars_bytes, dtype=np.complex128))


def sector(n_sites, n_dn, perms, chars):
    p, c = np.ascontiguousarray(perms, dtype=np.int32), np.ascontiguousarray(chars, dtype=np.complex128)
    return _sector_cached(n_sites, n_dn, p.tobytes(), c.tobytes(), len(p))


# ---------------------------------------------------------------------------------------------------------- reference --
def spin_repr(n_sites, n_dn, perms, chars, psi, fault=None):
    """dict(norm2, sz, zz, pm, A=dict(the same keys), dim, zero) from the representatives alone; fault: one of FAULTS, a
    deliberately wrong variant that the comparison with the explicit route has to reject"""
    assert fault is None or fault in FAULTS
    S = sector(n_sites, n_dn, perms, chars)
    N, G = n_sites, S.G
    assert len(psi) == S.dim
    p = np.asarray(psi).astype(CLD)
    live = np.ones(S.dim, dtype=bool) if fault == "zero_norm_counted" else ~S.zero
    w = np.where(live, np.abs(p) ** 2, LD(0)).astype(LD)
    norm2 = np.sum(w)
    down = [((S.reps >> np.uint64(s)) & np.uint64(1)).astype(bool) for s in range(N)]
    s_of = [np.where(d, LD(-0.5), LD(0.5)) for d in down]
    site = np.array([np.sum(w * s_of[s]) for s in range(N)], dtype=LD)
    pair = np.array([[np.sum(w * s_of[a] * s_of[b]) for b in range(N)] for a in range(N)], dtype=LD)
    # T[p][q] = sum over the representatives with p up and q down of the term of the flipped word
    chi = S.chars if fault == "chi_not_conjugated" else np.conj(S.chars)
    T, TA = np.zeros((N, N), dtype=CLD), np.zeros((N, N), dtype=LD)
    for a in range(N):
        for b in range(N):
            if a == b:
                continue
            hit = ~S.zero & ~down[a] & down[b]
            if not hit.any():
                continue
            rows = np.nonzero(hit)[0]
            c = S.reps[rows] ^ np.uint64((1 << a) | (1 << b))
            at = np.searchsorted(S.pat, c)
            assert np.all(S.pat[at] == c)
            tgt, g = S.rep_of[at], S.gstar[at]
            ok = ~S.zero[tgt]
            ratio = np.ones(len(rows), dtype=LD) if fault == "no_sqrt" else np.sqrt(S.nstab[tgt].astype(LD) / S.nstab[rows].astype(LD))
            term = np.conj(p[rows]) * chi[g].astype(CLD) * ratio * p[tgt]
            T[a, b] = np.sum(term[ok])
            TA[a, b] = np.sum(np.abs(term[ok]))
    out = {"norm2": norm2, "sz": np.zeros(N, dtype=LD), "zz": np.zeros((N, N), dtype=LD), "pm": np.zeros((N, N), dtype=CLD),
           "dim": S.dim, "zero": S.zero}
    A = {"norm2": norm2, "sz": np.full(N, norm2 / 2, dtype=LD), "zz": np.full((N, N), norm2 / 4, dtype=LD), "pm": np.zeros((N, N), dtype=LD)}
    for g in range(G):                                           # the sums over g of the formulas, one image of every (i, j) each
        pg = S.perms[g]
        out["sz"] += site[pg] / LD(G)
        out["zz"] += pair[np.ix_(pg, pg)] / LD(G)
        out["pm"] += T[np.ix_(pg, pg)] / LD(G)
        A["pm"] += TA[np.ix_(pg, pg)] / LD(G)
    for i in range(N):
        out["pm"][i, i] = norm2 / 2 + out["sz"][i]
        A["pm"][i, i] = norm2
    out["A"] = A
    return out


# ----------------------------------------------------------------------------------------------------- explicit route --
def unfold(n_sites, n_dn, perms, chars, psi):
    """the full-space vector (order of corrref.patterns): Psi[T_g a] += chi(g) psi_a, every column normalised on its own, the
    columns of zero norm left out"""
    S = sector(n_sites, n_dn, perms, chars)
    p = np.asarray(psi).astype(CLD)
    full = np.zeros(len(S.pat), dtype=CLD)
    for r in range(S.dim):
        col = np.zeros(len(S.pat), dtype=CLD)
        word = S.reps[r:r + 1]
        for g in range(S.G):
            col[np.searchsorted(S.pat, translate(word, S.perms[g])[0])] += CLD(S.chars[g])
        nrm = np.sqrt(np.sum(np.abs(col) ** 2))
        if nrm < 1e-9:
            assert S.zero[r]
            continue
        assert not S.zero[r]
        full += p[r] * col / nrm
    return full


def explicit(n_sites, n_dn, perms, chars, psi):
    """corrref.spin on the unfolded state (clongdouble all the way)"""
    return corrref.spin(n_sites, n_dn, unfold(n_sites, n_dn, perms, chars, psi))
