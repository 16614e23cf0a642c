"""Independent host reference for the all-pair static correlations of a two-species fermion MOMENTUM-SECTOR state
(qbh_corr_hubbard_repr_dev), in numpy longdouble, written from the formulas of the call with their sums over the group elements g
left in place (no pair classes, no Hermiticity, no site orbits), plus the explicit route that pins it: unfold the state to the full
space with the fermion signs, move it to the order of qbh_gen_hubbard and evaluate the operator definitions of tests/corrref.py
there (tests/test_corrhubreprref.py).

Conventions (those of qbh_gen_hubbard_repr): word = u | d << N with the operator order "all up (ascending site), then all down";
G = the n_trans site permutations perms[g][s]; T_g |u, d> = sgn(g, u) sgn(g, d) |g(u), g(d)>, sgn the parity of the permutation that
sorts the images of the occupied sites (secforms._images); the basis is ALL orbit representatives (the smallest word of every
orbit), ascending; a representative whose SIGNED character sum over its stabiliser vanishes has zero norm and is ignored; the
momentum state of representative a is the normalised sum_g chi(g) T_g |a>.  With no_double the words with a doubly occupied site
are not in the space.  The enumeration (images, parities, representatives, |S_a|) is taken from secforms._images; the matrix
elements of the operators are NOT taken from the 'between' masks of the kernels but from corrref._fermi_apply: the candidate word c
is built with bit operations and <a| O |c> = +-1 is read off by applying the factors of O to c one by one.

Every value comes with A = the sum of the absolute values of the terms it is a sum of (the scale of its rounding error), w_a =
|psi_a|^2 over the representatives of nonzero norm:
  norm2           sum_a w_a                                                                               A = norm2
  dens[s][i]      sum_a w_a (1/|G|) sum_g n_{g(i),s}(a)                                                   A = the value
  nn[2A+B][i][j]  sum_a w_a (1/|G|) sum_g n_{g(i),A}(a) n_{g(j),B}(a)   (i = j included)                  A = the value
  hop[s][i][j]    (1/|G|) sum_a sum_{g: a has g(i) occupied, g(j) empty in s} conj(psi_a) <a|c+_{g(i)} c_{g(j)}|c> sigma(g*)
                  conj(chi(g*)) sqrt(|S_b|/|S_a|) psi_b,  T_{g*} |c> = sigma |b>;  targets of zero norm (and, with no_double, targets
                  with a doubly occupied site) skipped;  diagonal: dens[s][i]                              A = sum of the |terms|
  flip[i][j]      the same with <a| c+_{g(i),up} c_{g(i),dn} c+_{g(j),dn} c_{g(j),up} |c>;  diagonal: sum_a w_a (1/|G|) sum_g
                  (n_up - n_up n_dn)_{g(i)}(a), the terms being the n_up and the n_up n_dn: A = dens[0][i] + nn[1][i][i]

Bound of the GPU test: |got - want| <= (dim |G| + C_ROUND) 2^-53 A.  dim |G| bounds the number of terms of an entry (every
representative contributes at most one term per group element), so it covers the additions of the sum in any order; C_ROUND counts
the roundings of ONE term in k_corr_hubrepr before it is added, and the host's one division afterwards:
  gathered term: |S_b| / |S_a| (1), its square root (1), the product with the character (1; the sign is exact), the complex product
  with psi_b (two products and an addition per component: 3), the product with conj(psi_a) (3), the division by 2 n_u on the
  host (1): 10.
  diagonal groups: w_a = fma(re, re, im * im) (2), w_a times the integer count (1), the division by n_u or n_s (1): 4; the flip
  diagonal subtracts two such values (1 more): 5.
C_ROUND = 10."""
import functools

import numpy as np

import corrref
from refham import bit_patterns
from secforms import _images, _dihedral               # noqa: F401  (_dihedral re-exported for the tests)

LD, CLD = np.longdouble, np.clongdouble
C_ROUND = 10
FAULTS = ("chi_not_conjugated", "no_sigma", "no_hop_sign", "no_sqrt", "zero_norm_counted", "ud_swapped")
KEYS = ("norm2", "dens", "nn", "hop", "flip")


# ------------------------------------------------------------------------------------------------------------ lattices --
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


def ring(n, k):
    """(perms, chars) of the n translations of a ring at momentum 2 pi k / n"""
    perms = np.array([[(s + g) % n for s in range(n)] for g in range(n)], dtype=np.int32)
    return perms, _chars([k * g / n for g in range(n)])


def torus(lx, ly, kx, ky):
    """lx x ly sites (site = x + lx * y) under all translations at momentum (2 pi kx / lx, 2 pi ky / ly)"""
    perms, phase = [], []
    for ty in range(ly):
        for tx in range(lx):
            perms.append([((x + tx) % lx) + lx * ((y + ty) % ly) for y in range(ly) for x in range(lx)])
            phase.append(kx * tx / lx + ky * ty / ly)
    return np.array(perms, dtype=np.int32), _chars(phase)


def dihedral(n, sign):
    """the 2n rotations and reflections of a ring (secforms._dihedral); the trivial representation, or the one that is -1 on the
    reflections"""
    chars = np.array([1.0] * n + [-1.0 if sign else 1.0] * n, dtype=np.complex128)
    return np.array(_dihedral(n), dtype=np.int32), chars


def identity(n):
    return np.arange(n, dtype=np.int32)[None, :], np.ones(1, dtype=np.complex128)


# -------------------------------------------------------------------------------------------------------------- basis --
class Sector:
    """for every word (index = rank(d) * C(n, nu) + rank(u), the ascending order of the words): its smallest image, the first group
    element that reaches it and the sign of that element on the word; the representatives, |S_a| and which norms vanish"""

    def __init__(self, n, nu, nd, perms, chars, no_double):
        self.n, self.nu, self.nd = n, nu, nd
        self.perms, self.chars = np.asarray(perms, dtype=np.int64), np.asarray(chars, dtype=np.complex128)
        self.G = len(self.perms)
        assert np.array_equal(self.perms[0], np.arange(n))
        self.ups, self.dns = bit_patterns(n, nu), bit_patterns(n, nd)
        cu, cd = len(self.ups), len(self.dns)
        self.cu, self.cd = cu, cd
        img_u, par_u = _images(self.ups, self.perms, n)
        img_d, par_d = _images(self.dns, self.perms, n)
        self.rank_u, self.rank_d = np.searchsorted(self.ups, img_u), np.searchsorted(self.dns, img_d)
        self.par_u, self.par_d = par_u, par_d
        nw = cu * cd
        me = np.arange(nw, dtype=np.int64)
        wd, wu = np.divmod(me, cu)
        best, gstar, sigma = me.copy(), np.zeros(nw, dtype=np.int64), np.ones(nw, dtype=np.int64)
        nstab, csum = np.zeros(nw, dtype=np.int64), np.zeros(nw, dtype=np.complex128)
        for g in range(self.G):
            im = self.rank_d[g][wd] * cu + self.rank_u[g][wu]
            sg = 1 - 2 * (par_u[g][wu] ^ par_d[g][wd])
            lt = im < best                                           # the first element that reaches the smallest image
            best[lt], gstar[lt], sigma[lt] = im[lt], g, sg[lt]
            eq = im == me
            nstab += eq
            csum[eq] += self.chars[g] * sg[eq]
        allowed = (self.ups[wu] & self.dns[wd]) == 0 if no_double else np.ones(nw, dtype=bool)
        self.best, self.gstar, self.sigma = best, gstar, sigma
        rep = np.nonzero((best == me) & allowed)[0]
        self.dim = len(rep)
        self.pos = np.full(nw, -1, dtype=np.int64)
        self.pos[rep] = np.arange(self.dim)
        self.row_u, self.row_d = wu[rep], wd[rep]
        self.U, self.D = self.ups[self.row_u], self.dns[self.row_d]
        self.reps = self.U | (self.D << n)                           # ascending
        assert np.all(np.diff(self.reps) > 0)
        self.nstab = nstab[rep]
        self.zero = np.abs(csum[rep]) ** 2 < 1e-20
        assert np.all(np.abs(np.abs(csum[rep]) - np.where(self.zero, 0, self.nstab)) < 1e-9)

    def index(self, u, d):
        """index of the words u | d << n"""
        ru, rd = np.searchsorted(self.ups, u), np.searchsorted(self.dns, d)
        assert np.all(self.ups[ru] == u) and np.all(self.dns[rd] == d)
        return rd * self.cu + ru


@functools.lru_cache(maxsize=None)
def _sector_cached(n, nu, nd, perms_bytes, chars_bytes, n_trans, no_double):
    perms = np.frombuffer(perms_bytes, dtype=np.int32).reshape(n_trans, n)
    return Sector(n, nu, nd, perms, np.frombuffer(chars_bytes, dtype=np.complex128), no_double)


def sector(n, nu, nd, perms, chars, no_double=False):
    p, c = np.ascontiguousarray(perms, dtype=np.int32), np.ascontiguousarray(chars, dtype=np.complex128)
    return _sector_cached(n, nu, nd, p.tobytes(), c.tobytes(), len(p), bool(no_double))


# ---------------------------------------------------------------------------------------------------------- reference --
def _element(S, a_words, c_words, ops):
    """<a| O |c> for O = the product of ops = [(kind, orbital), ...] (the leftmost factor first), from corrref._fermi_apply"""
    w = c_words.astype(np.uint64)
    amp, alive = np.ones(len(w)), np.ones(len(w), dtype=bool)
    for kind, orb in reversed(ops):
        w, amp, alive = corrref._fermi_apply(w, amp, alive, kind, orb)
    assert alive.all() and np.all(w == a_words.astype(np.uint64))
    return amp


def hubbard_repr(n, nu, nd, perms, chars, psi, no_double=False, fault=None):
    """dict(norm2, dens, nn, hop, flip, A=dict(the same keys), dim, zero) from the representatives alone; fault: one of FAULTS, a
    deliberately wrong variant that the comparison with the explicit route has to reject"""
    assert fault is None or fault in FAULTS
    S = sector(n, nu, nd, perms, chars, no_double)
    N, G = n, S.G
    assert len(psi) == S.dim
    p = np.asarray(psi).astype(CLD)
    live = np.ones(S.dim, dtype=bool) if fault == "zero_norm_counted" else ~S.zero
    w = np.where(live, np.abs(p) ** 2, LD(0)).astype(LD)
    norm2 = np.sum(w)
    occ = [[((X >> s) & 1).astype(LD) for s in range(N)] for X in (S.U, S.D)]          # occ[species][site]
    site = np.array([[np.sum(w * occ[s][a]) for a in range(N)] for s in (0, 1)], dtype=LD)
    pair = np.array([[[np.sum(w * occ[sa][a] * occ[sb][b]) for b in range(N)] for a in range(N)] for sa in (0, 1) for sb in (0, 1)], dtype=LD)
    if fault == "ud_swapped":
        pair = pair[[0, 2, 1, 3]]
    chi = (S.chars if fault == "chi_not_conjugated" else np.conj(S.chars)).astype(CLD)
    words = S.reps
    ok_row = ~S.zero
    # T[kind][a][b] = sum over the representatives of the terms of the one operator with sites (a, b): kind 0 / 1 hop of up / down
    T, TA = np.zeros((3, N, N), dtype=CLD), np.zeros((3, N, N), dtype=LD)
    for kind in range(3):
        for a in range(N):
            for b in range(N):
                if a == b:
                    continue
                ba, bb = np.int64(1) << a, np.int64(1) << b
                if kind < 2:
                    X, Y = (S.U, S.D) if kind == 0 else (S.D, S.U)
                    hit = ok_row & ((X & ba) != 0) & ((X & bb) == 0)                   # the particle moves from a to b
                    if no_double:
                        hit &= (Y & bb) == 0
                    rows = np.nonzero(hit)[0]
                    X2 = X[rows] ^ ba ^ bb
                    cu_, cd_ = (X2, S.D[rows]) if kind == 0 else (S.U[rows], X2)
                    ops = [(1, a + kind * N), (2, b + kind * N)]
                else:
                    hit = ok_row & ((S.U & ba) != 0) & ((S.D & ba) == 0) & ((S.D & bb) != 0) & ((S.U & bb) == 0)
                    rows = np.nonzero(hit)[0]
                    cu_, cd_ = S.U[rows] ^ ba ^ bb, S.D[rows] ^ ba ^ bb
                    ops = [(1, a), (2, a + N), (1, b + N), (2, b)]
                if len(rows) == 0:
                    continue
                amp = _element(S, words[rows], cu_ | (cd_ << N), ops)
                if fault == "no_hop_sign":
                    amp = np.ones(len(rows))
                at = S.index(cu_, cd_)
                tgt, g = S.pos[S.best[at]], S.gstar[at]
                assert np.all(tgt >= 0)
                sig = np.ones(len(rows)) if fault == "no_sigma" else S.sigma[at]
                ok = ~S.zero[tgt]
                ratio = np.ones(len(rows), dtype=LD) if fault == "no_sqrt" else np.sqrt(S.nstab[tgt].astype(LD) / S.nstab[rows].astype(LD))
                term = np.conj(p[rows]) * (amp * sig).astype(LD) * chi[g] * ratio * p[tgt]
                T[kind, a, b] = np.sum(term[ok])
                TA[kind, a, b] = np.sum(np.abs(term[ok]))
    out = {"norm2": norm2, "dens": np.zeros((2, N), dtype=LD), "nn": np.zeros((4, N, N), dtype=LD), "hop": np.zeros((2, N, N), dtype=CLD),
           "flip": np.zeros((N, N), dtype=CLD), "dim": S.dim, "zero": S.zero}
    A = {"norm2": norm2, "hop": np.zeros((2, N, N), dtype=LD), "flip": np.zeros((N, N), dtype=LD)}
    for g in range(G):                                               # the sums over g of the formulas, one image of every (i, j) each
        pg = S.perms[g]
        out["dens"] += site[:, pg] / LD(G)
        out["nn"] += pair[:, pg][:, :, pg] / LD(G)
        out["hop"] += T[:2][:, pg][:, :, pg] / LD(G)
        out["flip"] += T[2][np.ix_(pg, pg)] / LD(G)
        A["hop"] += TA[:2][:, pg][:, :, pg] / LD(G)
        A["flip"] += TA[2][np.ix_(pg, pg)] / LD(G)
    A["dens"], A["nn"] = out["dens"].copy(), out["nn"].copy()
    for i in range(N):
        for s in (0, 1):
            out["hop"][s, i, i] = A["hop"][s, i, i] = out["dens"][s, i]
        out["flip"][i, i] = out["dens"][0, i] - out["nn"][1, i, i]
        A["flip"][i, i] = out["dens"][0, i] + out["nn"][1, i, i]
    out["A"] = A
    return out


# ----------------------------------------------------------------------------------------------------- explicit route --
def unfold(n, nu, nd, perms, chars, psi, no_double=False):
    """the full-space vector in the order of qbh_gen_hubbard (row = rank(u) * C(n, nd) + rank(d)): Psi[T_g a] += chi(g) sgn(g, a)
    psi_a, every column normalised on its own, the columns of zero norm left out"""
    S = sector(n, nu, nd, perms, chars, no_double)
    p = np.asarray(psi).astype(CLD)
    M = np.zeros((S.cu * S.cd, S.dim), dtype=CLD)
    cols = np.arange(S.dim)
    for g in range(S.G):
        idx = S.rank_d[g][S.row_d] * S.cu + S.rank_u[g][S.row_u]
        sg = 1 - 2 * (S.par_u[g][S.row_u] ^ S.par_d[g][S.row_d])
        np.add.at(M, (idx, cols), (S.chars[g] * sg).astype(CLD))
    nrm = np.sqrt(np.sum(np.abs(M) ** 2, axis=0))
    alive = nrm > 1e-9
    assert np.array_equal(alive, ~S.zero)
    full = M[:, alive] @ (p[alive] / nrm[alive])
    return full.reshape(S.cd, S.cu).T.reshape(-1)                     # [rd][ru] -> ru * cd + rd


def explicit(n, nu, nd, perms, chars, psi, no_double=False):
    """corrref.hubbard on the unfolded state (clongdouble all the way)"""
    return corrref.hubbard(n, nu, nd, unfold(n, nu, nd, perms, chars, psi, no_double))


def to_generator_order(n, nu, nd, x):
    """a full-space vector indexed by the ascending words (rank(d) * C(n, nu) + rank(u)) in the order of qbh_gen_hubbard"""
    cu, cd = len(bit_patterns(n, nu)), len(bit_patterns(n, nd))
    return np.ascontiguousarray(np.asarray(x).reshape(cd, cu).T.reshape(-1))
