"""The operators between Kondo-lattice sectors, in numpy alone and independent of the device code: the reference of
tests/test_kondoops.py (which pins it by algebra), tests/test_gpu_kondo_mopr.py and tools/kondo_mopr_time.py.

Words, basis order and fermion convention are those of quantum_basis_amd.kondo: w = u | d << n | s << 2n (s: local spin DOWN),
ascending; the operator string is all up operators, then all down operators, sites ascending; the local spins commute with
everything.  Everything is written from the SOURCE word, straight from the definitions:
    c_{i,up} |u d s> = (-1)^popcount(u below i) |u \\ i, d, s>            c_{i,dn}: (-1)^(popcount(u) + popcount(d below i))
    c^dag: the same sign, the orbital empty before it acts
    s^+_i = c^dag_{i,up} c_{i,dn},  s^-_i = c^dag_{i,dn} c_{i,up}        the product, applied right to left
    S^+_i clears bit i of s (down -> up), S^-_i sets it                   element 1
A sector case is  B_new^dag O (B_old x)  with B[:, a] = (|G| |S_a|)^(-1/2) sum_g chi(g) T_g |a> over the orbit representatives a
(the smallest word of an orbit), T_g moving every operator to its image and sorting each electron species (the sign of the
sorting permutation); Sectors.project evaluates it in longdouble without forming a matrix."""
from fractions import Fraction
from math import comb

import numpy as np
import scipy.sparse as sp

from quantum_basis_amd import kondo

C_UP, C_DN, CDAG_UP, CDAG_DN, SPIN_PLUS, SPIN_MINUS = range(6)
OPS = (C_UP, C_DN, CDAG_UP, CDAG_DN, SPIN_PLUS, SPIN_MINUS)
TARGET = {C_UP: (-1, -1), C_DN: (-1, 1), CDAG_UP: (1, 1), CDAG_DN: (1, -1), SPIN_PLUS: (0, 2), SPIN_MINUS: (0, -2)}
LD, CLD = np.longdouble, np.clongdouble
PI_LD = 4 * np.arctan(LD(1))


def target(n_elec, two_sz, op):
    return n_elec + TARGET[op][0], two_sz + TARGET[op][1]


_PC16 = np.array([bin(v).count("1") for v in range(1 << 16)], dtype=np.int64)


def popcount(a):
    """of non-negative integers, sixteen bits at a time"""
    a = np.asarray(a, dtype=np.int64)
    c = _PC16[a & 0xffff]
    top = int(a.max()) if a.size else 0
    shift = 16
    while top >> shift:
        c = c + _PC16[(a >> shift) & 0xffff]
        shift += 16
    return c


# ---- the one-site operators on arrays of fields: (cols, u', d', s', sign), cols = the words the operator does not destroy ----
def fermion(u, d, s, i, species, create):
    """c_{i,species} (create = 0) or c^dag_{i,species} (create = 1), species 0 = up, 1 = down"""
    occ = d if species else u
    cols = np.flatnonzero(((occ >> i) & 1) == (0 if create else 1))
    u, d, s, occ = u[cols], d[cols], s[cols], occ[cols]
    par = popcount(occ & ((1 << i) - 1)) + (popcount(u) if species else 0)
    flipped = occ ^ (1 << i)
    return cols, (u if species else flipped), (flipped if species else d), s, 1 - 2 * (par & 1)


def electron_flip(u, d, s, i, plus):
    """s^+_i = c^dag_{i,up} c_{i,dn} (plus) or s^-_i = c^dag_{i,dn} c_{i,up}: the right factor first"""
    first, second = (1, 0) if plus else (0, 1)
    c1, u1, d1, s1, g1 = fermion(u, d, s, i, first, 0)
    c2, u2, d2, s2, g2 = fermion(u1, d1, s1, i, second, 1)
    return c1[c2], u2, d2, s2, g1[c2] * g2


def local_flip(u, d, s, i, plus):
    """S^+_i: the local spin of site i from down (bit set) to up; S^-_i the reverse"""
    cols = np.flatnonzero(((s >> i) & 1) == (1 if plus else 0))
    return cols, u[cols], d[cols], s[cols] ^ (1 << i), np.ones(len(cols), dtype=np.int64)


def site_parts(op, coef_elec, coef_spin):
    """[(function of (u, d, s, i), coefficient set), ...] of O = sum_i coef[i] O_i"""
    if op in (C_UP, C_DN, CDAG_UP, CDAG_DN):
        assert coef_spin is None
        return [(lambda u, d, s, i: fermion(u, d, s, i, op & 1, op >> 1), coef_elec)]
    plus = op == SPIN_PLUS
    parts = []
    if coef_elec is not None:
        parts.append((lambda u, d, s, i: electron_flip(u, d, s, i, plus), coef_elec))
    if coef_spin is not None:
        parts.append((lambda u, d, s, i: local_flip(u, d, s, i, plus), coef_spin))
    assert parts
    return parts


class Sector:
    """The words of (n_elec, two_sz), ascending, as int64 fields; index() finds words in it."""

    def __init__(self, n, n_elec, two_sz):
        self.n, self.n_elec, self.two_sz = n, n_elec, two_sz
        self.w = kondo.words(n, n_elec, two_sz).astype(np.int64)
        m = (1 << n) - 1
        self.u, self.d, self.s = self.w & m, (self.w >> n) & m, self.w >> (2 * n)
        self.N = len(self.w)
        self._tables = None

    def index(self, u, d, s):
        """positions of the words u | d << n | s << 2n, which must belong to the sector (checked against kondo.words).  By
        np.searchsorted, or, for many words, from three tables over the n-bit patterns: the words before the block of s, the
        rank of a pattern among those of its popcount and the number of up patterns of the block."""
        new = u | (d << self.n) | (s << (2 * self.n))
        if len(new) < (1 << self.n):
            r = np.minimum(np.searchsorted(self.w, new), self.N - 1)
        else:
            if self._tables is None:
                pats = np.arange(1 << self.n, dtype=np.int64)
                pc = popcount(pats)
                rk = np.zeros(len(pats), dtype=np.int64)
                for k in range(self.n + 1):
                    sel = np.flatnonzero(pc == k)
                    rk[sel] = np.arange(len(sel))
                blocks = {m: (nu, nd) for (nu, nd, m) in kondo.sector_blocks(self.n, self.n_elec, self.two_sz)}
                cu = np.array([comb(self.n, blocks[m][0]) if m in blocks else 0 for m in range(self.n + 1)], dtype=np.int64)
                wt = np.array([comb(self.n, blocks[m][0]) * comb(self.n, blocks[m][1]) if m in blocks else 0 for m in range(self.n + 1)],
                              dtype=np.int64)
                before = np.concatenate([[0], np.cumsum(wt[pc])[:-1]])
                self._tables = (before, rk, cu[pc])
            before, rk, cus = self._tables
            r = np.clip(before[s] + rk[d] * cus[s] + rk[u], 0, self.N - 1)
        assert np.array_equal(self.w[r], new)
        return r


def site_terms(src, dst, op, coef_elec=None, coef_spin=None):
    """yields (rows in dst, cols in src, signs, coef[i]) of coef[i] O_i for every site and part with a nonzero coefficient: the
    entries are coef[i] * signs; inside one site and part no row and no column repeats"""
    for fn, coef in site_parts(op, coef_elec, coef_spin):
        for i in range(src.n):
            if coef[i] == 0:
                continue
            cols, u2, d2, s2, sign = fn(src.u, src.d, src.s, i)
            yield dst.index(u2, d2, s2), cols, sign, complex(coef[i])


def operator(src, dst, op, coef_elec=None, coef_spin=None):
    """the sparse matrix of O from src to dst (scipy CSR, complex128), one stored entry per contribution"""
    r, c, v = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.complex128)]
    for rows, cols, sign, ci in site_terms(src, dst, op, coef_elec, coef_spin):
        r.append(rows); c.append(cols); v.append(ci * sign.astype(np.complex128))
    return sp.coo_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(dst.N, src.N))


def apply_full(src, dst, op, coef_elec, coef_spin, x):
    """(O x, n_i, sum_k |w_k| |x_k|) in longdouble: the contributions of every target row, their number and absolute sum"""
    y, ab, cnt = np.zeros(dst.N, dtype=CLD), np.zeros(dst.N, dtype=LD), np.zeros(dst.N, dtype=np.int64)
    xl, xa = x.astype(CLD), np.abs(x.astype(CLD))
    for rows, cols, sign, ci in site_terms(src, dst, op, coef_elec, coef_spin):
        y[rows] += CLD(ci) * _signed(xl[cols], sign)
        ab[rows] += abs(CLD(ci)) * xa[cols]
        cnt[rows] += 1
    return y, cnt, ab


def _signed(t, sign):
    """t with the entries of sign -1 negated (t is a fresh array)"""
    neg = sign < 0
    t[neg] = -t[neg]
    return t


# ---- momentum states ----
def chars_ld(turns):
    """exp(-2 pi i turns[g]) in longdouble from exact fractions of a turn"""
    a = np.array([LD(Fraction(t).numerator) / LD(Fraction(t).denominator) for t in turns], dtype=LD) * (2 * PI_LD)
    return np.cos(a).astype(CLD) - 1j * np.sin(a).astype(CLD)


def _pattern_tables(patterns, perm, fermion_sign):
    """image and sorting parity of every n-bit pattern in `patterns` under the site permutation perm"""
    n = len(perm)
    img = np.zeros(len(patterns), dtype=np.int64)
    par = np.zeros(len(patterns), dtype=np.int64)
    for i in range(n):
        img |= ((patterns >> i) & 1) << perm[i]
        if fermion_sign:
            for j in range(i + 1, n):
                if perm[i] > perm[j]:
                    par ^= (patterns >> i) & (patterns >> j) & 1
    return img, par


def translate(sec, perm, sel=None):
    """(u', d', s', sign) of T_g on the words of sec (or on sec's words sel): tables over the distinct patterns of each field"""
    out, par = [], 0
    for f, signed in ((sec.u, True), (sec.d, True), (sec.s, False)):
        f = f if sel is None else f[sel]
        if len(f) >= (1 << sec.n):
            pats, inv = np.arange(1 << sec.n, dtype=np.int64), f
        else:
            pats, inv = np.unique(f, return_inverse=True)
        img, p = _pattern_tables(pats, perm, signed)
        out.append(img[inv])
        par = par ^ p[inv]
    return out[0], out[1], out[2], 1 - 2 * par


class Momentum:
    """The momentum states of a sector: reps (positions in sec of the orbit representatives, ascending), stab = |S_a|,
    zero[a] = the state vanishes at this momentum, and for every g the position idx[g][a] of T_g a with the coefficient
    val[g][a] = chi(g) sign / sqrt(|G| |S_a|) (0 on zero-norm columns), in longdouble."""

    def __init__(self, sec, perms, turns):
        self.sec, G = sec, len(perms)
        assert list(perms[0]) == list(range(sec.n))
        cand = np.arange(sec.N)                            # the words no translation has made smaller yet
        for p in perms[1:]:
            u2, d2, s2, _ = translate(sec, p, cand)
            cand = cand[(u2 | (d2 << sec.n) | (s2 << (2 * sec.n))) >= sec.w[cand]]
        self.reps = cand
        self.dim = len(self.reps)
        chi = chars_ld(turns)
        self.idx, sgn = [], []
        for p in perms:
            u2, d2, s2, sg = translate(sec, p, self.reps)
            self.idx.append(sec.index(u2, d2, s2))
            sgn.append(sg)
        self.stab = sum((ix == self.reps).astype(np.int64) for ix in self.idx)
        ssum = sum(np.where(ix == self.reps, chi[g] * sg.astype(LD), 0) for g, (ix, sg) in enumerate(zip(self.idx, sgn)))
        self.zero = np.abs(ssum) < 1e-9
        norm = np.sqrt(LD(G) * self.stab.astype(LD))
        self.val = [np.where(self.zero, 0, chi[g] * sgn[g].astype(LD) / norm) for g in range(G)]

    def expand(self, x):
        """B x on the words of the sector (longdouble)"""
        y = np.zeros(self.sec.N, dtype=x.dtype)
        for ix, v in zip(self.idx, self.val):
            y[ix] += (v if np.iscomplexobj(x) else np.abs(v)) * x       # a real x asks for |B| |x|
        return y

    def contract(self, z):
        """B^dag z (or |B|^T z for a real z)"""
        out = np.zeros(self.dim, dtype=z.dtype)
        for ix, v in zip(self.idx, self.val):
            out += (np.conj(v) if np.iscomplexobj(z) else np.abs(v)) * z[ix]
        return out

    def matrix(self):
        """B as a scipy matrix in double (words x representatives)"""
        rows = np.concatenate(self.idx)
        cols = np.tile(np.arange(self.dim), len(self.idx))
        return sp.coo_matrix((np.concatenate(self.val).astype(np.complex128), (rows, cols)), shape=(self.sec.N, self.dim)).tocsc()


def project(mo, mn, op, coef_elec, coef_spin, x):
    """(B_new^dag O B_old x, n_i, sum_k |w_k| |x_k|) in longdouble for the momentum states mo (source) and mn (target).
    n_i counts the sites and parts whose one-site operator reaches the representative's own word from a word that B_old |x|
    occupies; the absolute sum is |B_new|^T |O| |B_old| |x|, which equals the sum over the contributions because the terms
    of a live orbit add with one phase."""
    src, dst = mo.sec, mn.sec
    full, fabs = mo.expand(x.astype(CLD)), mo.expand(np.abs(x.astype(CLD)))
    z, za, cnt = np.zeros(dst.N, dtype=CLD), np.zeros(dst.N, dtype=LD), np.zeros(dst.N, dtype=np.int64)
    for rows, cols, sign, ci in site_terms(src, dst, op, coef_elec, coef_spin):
        z[rows] += CLD(ci) * _signed(full[cols], sign)
        fa = fabs[cols]
        za[rows] += abs(CLD(ci)) * fa
        cnt[rows] += fa > 0
    n_i = np.where(mn.zero, 0, cnt[mn.reps])
    return mn.contract(z), n_i, mn.contract(za)


# ---- lattices and groups: (perms, turns) with the character of translation g = exp(-2 pi i turns[g]) ----
def chain(L, periodic=True):
    return [(i, (i + 1) % L) for i in range(L if periodic else L - 1)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], [Fraction(m * t, L) % 1 for t in range(L)]


def phases(turns):
    """exp(2 pi i turns) rounded to double from longdouble, the turns reduced to [0, 1) exactly: the coefficients carry their
    character to the last bit a double can hold"""
    return np.conj(chars_ld([Fraction(t) % 1 for t in turns])).astype(np.complex128)


def chain_coef(L, q, amp=0.7):
    """amp exp(2 pi i q s / L): under s -> s + t it picks up exp(2 pi i q t / L), so momentum m goes to m - q"""
    return amp * phases([Fraction(q * s, L) for s in range(L)])


def torus_site(Lx, Ly, x, y):
    return (x % Lx) + Lx * (y % Ly)


def torus_group(Lx, Ly, mx, my):
    perms, turns = [], []
    for ty in range(Ly):
        for tx in range(Lx):
            perms.append([torus_site(Lx, Ly, x + tx, y + ty) for y in range(Ly) for x in range(Lx)])
            turns.append((Fraction(mx * tx, Lx) + Fraction(my * ty, Ly)) % 1)
    return perms, turns


def torus_coef(Lx, Ly, qx, qy, amp=0.7):
    return amp * phases([Fraction(qx * x, Lx) + Fraction(qy * y, Ly) for y in range(Ly) for x in range(Lx)])


def chars_of(turns):
    """the characters handed to the library: the exact ones rounded to double"""
    return chars_ld(turns).astype(np.complex128)
