"""Independent host reference for the all-pair correlations and string order of a d-level MOMENTUM-SECTOR state
(qbh_corr_qudit_repr_dev), in numpy longdouble, computed from the representatives alone by the class formulas of the call, plus the
explicit route that pins it: unfold the state to the full sector in generator order and evaluate the operator definitions of
tests/quditcorrref.py there (tests/test_quditcorrreprref.py).

Conventions (those of qbh_gen_qudit_repr): site s holds its level in bits [s b, (s + 1) b) of the word; G = the n_trans site
permutations perms[g][s], T_g carries the level of site s to site perms[g][s]; the basis is ALL orbit representatives (the smallest
word of every orbit), ascending; a representative whose character sum over its stabiliser vanishes has zero norm and is ignored; the
momentum state of representative a is the normalised sum_g chi(g) T_g |a>.  Words are handled as packed keys; a target word is
canonicalised by translating it (12-bit slices of the key through a table per group element) and found among the representatives by
search.  The orbits of sites, ordered site pairs and decorated strings are found by breadth-first closure under the permutations.

With w_a = |psi_a|^2 over the representatives of nonzero norm, every value comes with A = the sum of the absolute values of the
terms it is a sum of (the scale of its rounding error):
  norm2           sum_a w_a                                                                                  A = norm2
  pop[s][l]       sum_a w_a (1/n_s) #{p in the orbit of s: l_p = l}                                          A = the value
  dd[a][b][i][j]  sum_a w_a (1/|O|) sum_{(p,q) in O(i,j)} f_a(l_p) f_b(l_q); a class is an orbit O (forward) and its mirror image:
                  the forward orbit is summed, the mirror orientation carries dd[b][a]; a class that is its own mirror holds both
                  orientations in O; diagonal sum_l pop[i][l] f_a(l) f_b(l)                                   A = sum of the |terms|
  str[i][j]       i < j, mirrored: sum_a w_a (1/|orbit(m)|) sum_{m' in orbit(m)} h(l_e1') h(l_e2') prod_{k in M'} g(l_k),
                  m = ({i, j}, {k: i < k < j}), the group acting on ends and middle set site by site; diagonal sum_l pop h(l)^2
  aa[i][j]        (1/|O|) sum_a sum_{(p,q) in O, l_p >= 1, l_q <= d-2} lower[l_p] lower[l_q + 1] sqrt(|S_b|/|S_a|) chi(g*)
                  conj(psi_b) psi_a, c = a with l_p - 1 and l_q + 1, b = g* c (zero-norm targets skipped); forward orbit only, the
                  mirror orientation gets the conjugate; a class that is its own mirror sums both orientations and its value is
                  real (the imaginary part is set to 0, as the call does); diagonal sum_l pop[i][l] lower[l + 1]^2

Bound of the GPU test: |got - want| <= (dim |G| + n_sites + C_ROUND) 2^-53 A, C_ROUND = 10.  dim |G| bounds the number of terms
of an entry (a representative contributes at most one term per member of an orbit, and an orbit has at most |G| members), so it covers
the additions in any order, the two-stage sum included.  n_sites + C_ROUND counts the roundings of ONE term in k_corr_quditrepr
before it is added, and the host's division afterwards:
  str: h h (1); a level with n middle sites contributes gpow[l][n] = g(l)^n, rounded once from long double, and one product --
       nothing for n = 0 (the factor is 1), one rounding for n = 1 (g itself is exact), two for n >= 2: at most n, so at most
       |M| <= n_sites - 2 in all; w_a = fma(re, re, im im) (2); w_a times the sum of the row (1); the division by the number of
       members (1): at most n_sites + 3.
  aa:  |S_b| / |S_a| (1), its square root (1), lower lower (1), their product (1), times the character (1), conj(psi_b) psi_a (two
       products and an addition per component: 3), the complex product of the two (3), the division (1): 12 <= n_sites + 10 wherever
       a pair of sites exists.
  dd:  w_a (2), f f (1), times w_a (1), the division (1): 5.  pop and norm2: w_a (2), times the count (1), the division (1): 4.
  diagonals of dd / str / aa: a sum of at most d <= 8 products pop[i][l] (f f): pop (4), f f (1), the product (1) and at most
       min(d, dim) - 1 further additions of nonzero terms, within n_sites + 10 for every shape with more than one site.
So the implementation stays within the constant the bound was stated with."""
import functools

import numpy as np

import quditcorrref
import quditforms as qf
from corrhubreprref import ring, torus, dihedral, identity        # noqa: F401  (the lattices of the sibling references)
from corrreprref import cells_chain                               # noqa: F401

LD, CLD = np.longdouble, np.clongdouble
U64 = np.uint64
C_ROUND = 10
FAULTS = ("zero_norm_counted", "chi_conjugated", "no_sqrt", "one_orientation_in_self_mirror", "string_middle_not_translated",
          "dd_not_swapped_on_mirror")
KEYS = ("norm2", "pop", "dd", "str", "aa")


# -------------------------------------------------------------------------------------------------------------- basis --
def sector_keys(n, d, total):
    """the packed words of charge `total`, ascending (the generator's order)"""
    b = qf.bits_per_level(d)

    @functools.lru_cache(maxsize=None)
    def rec(s, q):
        if q < 0 or q > s * (d - 1):
            return np.zeros(0, dtype=U64)
        if s == 0:
            return np.zeros(1, dtype=U64)
        return np.concatenate([rec(s - 1, q - l) | U64(l << ((s - 1) * b)) for l in range(min(d - 1, q) + 1)])

    return rec(n, total)


class Sector:
    def __init__(self, n, d, total, perms, chars):
        self.n, self.d, self.total = n, d, total
        self.bits = b = qf.bits_per_level(d)
        self.perms, self.chars = np.asarray(perms, dtype=np.int64), np.asarray(chars, dtype=np.complex128)
        self.G = len(self.perms)
        assert np.array_equal(self.perms[0], np.arange(n))
        per = 12 // b                                                # whole sites in a 12-bit slice of the key
        self.n_slices = (n + per - 1) // per
        vals = np.arange(4096, dtype=U64)
        self.tab = np.zeros((self.G, self.n_slices, 4096), dtype=U64)
        for g in range(self.G):
            for c in range(self.n_slices):
                for k in range(per):
                    s = c * per + k
                    if s < n:
                        self.tab[g, c] |= ((vals >> U64(k * b)) & U64((1 << b) - 1)) << U64(int(self.perms[g][s]) * b)
        keys = sector_keys(n, d, total)
        self.n_words = len(keys)
        best, _, nstab, csum = self._scan(keys, stabiliser=True)
        rep = best == keys
        self.reps = keys[rep]                                        # ascending
        self.dim = len(self.reps)
        self.nstab = nstab[rep]
        self.zero = np.abs(csum[rep]) ** 2 < 1e-20
        assert np.all(np.abs(np.abs(csum[rep]) - np.where(self.zero, 0, self.nstab)) < 1e-9)
        self.levels = None

    def translate(self, keys, g):
        out = np.zeros_like(keys)
        for c in range(self.n_slices):
            out |= self.tab[g, c][((keys >> U64(12 * c)) & U64(4095)).astype(np.int64)]
        return out

    def _scan(self, keys, stabiliser=False):
        best, gstar = keys.copy(), np.zeros(len(keys), dtype=np.int64)
        nstab = np.ones(len(keys), dtype=np.int64) if stabiliser else None
        csum = np.full(len(keys), self.chars[0]) if stabiliser else None
        for g in range(1, self.G):
            img = self.translate(keys, g)
            lt = img < best                                          # the first element that reaches the smallest image
            best[lt], gstar[lt] = img[lt], g
            if stabiliser:
                eq = img == keys
                nstab += eq
                csum[eq] += self.chars[g]
        return best, gstar, nstab, csum

    def canonical(self, keys):
        """(position of the representative, group element that carries the word there)"""
        best, gstar, _, _ = self._scan(keys)
        pos = np.searchsorted(self.reps, best)
        assert np.all(self.reps[pos] == best)
        return pos, gstar

    def rep_levels(self):
        if self.levels is None:
            self.levels = qf.unpack(self.reps, self.n, self.d).astype(np.int64)      # [dim][site]
        return self.levels


@functools.lru_cache(maxsize=None)
def _sector_cached(n, d, total, perms_bytes, chars_bytes, n_trans):
    perms = np.frombuffer(perms_bytes, dtype=np.int32).reshape(n_trans, n)
    return Sector(n, d, total, perms, np.frombuffer(chars_bytes, dtype=np.complex128))


def sector(n, d, total, perms, chars):
    p, c = np.ascontiguousarray(perms, dtype=np.int32), np.ascontiguousarray(chars, dtype=np.complex128)
    return _sector_cached(n, d, total, p.tobytes(), c.tobytes(), len(p))


# ------------------------------------------------------------------------------------------------------------ classes --
def _orbit(start, act, n_g):
    """the images of `start` under the n_g elements: its orbit, the elements being a group (tests/test_quditcorrreprref.py checks
    it against `_closure` on its cases)"""
    return {start} | {act(g, start) for g in range(n_g)}


def _closure(start, act, n_g):
    """everything repeated application of the elements makes of `start`, breadth first"""
    seen, todo = {start}, [start]
    while todo:
        x = todo.pop()
        for g in range(n_g):
            y = act(g, x)
            if y not in seen:
                seen.add(y)
                todo.append(y)
    return seen


def site_orbits(n, perms):
    return [sorted(_orbit(s, lambda g, x: int(perms[g][x]), len(perms))) for s in range(n)]


def pair_classes(n, perms):
    """cls[i][j] -> (forward orbit as a sorted list of ordered pairs, (i, j) is in it, the class is its own mirror); the forward
    orbit of a class is the one that holds the smallest ordered pair of the class"""
    out, done = {}, {}
    for i in range(n):
        for j in range(n):
            if i == j or (i, j) in done:
                continue
            orb = _orbit((i, j), lambda g, x: (int(perms[g][x[0]]), int(perms[g][x[1]])), len(perms))
            mirror = {(q, p) for p, q in orb}
            own = (j, i) in orb
            fwd = sorted(orb) if own or min(orb) < min(mirror) else sorted(mirror)
            for x in orb | mirror:
                done[x] = (fwd, own)
    for (i, j), (fwd, own) in done.items():
        out[(i, j)] = (fwd, (i, j) in fwd, own)
    return out


def string_members(n, perms, i, j, fault=None, orbit=_orbit):
    """the orbit of the decorated string ({i, j}, {k: i < k < j}): a sorted list of (e1, e2, tuple of middle sites)"""
    def act(g, m):
        e = sorted((int(perms[g][m[0]]), int(perms[g][m[1]])))
        if fault == "string_middle_not_translated":
            mid = tuple(range(e[0] + 1, e[1]))                       # the index interval of the image ends
        else:
            mid = tuple(sorted(int(perms[g][k]) for k in m[2]))
        return (e[0], e[1], mid)

    return sorted(orbit((i, j, tuple(range(i + 1, j))), act, len(perms)))


# ---------------------------------------------------------------------------------------------------------- reference --
def qudit_repr(n, d, total, perms, chars, psi, diag=None, string=None, lower=None, fault=None, entries=None):
    """dict(norm2, pop, dd, str, aa, A=dict(the same keys), dim, zero) from the representatives alone, for the tables that are given.
    fault: one of FAULTS, a deliberately wrong variant that the comparison with the explicit route has to reject.  entries: a list of
    site pairs (i, j); only the off-diagonal entries of dd, str and aa whose class one of them names are computed, the others are NaN
    (with A = NaN) and are skipped by `compare` -- for sectors too large to walk every class within seconds."""
    assert fault is None or fault in FAULTS
    S = sector(n, d, total, perms, chars)
    N, b = n, S.bits
    assert len(psi) == S.dim
    p = np.asarray(psi).astype(CLD)
    live = np.ones(S.dim, dtype=bool) if fault == "zero_norm_counted" else ~S.zero
    p = np.where(live, p, CLD(0))                                    # an entry at a zero-norm representative is never used
    rows = np.nonzero(live & (p != 0))[0]                            # a row of amplitude 0 contributes exactly nothing
    w = (np.abs(p[rows]) ** 2).astype(LD)
    L = S.rep_levels()[rows]                                         # [live row][site]
    norm2 = np.sum(w)
    out = {"norm2": norm2, "pop": np.zeros((N, d), dtype=LD), "dim": S.dim, "zero": S.zero}
    A = {"norm2": norm2}
    for s, orb in enumerate(site_orbits(N, S.perms)):
        for l in range(d):
            out["pop"][s, l] = np.sum(w * np.sum(L[:, orb] == l, axis=1)) / LD(len(orb))
    A["pop"] = out["pop"].copy()
    wanted = None if entries is None else {(min(i, j), max(i, j)) for i, j in entries}
    nan = LD(np.nan)
    classes = pair_classes(N, S.perms) if (diag is not None or lower is not None) else None

    def class_wanted(fwd):
        return wanted is None or any((min(x), max(x)) in wanted for x in fwd)

    if diag is not None:
        f = np.asarray(diag, dtype=np.float64).reshape(-1, d).astype(LD)
        K = len(f)
        out["dd"], A["dd"] = np.full((K, K, N, N), nan), np.full((K, K, N, N), nan)
        cache = {}
        for i in range(N):
            for a in range(K):
                for c in range(K):
                    t = out["pop"][i] * f[a] * f[c]
                    out["dd"][a, c, i, i], A["dd"][a, c, i, i] = np.sum(t), np.sum(np.abs(t))
            for j in range(N):
                if i == j:
                    continue
                fwd, is_fwd, _ = classes[(i, j)]
                if not class_wanted(fwd):
                    continue
                key = id(fwd)
                if key not in cache:
                    F, FA = np.zeros((K, K), dtype=LD), np.zeros((K, K), dtype=LD)
                    for (pp, qq) in fwd:
                        for a in range(K):
                            for c in range(K):
                                t = w * f[a][L[:, pp]] * f[c][L[:, qq]]
                                F[a, c] += np.sum(t)
                                FA[a, c] += np.sum(np.abs(t))
                    cache[key] = (F / LD(len(fwd)), FA / LD(len(fwd)))
                F, FA = cache[key]
                swap = not is_fwd and fault != "dd_not_swapped_on_mirror"
                out["dd"][:, :, i, j], A["dd"][:, :, i, j] = (F.T, FA.T) if swap else (F, FA)
    if string is not None:
        h, gm = (np.asarray(t, dtype=np.float64).astype(LD) for t in string)
        out["str"], A["str"] = np.full((N, N), nan), np.full((N, N), nan)
        cache = {}                                                   # seed -> its class's value, None for a class not wanted
        for i in range(N):
            t = out["pop"][i] * h * h
            out["str"][i, i], A["str"][i, i] = np.sum(t), np.sum(np.abs(t))
            for j in range(i + 1, N):
                if (i, j) not in cache:
                    mem = string_members(N, S.perms, i, j, fault)
                    seeds = [(m[0], m[1]) for m in mem if m[2] == tuple(range(m[0] + 1, m[1]))]      # the seeds of this class
                    val = None
                    if wanted is None or any(x in wanted for x in seeds):
                        v, va = LD(0), LD(0)
                        for (e1, e2, mid) in mem:
                            t = w * h[L[:, e1]] * h[L[:, e2]]
                            for k in mid:
                                t = t * gm[L[:, k]]
                            v += np.sum(t)
                            va += np.sum(np.abs(t))
                        val = (v / LD(len(mem)), va / LD(len(mem)))
                    for x in seeds:
                        cache.setdefault(x, val)
                if cache[(i, j)] is not None:
                    out["str"][i, j] = out["str"][j, i] = cache[(i, j)][0]
                    A["str"][i, j] = A["str"][j, i] = cache[(i, j)][1]
    if lower is not None:
        low = np.asarray(lower, dtype=np.float64).astype(LD)
        chi = (np.conj(S.chars) if fault == "chi_conjugated" else S.chars).astype(CLD)
        out["aa"], A["aa"] = np.full((N, N), nan + 0j, dtype=CLD), np.full((N, N), nan)
        keys = S.reps[rows]
        cache = {}
        for i in range(N):
            t = out["pop"][i, :d - 1] * low[1:] * low[1:]
            out["aa"][i, i], A["aa"][i, i] = np.sum(t), np.sum(np.abs(t))
            for j in range(N):
                if i == j:
                    continue
                fwd, is_fwd, own = classes[(i, j)]
                if not class_wanted(fwd):
                    continue
                key = id(fwd)
                if key not in cache:
                    members = [x for x in fwd if x[0] < x[1]] if (own and fault == "one_orientation_in_self_mirror") else fwd
                    T, TA = CLD(0), LD(0)
                    hits, cs, amps = [], [], []                      # all members of the class: one canonicalisation
                    for (pp, qq) in members:
                        hit = np.nonzero((L[:, pp] >= 1) & (L[:, qq] <= d - 2))[0]
                        hits.append(hit)
                        cs.append(keys[hit] - (U64(1) << U64(pp * b)) + (U64(1) << U64(qq * b)))
                        amps.append(low[L[hit, pp]] * low[L[hit, qq] + 1])
                    hit, c, amp = np.concatenate(hits), np.concatenate(cs), np.concatenate(amps)
                    if len(hit):
                        tgt, g = S.canonical(c)
                        ok = live[tgt]
                        ratio = np.ones(len(hit), dtype=LD) if fault == "no_sqrt" else \
                            np.sqrt(S.nstab[tgt].astype(LD) / S.nstab[rows[hit]].astype(LD))
                        term = amp * ratio * chi[g] * np.conj(p[tgt]) * p[rows[hit]]
                        T, TA = np.sum(term[ok]), np.sum(np.abs(term[ok]))
                    n_o = LD(len(members))
                    cache[key] = (CLD(T.real / n_o) if own and fault is None else T / n_o, TA / n_o)
                T, TA = cache[key]
                out["aa"][i, j], A["aa"][i, j] = (T if is_fwd else np.conj(T)), TA
    out["A"] = A
    return out


# ----------------------------------------------------------------------------------------------------- explicit route --
def unfold(n, d, total, perms, chars, psi):
    """the vector of the full sector in generator order: Psi[T_g a] += chi(g) psi_a, every column normalised on its own, the columns
    of zero norm left out"""
    S = sector(n, d, total, perms, chars)
    allk = sector_keys(n, d, total)
    p = np.asarray(psi).astype(CLD)
    M = np.zeros((len(allk), S.dim), dtype=CLD)
    cols = np.arange(S.dim)
    for g in range(S.G):
        idx = np.searchsorted(allk, S.translate(S.reps, g))
        np.add.at(M, (idx, cols), CLD(S.chars[g]))
    nrm = np.sqrt(np.sum(np.abs(M) ** 2, axis=0))
    alive = nrm > 1e-9
    assert np.array_equal(alive, ~S.zero)
    return M[:, alive] @ (p[alive] / nrm[alive])


def explicit(n, d, total, perms, chars, psi, diag=None, string=None, lower=None):
    """quditcorrref.correlations on the unfolded state (clongdouble all the way)"""
    return quditcorrref.correlations(n, d, total, unfold(n, d, total, perms, chars, psi), diag=diag, string=string, lower=lower)


# --------------------------------------------------------------------------------------------------------- comparison --
def tolerance(ref, n_trans, n_sites, key):
    return (ref["dim"] * n_trans + n_sites + C_ROUND) * 2.0 ** -53 * np.asarray(ref["A"][key]).astype(np.float64)


def compare(label, got, ref, n_trans, n_sites, keys=None):
    """every computed entry of every array within `tolerance` (an entry with A = 0 must vanish exactly); prints the worst ratio per
    array and returns them"""
    keys = [k for k in KEYS if k in ref] if keys is None else keys
    worst = {}
    for k in keys:
        w = np.asarray(ref[k])
        g = np.asarray(got[k]).reshape(w.shape)
        tol = np.asarray(tolerance(ref, n_trans, n_sites, k))
        there = ~np.isnan(tol)
        assert np.all(np.isfinite(g[there])), (label, k, "not finite")
        err = np.abs(g.astype(w.dtype) - w).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))      # exact zeros stay exact
        worst[k] = float(np.max(ratio[there])) if there.any() else 0.0
    print("%s dim %d |G| %d: worst |got - want| / bound  %s" % (label, ref["dim"], n_trans, "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k in keys:
        assert worst[k] <= 1.0, (label, k, worst[k])
    return worst
