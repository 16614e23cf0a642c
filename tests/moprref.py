"""Host reference of the full-space operator-times-vector step (qbh_mopr_spin_dev, qbh_mopr_onebody_dev, qbh_mopr_terms_dev,
qbh_mopr_qudit_dev) and the comparison the GPU tests share.  Plain numpy, no import of the library.

Independent in direction: the kernels gather per TARGET row by running adjoint factors and find the source through a colex rank
formula or a counting table; here every SOURCE state is scattered forward, the factors applied right to left to its word, and
the target index is np.searchsorted on the ascending list of the target sector's words.  Sectors are enumerated here from
integers only (words(): tuples of levels with a given sum, bit patterns being the case d = 2).  Indices are exact integers
(uint64), values are accumulated in longdouble / clongdouble.  Everything is vectorised over the states: one fancy-indexed
update per term or site, so a sector of 7e5 rows takes about a second.

Every function returns (want, scale, k):  want[i] the target vector,  scale[i] = sum |coef_t| |amplitude_t| |x_j| and k[i] the
number of terms, over the terms that reach row i with a nonzero amplitude.  compare() holds a device result against them:
|got_i - want_i| <= 4 (k_i + 4) 2^-53 scale_i for every row, which for k_i = 0 means exactly zero."""
import collections
import functools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U64 = np.uint64
SENTINEL = -7.5e300


# ------------------------------------------------------------------------------------------------ enumeration --
def _words_up(n_sites, d, total):
    """DP over the sites: layer[q] = the ascending keys sum_s l_s d^s on the sites done so far that carry charge q"""
    layer = {0: np.zeros(1, dtype=U64)}
    for s in range(n_sites):
        q_min = max(0, total - (n_sites - s - 1) * (d - 1))            # the sites above s cannot supply more than this
        nxt = {}
        for q in range(q_min, total + 1):
            parts = [layer[q - l] + U64(l * d ** s) for l in range(min(d - 1, q) + 1) if (q - l) in layer]
            if parts:
                nxt[q] = np.concatenate(parts)                             # ascending: the level of site s dominates
        layer = nxt
    return layer.get(total, np.zeros(0, dtype=U64))


@functools.lru_cache(maxsize=64)
def words(n_sites, d, total):
    """Every tuple of levels (l_0 .. l_{n-1}), 0 <= l_s < d, with sum total, as the key sum_s l_s d^s (uint64), ascending.
    Beyond half filling the complement l_s -> d - 1 - l_s is enumerated and mirrored."""
    top = n_sites * (d - 1)
    if total < 0 or total > top:
        return np.zeros(0, dtype=U64)
    if 2 * total > top:
        w = U64(d ** n_sites - 1) - _words_up(n_sites, d, top - total)[::-1]
    else:
        w = _words_up(n_sites, d, total)
    w = np.ascontiguousarray(w)
    w.setflags(write=False)
    return w


def count(n_sites, d, total):
    """len(words(n_sites, d, total)) without listing them"""
    cnt = [1] + [0] * max(total, 0)
    for _ in range(n_sites):
        cnt = [sum(cnt[q - l] for l in range(min(d - 1, q) + 1)) for q in range(len(cnt))]
    return cnt[total] if 0 <= total <= n_sites * (d - 1) else 0


def patterns(n_sites, n_set):
    """bit patterns of n_sites bits with n_set bits set, ascending (uint64)"""
    return words(n_sites, 2, n_set)


def _lookup(sorted_words, w):
    idx = np.searchsorted(sorted_words, w)
    assert idx.size == 0 or (idx.max() < len(sorted_words) and np.array_equal(sorted_words[idx], w)), "a word outside the target sector"
    return idx


# ------------------------------------------------------------------------------------------------ accumulation --
def _accumulate(contribs, dim_new, x, dtype=CLD):
    """contribs yields (rows, cols, weight) per term: weight[m] x[cols[m]] goes to rows[m]; a term maps distinct sources to
    distinct targets, so rows holds no index twice and the fancy-indexed update is a plain sum in the order of the terms."""
    real = LD if dtype == CLD else np.float64
    want, scale, k = np.zeros(dim_new, dtype=dtype), np.zeros(dim_new, dtype=real), np.zeros(dim_new, dtype=np.int64)
    xs = np.asarray(x).astype(dtype)
    for rows, cols, weight in contribs:
        weight = np.asarray(weight).astype(dtype)
        want[rows] += weight * xs[cols]
        scale[rows] += np.abs(weight) * np.abs(xs[cols])
        k[rows] += 1
    return want, scale, k


# ------------------------------------------------------------------------------------------------------- spin --
def spin_contribs(n_sites, n_dn_old, kind, coef):
    """S^z_q (kind 0), S^-_q (kind -1: adds a down spin), S^+_q (kind +1): one term per site.  Bit = 1 means down."""
    old, new = patterns(n_sites, n_dn_old), patterns(n_sites, n_dn_old - kind)
    src = np.arange(len(old), dtype=np.int64)
    same = _lookup(new, old) if kind == 0 else None
    for s in range(n_sites):
        bit = U64(1 << s)
        down = (old & bit) != 0
        c = CLD(complex(coef[s]))
        if kind == 0:
            yield same, src, c * np.where(down, LD(-0.5), LD(0.5))
        else:
            sel = ~down if kind < 0 else down
            yield _lookup(new, old[sel] ^ bit), src[sel], np.full(int(sel.sum()), c, dtype=CLD)


def spin(n_sites, n_dn_old, kind, coef, x, dtype=CLD):
    dim_new = len(patterns(n_sites, n_dn_old - kind))
    return _accumulate(spin_contribs(n_sites, n_dn_old, kind, coef), dim_new, x, dtype)


# ------------------------------------------------------------------------------------- ordered products of factors --
# factor = (kind, site, species).  family 0 (spin-1/2): kind 0 S^z, 1 S^+ (down -> up), 2 S^- (up -> down), species ignored.
# family 1 (two-species fermions, Jordan-Wigner on the word u | d << n_sites): kind 0 n, 1 c^dag, 2 c;
# c^dag_o |w> = (-1)^{occupied orbitals below o} |w + o>, o = site + species * n_sites.
def _sector_change(family, factors):
    da = db = 0
    for kind, _, sp in factors:
        delta = 0 if kind == 0 else (-1 if kind == 1 else 1) if family == 0 else (1 if kind == 1 else -1)
        if family == 1 and sp:
            db += delta
        else:
            da += delta
    return da, db


def _sector_words(family, n_sites, n_a, n_b):
    """(words in index order, their ascending sort keys).  family 1: index = rank(up) * C(n, n_dn) + rank(down), so the key that
    ascends with the index is up << n | down while the word the factors act on is up | down << n."""
    if family == 0:
        w = patterns(n_sites, n_a)
        return w, w
    up, dn = patterns(n_sites, n_a), patterns(n_sites, n_b)
    sh = U64(n_sites)
    return (up[:, None] | (dn[None, :] << sh)).ravel(), ((up[:, None] << sh) | dn[None, :]).ravel()


def terms_contribs(family, n_sites, n_a_old, n_b_old, terms):
    """terms = [(coef, [factor, ...]), ...]; the factors of a product act right to left on the source word"""
    da, db = _sector_change(family, terms[0][1])
    W, _ = _sector_words(family, n_sites, n_a_old, n_b_old)
    _, new_keys = _sector_words(family, n_sites, n_a_old + da, n_b_old + db)
    src = np.arange(len(W), dtype=np.int64)
    for coef, factors in terms:
        assert _sector_change(family, factors) == (da, db), "one target sector only"
        w, amp, alive = W.copy(), np.ones(len(W), dtype=LD), np.ones(len(W), dtype=bool)
        for kind, site, sp in reversed(factors):
            bit = U64(1 << (site + (sp * n_sites if family == 1 else 0)))
            occ = (w & bit) != 0
            if family == 0:
                if kind == 0:
                    amp = amp * np.where(occ, LD(-0.5), LD(0.5))
                else:
                    alive &= occ if kind == 1 else ~occ                       # S^+ needs a down spin, S^- an up spin
                    w = w ^ bit
            elif kind == 0:
                alive &= occ
            else:
                alive &= ~occ if kind == 1 else occ
                below = np.bitwise_count(w & (bit - U64(1)))
                amp = np.where(below & 1, -amp, amp)
                w = w ^ bit
        w, amp, cols = w[alive], amp[alive], src[alive]
        if family == 1:
            sh = U64(n_sites)
            w = ((w & ((U64(1) << sh) - U64(1))) << sh) | (w >> sh)
        yield _lookup(new_keys, w), cols, CLD(complex(coef)) * amp


def terms(family, n_sites, n_a_old, n_b_old, terms, x, dtype=CLD):
    da, db = _sector_change(family, terms[0][1])
    dim_new = len(_sector_words(family, n_sites, n_a_old + da, n_b_old + db)[1])
    return _accumulate(terms_contribs(family, n_sites, n_a_old, n_b_old, terms), dim_new, x, dtype)


def onebody_as_products(terms):
    """[(a, b, spin, w)] -> w c^dag_{a,spin} c_{b,spin} as ordered products; a == b is the density"""
    return [(w, [(1, a, sp), (2, b, sp)]) for a, b, sp, w in terms]


def onebody_contribs(n_sites, n_up, n_dn, terms):
    return terms_contribs(1, n_sites, n_up, n_dn, onebody_as_products(terms))


def onebody(n_sites, n_up, n_dn, terms, x, dtype=CLD):
    dim = len(patterns(n_sites, n_up)) * len(patterns(n_sites, n_dn))
    return _accumulate(onebody_contribs(n_sites, n_up, n_dn, terms), dim, x, dtype)


# ------------------------------------------------------------------------------------------------------ qudit --
def qudit_contribs(n_sites, d, total_old, dq, coef, local):
    """sum_s coef[s] O_s with local[l' d + l] = <l'|O|l>, nonzero only where l' = l + dq; words ranked by sum_s l_s d^s"""
    old, new = words(n_sites, d, total_old), words(n_sites, d, total_old + dq)
    loc = np.asarray(local, dtype=np.complex128).reshape(d, d)
    src = np.arange(len(old), dtype=np.int64)
    for s in range(n_sites):
        unit = d ** s
        lev = ((old // U64(unit)) % U64(d)).astype(np.int64)
        to = lev + dq
        ok = (to >= 0) & (to < d)
        a = np.zeros(len(old), dtype=np.complex128)
        a[ok] = loc[to[ok], lev[ok]]
        sel = ok & (a != 0)
        w = old[sel] + U64(dq * unit) if dq >= 0 else old[sel] - U64(-dq * unit)
        yield _lookup(new, w), src[sel], CLD(complex(coef[s])) * a[sel].astype(CLD)


def qudit(n_sites, d, total_old, dq, coef, local, x, dtype=CLD):
    dim_new = len(words(n_sites, d, total_old + dq))
    return _accumulate(qudit_contribs(n_sites, d, total_old, dq, coef, local), dim_new, x, dtype)


# ------------------------------------------------------------------------------------------------- comparison --
Verdict = collections.namedtuple("Verdict", "ok worst bad")


def bound(scale, k):
    """4 (k_i + 4) 2^-53 scale_i: at most k_i accumulated terms, each at most two nested complex products (sqrt(5) u each,
    at most 4 roundings), accumulated in the order of a plain sum"""
    return LD(4.0) * (np.asarray(k).astype(LD) + LD(4.0)) * LD(2.0) ** -53 * np.asarray(scale).astype(LD)


def compare(got, want, scale, k):
    """Every row of got against want: |got_i - want_i| <= bound_i, where bound_i = 0 (k_i = 0) asks for exactly 0.0 in both
    parts.  NaN, infinities and sentinels fail.  Returns Verdict(ok, worst ratio |got - want| / bound, failing rows)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return Verdict(False, float("inf"), np.arange(len(want)))
    # longdouble work only on the rows some term reaches; the others (most rows of a sparse operator) must be exactly zero
    pos = np.flatnonzero(np.asarray(scale) > 0)
    b = bound(np.asarray(scale)[pos], np.asarray(k)[pos])
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.abs(got[pos].astype(CLD) - want[pos].astype(CLD)) / b
    ratio = np.where(np.isnan(ratio), np.inf, ratio)                   # NaN fails
    nonzero = (got.real != 0) | (got.imag != 0)                        # true for NaN as well
    nonzero[pos] = False
    bad = np.union1d(pos[~(ratio <= 1)], np.flatnonzero(nonzero))
    worst = float("inf") if nonzero.any() else float(ratio.max()) if len(ratio) else 0.0
    return Verdict(len(bad) == 0, worst, bad)
