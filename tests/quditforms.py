"""Host-only reference, comparator, bounds, mirror and case table for the d-level family of qbh_qudit.hip: the generator
(qbh_gen_qudit: k_qudit_count, k_qudit_fill) and the operator applied without a stored matrix (qbh_mf_qudit: k_mf_qudit<REALX, TLDS>,
k_mf_qudit_count).  Plain numpy and Python integers, no library code.  Shared by tests/test_quditforms.py (CPU) and
tests/test_gpu_quditforms.py.

Basis (include/qbhip.h): site s holds a level l_s in [0, d); the words of one charge sum_s l_s are ranked in ascending order of
sum_s l_s d^s, which is the order of the packed words (b = 1, 2 or 3 bits per site, site s in bits [s b, (s + 1) b)) as UNSIGNED
64-bit integers: 4^32 - 1 and 2^64 - 1 occur, so keys are numpy uint64 throughout and are never compared as int64.

* `words`: the sector enumerated recursively (most significant site first, levels ascending: already in order);
* `Counter.rank / unrank`: by counting the words below, most significant site first, in Python integers, from
  N(s, q) = number of words on s sites with charge q; `rank_many` is the same count vectorised in uint64 (pinned against `rank`);
* `assemble`: the expected CSR of rows [r0, r1) (default: all) and, per row, the unmerged terms behind it (count and sum of moduli);
* `mf_layout`: a mirror of the host code of qbh_mf_qudit (classes, slots, LDS bytes, table placement, bytes held, longest row);
* the comparator (`assert_same_csr`, on genforms.assert_same_csr) and the row bound (`reference`, on csrforms.row_sums and
  csrforms.epilogue through kronforms.epilogue);
* the case table, each case with the edge it exists for (tests/test_quditforms.py asserts every edge on the reference alone).

Bounds.  A stored off-diagonal value is one element of a merged pair matrix; repeated pairs are merged by one complex addition
each, in the given order, here as in the library: IEEE addition is deterministic, so these values are expected bit for bit.  The
diagonal of a row is the sum of n_sites single-site terms and one term per merged pair, added in double in some order:
|got - ref| <= (n_sites + n_pairs + 2) eps sum |terms| covers the n_sites + n_pairs - 1 additions (eps / 2 each, first order, on
a partial sum bounded by sum |terms|) and the rounding of the long-double reference with room to spare.

An applied row is a sum over its unmerged terms: the n_sites + n_pairs diagonal terms and one term per off-diagonal entry (one
slot of the kernel each); terms_i counts them.  Roundings per component (u = eps / 2): the diagonal sum (n_sites + n_pairs - 1
additions), its product with x_i (1), a complex product per slot (2), one addition per slot, the diagonal joined to the slots'
sum (1), alpha (1, 2 where complex), the two additions of the epilogue (2): at most terms_i + 7 on every term.  The modulus errs
by sqrt(2) times a component, and sqrt(2) * 1.01 * (k + 8) u < 0.72 (k + 8) eps, so, as tests/secforms.py has it,

    |y_i - ref_i| <= (terms_i + 4 + EXTRA) eps S_i,   S_i = |alpha| sum_unmerged |a||x_j| + |beta||y_i| + |gamma||x_i|,   EXTRA = 4.

The reductions take csrforms.epilogue's t_dot / t_nrm with this row bound.  Probe vectors have |x_j| >= 0.5 (complex,
csrforms.probe_vector) or >= 0.25 before normalisation (real, kronsum.probe_vector), and every off-diagonal amplitude of every case
has |a| >= 0.1: a dropped, doubled, mis-signed or misplaced term is orders of magnitude outside its row's bound.
"""
from functools import lru_cache
from math import comb
from types import SimpleNamespace

import numpy as np

import csrforms as cf
import genforms as gf
import kronforms as kf
from csrforms import CL, EPS, L, probe_vector, worst      # noqa: F401  (re-exported for the tests)

EXTRA = 4
MAX_ROW = 240                # kQuditMaxRow: entries of one row of the stored form, counted from the merged terms
FILL_BLOCK = 64              # kQuditFillBlock: rows one workgroup of k_qudit_fill sorts in LDS
MF_BLOCK = 512               # kMfQuditBlock
LDS_CAP = 150 * 1024         # kMfQuditLdsCap: the class tables go to LDS when everything fits below it
LDS_DEVICE = 160 * 1024      # LDS of one CU
GRID_ROWS = 256 * 4 * MF_BLOCK     # rows of one resident grid of k_mf_qudit (256 CUs x at most 4 workgroups)
U64 = np.uint64


def bits_per_level(d):
    return 1 if d <= 2 else 2 if d <= 4 else 3


# ------------------------------------------------------------------------------------------------------------- basis --
def pack(levels, d):
    """levels [..., n] -> packed words, uint64"""
    lv = np.asarray(levels)
    b = bits_per_level(d)
    w = np.zeros(lv.shape[:-1], dtype=U64)
    for s in range(lv.shape[-1]):
        w |= lv[..., s].astype(U64) << U64(s * b)
    return w


def unpack(keys, n, d, bits=None):
    """packed words -> levels [len, n] (uint8).  `bits`: read with another field width (what a wrong-width kernel would see)."""
    b = bits_per_level(d) if bits is None else bits
    k = np.asarray(keys, dtype=U64)
    out = np.zeros(k.shape + (n,), dtype=np.uint8)
    for s in range(n):
        if s * b < 64:
            out[..., s] = ((k >> U64(s * b)) & U64((1 << b) - 1)).astype(np.uint8)
    return out


def words(n, d, total):
    """The sector in generator order: (levels [dim, n] uint8, packed keys [dim] uint64, strictly ascending as unsigned)."""
    @lru_cache(maxsize=None)
    def rec(s, q):                                   # words on sites 0 .. s-1 with charge q, ascending
        if q < 0 or q > s * (d - 1):
            return np.zeros((0, s), dtype=np.uint8)
        if s == 0:
            return np.zeros((1, 0), dtype=np.uint8)
        parts = []
        for l in range(0, min(d - 1, q) + 1):        # level of the most significant site, ascending
            low = rec(s - 1, q - l)
            if len(low):
                parts.append(np.concatenate([low, np.full((len(low), 1), l, dtype=np.uint8)], axis=1))
        return np.concatenate(parts) if parts else np.zeros((0, s), dtype=np.uint8)

    lv = rec(n, total)
    keys = pack(lv, d)
    assert keys.dtype == U64 and (len(keys) < 2 or bool(np.all(keys[1:] > keys[:-1])))
    return lv, keys


class Counter:
    """rank / unrank of one sector from N(s, q) = number of words on s sites with charge q (Python integers)."""

    def __init__(self, n, d, total):
        self.n, self.d, self.total = n, d, total
        N = [[1] + [0] * total]
        for s in range(n):
            N.append([sum(N[s][q - l] for l in range(min(d - 1, q) + 1)) for q in range(total + 1)])
        self.N = N
        self.dim = N[n][total]

    def rank(self, levels):
        """The number of words of the sector below this one: they agree with it above some site s and hold a smaller level there."""
        r, Q = 0, int(sum(int(l) for l in levels))
        assert Q == self.total
        for s in range(self.n - 1, -1, -1):
            for l in range(int(levels[s])):
                if Q - l >= 0:
                    r += self.N[s][Q - l]
            Q -= int(levels[s])
        return r

    def unrank(self, r):
        assert 0 <= r < self.dim
        w, Q = [0] * self.n, self.total
        for s in range(self.n - 1, -1, -1):
            for l in range(min(self.d - 1, Q) + 1):
                c = self.N[s][Q - l]
                if r < c:
                    break
                r -= c
            w[s] = l
            Q -= l
        assert r == 0 and Q == 0
        return w

    def rank_many(self, levels):
        """`rank` for levels [m, n], in uint64 (every count of a sector below 2^64 fits)."""
        assert self.dim < 1 << 64
        lv = np.asarray(levels).astype(np.int64)
        tab = np.array([[v if v < 1 << 64 else 0 for v in row] for row in self.N], dtype=U64)      # counts above dim are never added
        r = np.zeros(len(lv), dtype=U64)
        Q = lv.sum(axis=1)
        assert np.all(Q == self.total)
        for s in range(self.n - 1, -1, -1):
            for l in range(self.d - 1):
                take = (lv[:, s] > l) & (Q - l >= 0)
                r[take] += tab[s][(Q - l)[take]]
            Q = Q - lv[:, s]
        return r


# --------------------------------------------------------------------------------------------------------- operators --
def swap_index(d):
    return np.array([(r % d) * d + r // d for r in range(d * d)])


def merge_pairs(d, pairs):
    """[(i, j, M)] -> sorted [((lo, hi), merged matrix)]: a pair given as (j, i) is transposed, [(a' b'), (a b)] -> [(b' a'), (b a)];
    repeats are added in the given order (one complex addition each)."""
    sw = swap_index(d)
    acc = {}
    for (i, j, M) in pairs:
        M = np.asarray(M, dtype=np.complex128).reshape(d * d, d * d)
        if i > j:
            M = M[np.ix_(sw, sw)]
        key = (min(i, j), max(i, j))
        acc[key] = acc[key] + M if key in acc else np.zeros((d * d, d * d), dtype=np.complex128) + M
    return sorted(acc.items())


def merge_singles(n, d, singles):
    sd = np.zeros((n, d))
    for (s, dg) in singles:
        sd[s] += np.asarray(dg, dtype=np.float64)
    return sd


def _offdiag(M):
    """nonzero off-diagonal elements [(in, out, value)] of a merged matrix, row by row, columns ascending"""
    return [(r, c, M[r, c]) for r in range(M.shape[0]) for c in range(M.shape[1]) if r != c and (M[r, c].real != 0.0 or M[r, c].imag != 0.0)]


def assemble(n, d, total, pairs, singles, rows=None, keep_terms=True):
    """The expected CSR of rows [r0, r1) of the sector.  -> namespace:
    dim (of the sector), r0, nrows, keys (uint64 words of the rows), levels
    ia, ja (int64, global columns, ascending), val (complex128; off-diagonal values are elements of the merged matrices, unrounded)
    is_diag (per entry), diag (long double, per row; val holds it rounded), diag_abs (sum of the moduli of the row's diagonal terms)
    terms (per row: n + n_pairs + off-diagonal entries), off_abs-free: S_i comes from `reference`
    t_ia, t_ja, t_val (keep_terms): the unmerged terms as a CSR with repeated columns, every diagonal term on its own."""
    merged = merge_pairs(d, pairs)
    sd = merge_singles(n, d, singles)
    cnt = Counter(n, d, total)
    dim = cnt.dim
    if rows is None and dim <= 4_000_000:
        lv, keys = words(n, d, total)
        r0, r1 = 0, dim
        col_of = lambda t_lv: np.searchsorted(keys, pack(t_lv, d)).astype(np.int64)              # noqa: E731  (unsigned search)
    else:
        r0, r1 = (0, dim) if rows is None else rows
        lv = np.array([cnt.unrank(r) for r in range(r0, r1)], dtype=np.uint8).reshape(r1 - r0, n)
        keys = pack(lv, d)
        col_of = lambda t_lv: cnt.rank_many(t_lv).astype(np.int64)                                # noqa: E731
    m = len(lv)
    lvi = lv.astype(np.int64)
    diag, diag_abs, dterms = np.zeros(m, dtype=L), np.zeros(m, dtype=L), []

    def add_diag(t):
        nonlocal diag, diag_abs
        diag, diag_abs = diag + t.astype(L), diag_abs + np.abs(t).astype(L)
        if keep_terms:
            dterms.append(t)

    for s in range(n):
        add_diag(sd[s][lvi[:, s]])
    e_row, e_col, e_val = [], [], []
    for (i, j), M in merged:
        lin = lvi[:, i] * d + lvi[:, j]
        add_diag(M.real[lin, lin])
        off = _offdiag(M)
        for r_in in sorted({o[0] for o in off}):
            idx = np.nonzero(lin == r_in)[0]
            if not len(idx):
                continue
            for (_, c_out, z) in (o for o in off if o[0] == r_in):
                t = lv[idx].copy()
                t[:, i], t[:, j] = c_out // d, c_out % d
                e_row.append(idx)
                e_col.append(col_of(t))
                e_val.append(np.full(len(idx), z, dtype=np.complex128))
    me = np.arange(m, dtype=np.int64)
    row = np.concatenate(e_row + [me]) if m else np.zeros(0, dtype=np.int64)
    col = np.concatenate(e_col + [me + r0])
    val = np.concatenate(e_val + [diag.astype(np.float64).astype(np.complex128)])
    isd = np.concatenate([np.zeros(len(row) - m, dtype=bool), np.ones(m, dtype=bool)])
    o = np.lexsort((col, row))
    row, col, val, isd = row[o], col[o], val[o], isd[o]
    assert np.all((row[1:] != row[:-1]) | (col[1:] > col[:-1])), "two terms of a row reach one column"
    ia = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=m), out=ia[1:])
    out = SimpleNamespace(n=n, d=d, total=total, dim=dim, r0=r0, nrows=m, keys=keys, levels=lv, ia=ia, ja=col, val=val,
                          is_diag=isd, diag=diag, diag_abs=diag_abs, n_pairs=len(merged), terms=np.diff(ia) - 1 + n + len(merged),
                          merged=merged, sdiag=sd)
    if keep_terms:
        dt = np.stack(dterms, axis=1)
        nd = dt.shape[1]
        t_row = np.concatenate([row[~isd], np.repeat(me, nd)])
        t_col = np.concatenate([col[~isd], np.repeat(me + r0, nd)])
        t_val = np.concatenate([val[~isd].astype(CL), dt.reshape(-1).astype(CL)])
        o = np.argsort(t_row, kind="stable")
        out.t_ja, out.t_val = t_col[o], t_val[o]
        out.t_ia = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(np.bincount(t_row, minlength=m), out=out.t_ia[1:])
        assert np.array_equal(np.diff(out.t_ia), out.terms)
    return out


def val_ld(asm):
    """the values in long double: the off-diagonal ones as they are, the diagonal unrounded"""
    v = asm.val.astype(CL)
    v[asm.is_diag] = asm.diag
    return v


def diag_tol(asm):
    """per row: (n + n_pairs + 2) eps sum |diagonal terms|"""
    return (asm.n + asm.n_pairs + 2) * L(EPS) * asm.diag_abs


def assert_same_csr(got, asm):
    """got = (ia, ja, val) as downloaded (local row pointers, global columns).  Pointers and columns exactly, off-diagonal values by
    bits, the diagonal within diag_tol.  -> largest diagonal error / bound."""
    rows = np.repeat(np.arange(asm.nrows), np.diff(asm.ia))
    tol = np.where(asm.is_diag, diag_tol(asm)[rows], L(0))
    gia, gja, gval = got
    gf.assert_same_csr((gia, np.asarray(gja, dtype=np.int64), np.asarray(gval)), (asm.ia, asm.ja, val_ld(asm)), exact=False, tol=tol)
    off = ~asm.is_diag
    a = np.ascontiguousarray(np.asarray(gval)[off]).view(np.uint64)
    b = np.ascontiguousarray(asm.val[off]).view(np.uint64)
    bad = np.flatnonzero(a != b)
    assert len(bad) == 0, "off-diagonal value differs in its bits at entry %d of the off-diagonal list" % (bad[0] // 2)
    dg = np.abs(np.asarray(gval)[asm.is_diag].astype(CL) - asm.diag)
    assert not np.any(np.asarray(gval)[asm.is_diag].imag), "a diagonal with an imaginary part"
    bound = np.maximum(diag_tol(asm), L(np.finfo(np.float64).tiny))
    return float(np.max(dg / bound)) if len(dg) else 0.0


# --------------------------------------------------------------------------------------------------------- row bounds --
def compact_columns(asm):
    """(columns the rows touch, ascending; ja renumbered into them; the position of every row's own index among them)"""
    need = np.union1d(asm.ja, np.arange(asm.r0, asm.r0 + asm.nrows, dtype=np.int64))
    return need, np.searchsorted(need, asm.ja), np.searchsorted(need, np.arange(asm.r0, asm.r0 + asm.nrows, dtype=np.int64))


def row_sums(asm, xc, jc=None):
    """(sum_j a_ij x_j with the long-double diagonal, sum over the UNMERGED terms of |a||x_j|) per row, through csrforms.row_sums
    on the merged CSR: the rounding of the stored diagonal is put back, and |diagonal||x_i| is replaced by sum |terms| |x_i|.
    xc: x at the columns `jc` numbers (default: asm.ja numbers the whole vector)."""
    jc = asm.ja if jc is None else jc
    s, a = cf.row_sums(asm.ia, jc, asm.val, xc)
    own = jc[asm.is_diag]
    rounded = asm.val[asm.is_diag].real.astype(L)
    s = s + (asm.diag - rounded) * xc[own].astype(CL)
    a = a + (asm.diag_abs - np.abs(rounded)) * np.abs(xc[own]).astype(L)
    return s, a


def reference(asm, sums, x_own, y0, alpha, beta, gamma):
    """y, bound, dot, nrm, t_dot, t_nrm of csrforms.epilogue with the constant 4 + EXTRA over the unmerged term count."""
    return kf.epilogue(sums[0], sums[1], asm.terms, x_own, y0, alpha, beta, gamma, extra=EXTRA)


def name_row(asm, i):
    return "row %d (global %d), word 0x%016x = levels %s, %d terms" % (
        i, asm.r0 + i, int(asm.keys[i]), "".join(str(int(l)) for l in asm.levels[i]), int(asm.terms[i]))


# ------------------------------------------------------------------------------------------------------------- mirror --
def mf_layout(n, d, total, pairs, singles):
    """What the host code of qbh_mf_qudit builds: classes = distinct merged matrices by bit pattern, in pair order; maxk = the most
    off-diagonal nonzeros in one row of the class; one zero block of d^2 entries, then maxk blocks per class; max(1, maxk) slots per
    pair, padded to a multiple of 8."""
    merged = merge_pairs(d, pairs)
    sd = merge_singles(n, d, singles)
    d2n, tw = d * d, total + 1
    cls_of, cls, maxk, nrow = {}, [], [], []
    for _, M in merged:
        key = np.ascontiguousarray(M).tobytes()
        if key not in cls_of:
            cls_of[key] = len(maxk)
            k = np.zeros(d2n, dtype=np.int64)
            for (r, c, z) in _offdiag(M):
                k[r] += 1
            nrow.append(k)
            maxk.append(int(k.max()))
        cls.append(cls_of[key])
    n_cls = len(maxk)
    n_ent = d2n + sum(maxk) * d2n
    raw_slots = sum(max(1, maxk[c]) for c in cls)
    n_slots = -(-raw_slots // 8) * 8
    values_real = all(not np.any(M.imag[~np.eye(d2n, dtype=bool)]) for _, M in merged)

    def lds_bytes(tables):
        b = (n * tw + n * d) * 8 + n_slots * 8
        return b + (n_ent * 20 + n_cls * d2n * 8 if tables else 0)

    bytes_matrix = n * tw * 8 + len(merged) * 4 + n_cls * d2n * 4 + 2 * n_slots * 4 + n * d * 8 + n_cls * d2n * 8 + n_ent * 4 + n_ent * 16
    return SimpleNamespace(n_pairs=len(merged), cls=cls, n_cls=n_cls, maxk=maxk, nrow=nrow, n_ent=n_ent, raw_slots=raw_slots, n_slots=n_slots,
                           padding=n_slots - raw_slots, has_single=int(np.any(sd != 0.0)), values_real=values_real, lds_bytes=lds_bytes,
                           tables_lds=int(lds_bytes(True) <= LDS_CAP), bytes_matrix=bytes_matrix,
                           max_row=1 + sum(maxk[c] for c in cls), lds_per_class=[mk * d2n * 20 + d2n * 8 for mk in maxk])


def gen_fill_lds(max_row, n, tw):
    """dynamic LDS of k_qudit_fill: the counting table and 64 columns of max_row (column, entry) pairs"""
    return n * tw * 8 + FILL_BLOCK * max_row * 8


def count_rows(n, d, total, pairs, r0, r1):
    """nnz of rows [r0, r1) from `unrank` and the classes' row lengths alone (what k_mf_qudit_count sums)."""
    lay = mf_layout(n, d, total, pairs, [])
    sites = [ij for ij, _ in merge_pairs(d, pairs)]
    cnt = Counter(n, d, total)
    out = 0
    for r in range(r0, r1):
        w = cnt.unrank(r)
        out += 1 + sum(int(lay.nrow[c][w[i] * d + w[j]]) for (i, j), c in zip(sites, lay.cls))
    return out


# --------------------------------------------------------------------------------------------------------- case table --
def draw_pair(rng, d, real=False, p_zero=0.0, diagonal_only=False):
    """A Hermitian d^2 x d^2 matrix that conserves l_i + l_j: off-diagonal moduli in [0.1, 1], each exactly zero with p_zero."""
    M = np.zeros((d * d, d * d), dtype=np.complex128)
    for r in range(d * d):
        M[r, r] = rng.uniform(-1.0, 1.0)
        for c in range(r + 1, d * d):
            if diagonal_only or r // d + r % d != c // d + c % d or rng.random() < p_zero:
                continue
            z = rng.uniform(0.1, 1.0) * (rng.choice([-1.0, 1.0]) if real else np.exp(2j * np.pi * rng.random()))
            M[r, c], M[c, r] = z, np.conj(z)
    return M


def draw_operator(seed, n, d, sites, real=False, p_zero=0.0, singles=True, flip=True):
    """One matrix of its own per site pair; about half the pairs are handed over as (j, i) (the matrix then drawn for that order)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for (i, j) in sites:
        if flip and rng.random() < 0.5:
            i, j = j, i
        pairs.append((i, j, draw_pair(rng, d, real, p_zero)))
    sg = [(s, rng.uniform(-1.0, 1.0, d)) for s in range(n) if rng.random() < 0.7] if singles else []
    return pairs, sg


def _spread(n, k, seed):
    """k distinct site pairs of n sites: (0, n-1) and (0, 1) always, the rest drawn"""
    rng = np.random.default_rng(seed)
    rest = [(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) not in ((0, n - 1), (0, 1), (n - 2, n - 1))]
    pick = rng.choice(len(rest), size=k - 3, replace=False)
    return [(0, n - 1), (0, 1), (n - 2, n - 1)] + [rest[p] for p in sorted(pick)]


def _even_odd(k, seed):
    rng = np.random.default_rng(seed)
    allp = [(i, j) if i < j else (j, i) for i in range(0, 32, 2) for j in range(1, 32, 2)]
    return [allp[p] for p in sorted(rng.choice(len(allp), size=k, replace=False))]


ALTERNATING = [s & 1 for s in range(32)]          # levels 0101...: every even-odd pair can move


def _alt_rows():
    r = Counter(32, 2, 16).rank(ALTERNATING)
    return r - 2048, r + 2048


# name -> dict(n, d, total, op = (seed, sites, real, p_zero, singles), edge, dim); optional rows, gen (False: too large to store
# and download in a test), epilogues (how many of the five triples), drivers (True: also the three real drivers)
def _case(d, n, total, dim, sites, seed, real=False, p_zero=0.0, singles=True, **kw):
    return dict(dict(n=n, d=d, total=total, dim=dim, op=(seed, sites, real, p_zero, singles), real=real, gen=True, epilogues=5, rows=None), **kw)


CASES = {
    "d2_n64_q63": _case(2, 64, 63, 64, _spread(64, 40, 1), 11, edge=("bit63", "nb64")),
    "d2_n64_q1": _case(2, 64, 1, 64, _spread(64, 40, 1), 12, real=True, edge=("bit63", "nb64")),
    "d2_n64_q63_239pairs": _case(2, 64, 63, 64, _spread(64, 239, 2), 13, real=True, edge=("bit63", "max_row240")),
    "d2_n64_q3": _case(2, 64, 3, 41664, _spread(64, 14, 3), 14, edge=("bit63", "blocks")),
    "d3_n32_q2": _case(3, 32, 2, 528, _spread(32, 20, 4), 15, real=True, edge=("w64",)),
    "d3_n32_q62": _case(3, 32, 62, 528, _spread(32, 20, 4), 16, edge=("bit63", "top_full")),
    "d4_n32_q2": _case(4, 32, 2, 528, _spread(32, 14, 5), 17, edge=("w64",)),
    "d4_n32_q94": _case(4, 32, 94, 528, _spread(32, 14, 5), 18, real=True, edge=("bit63", "top_full")),
    "d6_n21_q3": _case(6, 21, 3, 1771, _spread(21, 12, 6), 19, edge=("bits3",)),
    "d7_n21_q3": _case(7, 21, 3, 1771, _spread(21, 10, 7), 20, real=True, edge=("bits3",)),
    "d8_n21_q3": _case(8, 21, 3, 1771, _spread(21, 8, 8), 21, edge=("bits3",)),
    "d8_n21_q145": _case(8, 21, 145, 231, _spread(21, 8, 8), 22, edge=("bits3", "top_full")),
    "d8_n7_q12": _case(8, 7, 12, 17094, _spread(7, 6, 9), 23, p_zero=0.3, edge=("bits3", "blocks")),
    "d7_n8_q10": _case(7, 8, 10, 18488, _spread(8, 7, 10), 24, real=True, p_zero=0.3, edge=("bits3", "blocks")),
    "d6_n9_q9": _case(6, 9, 9, 22825, _spread(9, 8, 11), 25, p_zero=0.3, edge=("bits3", "blocks")),
    "d8_n12_q5_34full": _case(8, 12, 5, 4368, _spread(12, 34, 12), 26, edge=("max_row239", "tlds_off")),
    "d2_n32_q16_alternating": _case(2, 32, 16, 601080390, _even_odd(239, 13), 27, real=True, rows="alternating", epilogues=2,
                                    edge=("max_row240", "row240")),
    "d8_n12_q5_15cls": _case(8, 12, 5, 4368, _spread(12, 15, 14), 28, edge=("tlds_on", "boundary")),
    "d8_n12_q5_16cls": _case(8, 12, 5, 4368, _spread(12, 16, 14), 28, edge=("tlds_off", "boundary")),
    "d8_n12_q5_15cls_real": _case(8, 12, 5, 4368, _spread(12, 15, 14), 29, real=True, edge=("tlds_on", "boundary")),
    "d8_n12_q5_16cls_real": _case(8, 12, 5, 4368, _spread(12, 16, 14), 29, real=True, edge=("tlds_off", "boundary")),
    "d8_n5_q0": _case(8, 5, 0, 1, _spread(5, 5, 15), 30, edge=("dim1",)),
    "d8_n5_q35": _case(8, 5, 35, 1, _spread(5, 5, 15), 31, real=True, edge=("dim1",)),
    "d3_n15_q15": _case(3, 15, 15, 1787607, [(0, 14), (0, 1), (6, 7), (13, 14), (3, 9)], 32, real=True, gen=False, epilogues=1,
                        edge=("grid_stride",)),
    # the slot list, on 6 sites of 4 levels (dim 580)
    "slots_diagonal_class": _case(4, 6, 9, 580, [(0, 5), (0, 1), (2, 4)], 33, edge=("maxk0",), special="diagonal"),
    "slots_shared_class": _case(4, 6, 9, 580, [(0, 5), (1, 2), (3, 4)], 34, real=True, edge=("shared",), special="shared"),
    "slots_cancelled": _case(4, 6, 9, 580, [(0, 5), (1, 3)], 35, edge=("cancelled",), special="cancelled"),
    "slots_no_singles": _case(4, 6, 9, 580, [(0, 5), (1, 2), (2, 3)], 36, real=True, singles=False, edge=("no_single",)),
    "slots_diagonal_only": _case(4, 6, 9, 580, [(0, 5)], 37, real=True, edge=("maxk0", "diag_operator"), special="all_diagonal"),
}
BOUNDARY_PAIRS = [("d8_n12_q5_15cls", "d8_n12_q5_16cls"), ("d8_n12_q5_15cls_real", "d8_n12_q5_16cls_real")]
CANCEL_AT = (1 * 4 + 2, 2 * 4 + 1)                     # |1 2> <-> |2 1> of the repeated pair


@lru_cache(maxsize=None)
def operator(name):
    """(pairs, singles) of a case.  Shared between tests: leave the arrays unchanged."""
    c = CASES[name]
    seed, sites, real, p_zero, singles = c["op"]
    n, d = c["n"], c["d"]
    special = c.get("special")
    pairs, sg = draw_operator(seed, n, d, sites, real, p_zero, singles)
    rng = np.random.default_rng(seed + 1000)
    if special == "diagonal":                          # a pair whose matrix is diagonal: a class with maxk = 0, slot base 0
        pairs.append((1, 3, draw_pair(rng, d, real, diagonal_only=True)))
    elif special == "all_diagonal":
        pairs = [(i, j, draw_pair(rng, d, real, diagonal_only=True)) for (i, j, _) in pairs]
    elif special == "shared":                          # two further pairs carry the first pair's merged matrix
        i, j, M = pairs[0]
        Ms = M if i < j else M[np.ix_(swap_index(d), swap_index(d))]
        pairs += [(2, 5, Ms), (4, 1, Ms[np.ix_(swap_index(d), swap_index(d))])]
    elif special == "cancelled":                       # the second pair once more, as (j, i), one element (and its conjugate) negated
        i, j, M = pairs[1]
        sw = swap_index(d)
        Mo = M if i < j else M[np.ix_(sw, sw)]        # in (lo, hi) order
        extra = draw_pair(rng, d, real, p_zero=0.5)
        r, cc = CANCEL_AT
        assert Mo[r, cc] != 0
        extra[r, cc], extra[cc, r] = -Mo[r, cc], -Mo[cc, r]
        pairs.append((max(i, j), min(i, j), extra[np.ix_(sw, sw)]))
    for (_, _, M) in pairs:
        M.setflags(write=False)
    return pairs, sg


def case_rows(name):
    c = CASES[name]
    return _alt_rows() if c["rows"] == "alternating" else None


@lru_cache(maxsize=None)
def reference_of(name):
    """`assemble` of a case, cached for the session (the arrays are shared: leave them unchanged)."""
    c = CASES[name]
    pairs, sg = operator(name)
    return assemble(c["n"], c["d"], c["total"], pairs, sg, rows=case_rows(name), keep_terms=c["dim"] <= 50_000 or c["rows"] is not None)


@lru_cache(maxsize=None)
def layout_of(name):
    c = CASES[name]
    pairs, sg = operator(name)
    return mf_layout(c["n"], c["d"], c["total"], pairs, sg)


def gen_shards(nrows):
    """row ranges of the generator's shard tests: first row, last row, 63 / 64 / 65 rows, a range across a 64-row fill block"""
    cand = {"first_row": (0, 1), "last_row": (nrows - 1, nrows), "63": (5, 68), "64": (5, 69), "65": (5, 70), "across_64": (40, 100)}
    return {k: (a, b) for k, (a, b) in cand.items() if 0 <= a < b <= nrows}


def instances(name):
    """the (REALX, TLDS) instances of k_mf_qudit the case runs: complex x always, real x where every amplitude is real"""
    t = bool(layout_of(name).tables_lds)
    return {(False, t)} | ({(True, t)} if CASES[name]["real"] else set())


def qudit_dim(n, d, total):
    return sum((-1) ** k * comb(n, k) * comb(total - k * d + n - 1, n - 1) for k in range(total // d + 1))


# ------------------------------------------------------------------------------------------------------------- faults --
def tampered(asm, how, row=None):
    """(ia, ja, val) of the reference with one fault a wrong generator would make (tests/test_quditforms.py shows each rejected)."""
    ia, ja, val = asm.ia.copy(), asm.ja.copy(), asm.val.copy()
    val[asm.is_diag] = asm.diag.astype(np.float64)
    rows = np.repeat(np.arange(asm.nrows), np.diff(ia))
    off = np.nonzero(~asm.is_diag & ((rows == row) if row is not None else True))[0]
    p = int(off[len(off) // 2])
    if how == "dropped":
        keep = np.ones(len(ja), dtype=bool)
        keep[p] = False
        ia[rows[p] + 1:] -= 1
        return ia, ja[keep], val[keep]
    if how == "flipped":
        val[p] = -val[p]
    elif how == "column":
        ja[p] += 1 if (p + 1 == ia[rows[p] + 1] or ja[p + 1] > ja[p] + 1) else -1
    elif how == "diagonal_term":
        i = int(rows[p])
        k = int(np.nonzero(asm.is_diag & (rows == i))[0][0])
        t = asm.t_val[asm.t_ia[i]:asm.t_ia[i + 1]][asm.t_ja[asm.t_ia[i]:asm.t_ia[i + 1]] == asm.r0 + i]
        val[k] -= complex(t[np.argmax(np.abs(t))])
    else:
        raise KeyError(how)
    return ia, ja, val
