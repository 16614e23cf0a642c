"""Host-only helpers for the entry-by-entry tests of operator creation from host arrays (qbh_csr_create / qbh_csr_create_rows ->
qbh_build.hip, the exclusive scan, the value dictionary and the shard column split of qbh_csrprep.hip) and of the re-ordering
pass of qbh_reorder.hip.

Two parts, numpy only (no GPU, no oracle, no scipy arithmetic: scipy drops stored zeros and may normalise signed zeros):

* `make(name)`: synthetic host matrices in the reference host layout (int64 ia / ja, complex128 val) whose row structure sits on
  the boundaries of the creation kernels.  Every profile returns the facts it claims and asserts them itself;
* the reference of what the device must hold: `expand` (the layout documented at the head of qbh_build.hip), `distinct_bits`
  / `code_width` (the dictionary counts bit patterns), `ref_order` / `reordered` (the convention at the head of
  qbh_reorder.hip, state by state in Python integers) and `same_bits`.
"""
import functools
import itertools
import math

import numpy as np

K_SHORT_CAP = 96          # qbh_build.hip kShortCap: longest mirrored part k_sort_lower_short sorts
K_BLOCK = 256             # workgroup of k_sort_lower_long
K_LONG_GRID = 4096        # largest grid of k_sort_lower_long
K_SCAN_CHUNK = 2048       # qbh_csrprep.hip kScanChunk
K_REF_MAX_ROW = 64        # qbh_reorder.hip kRefMaxRow
DICT_MAX = 65536          # qbh_dict.hpp kDictMax

MIRROR_L = (0, 1, 2, 95, 96, 97, 255, 256, 257, 600, 1500)
MIRROR_OWN = (0, 1, 40, 130)
SCAN_N = (1, 2, 2047, 2048, 2049, 4096, 4097, 6145)
DICT_N = (1, 255, 256, 257, 65535, 65536, 65537)


# ------------------------------------------------------------------------------------------------------------- bits ----
def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float64, np.complex128), a.dtype
    return a.view(np.uint64)


def same_bits(a, b):
    """float64 / complex128 arrays equal bit for bit (-0.0 is not +0.0, a last-bit neighbour is not the value)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def distinct_bits(val):
    """Number of distinct complex128 values by bit pattern: what the device dictionary (keyed by the two 64-bit words) counts."""
    w = _bits(np.asarray(val, dtype=np.complex128)).reshape(-1, 2)
    return int(len(np.unique(w, axis=0))) if len(w) else 0


def code_width(n):
    """Bytes per code of a dictionary of n values (qbh_dict.hpp dict_code_width); 0: not coded."""
    return 0 if n < 1 or n > DICT_MAX else 1 if n <= 256 else 2


def csr_mismatch(got, want):
    """None when the CSR triple `got` (ia, ja, val) is `want` -- pointers and columns exactly, values bit for bit -- else a line
    naming the first difference.  The one comparison every download in the GPU tests goes through."""
    (gia, gja, gval), (wia, wja, wval) = got, want
    gia, wia = np.asarray(gia, dtype=np.int64), np.asarray(wia, dtype=np.int64)
    if gia.shape != wia.shape or not np.array_equal(gia, wia):
        k = int(np.argmax(gia != wia)) if gia.shape == wia.shape else -1
        return "row pointers differ (first at %d: %s, want %s)" % (k, gia[k] if k >= 0 else gia.shape, wia[k] if k >= 0 else wia.shape)
    gja, wja = np.asarray(gja, dtype=np.int64), np.asarray(wja, dtype=np.int64)
    if gja.shape != wja.shape or not np.array_equal(gja, wja):
        k = int(np.argmax(gja != wja)) if gja.shape == wja.shape else -1
        row = int(np.searchsorted(wia, k, side="right")) - 1 if k >= 0 else -1
        return "columns differ (first at entry %d, row %d: %s, want %s)" % (k, row, gja[k] if k >= 0 else gja.shape,
                                                                           wja[k] if k >= 0 else wja.shape)
    gval, wval = np.asarray(gval), np.asarray(wval)
    if not same_bits(gval, wval):
        if gval.shape != wval.shape or gval.dtype != wval.dtype:
            return "values differ in shape or type"
        k = int(np.argmax(np.any(_bits(gval).reshape(-1, 2) != _bits(wval).reshape(-1, 2), axis=1)))
        row = int(np.searchsorted(wia, k, side="right")) - 1
        return "values differ by bits (first at entry %d, row %d, column %d: %r, want %r)" % (k, row, int(wja[k]), gval[k], wval[k])
    return None


# -------------------------------------------------------------------------------------------------------- reference ----
def expand(dim, ia, ja, val, sym, r0=0, r1=None):
    """Rows [r0, r1) of the device layout of qbh_build.hip as (ia rebased to 0, ja, val).

    sym: the host arrays hold the upper triangle (col >= row).  Device row c then holds first the mirrored copies (c, r, conj v) of
    the host entries (r, c, v), r < c, in ascending r, then the row's own host entries in the order given.  Full storage: the rows
    as given."""
    r1 = dim if r1 is None else r1
    ia = np.asarray(ia, dtype=np.int64)
    ja = np.asarray(ja, dtype=np.int64)
    val = np.asarray(val, dtype=np.complex128)
    n = r1 - r0
    own_len = ia[r0 + 1:r1 + 1] - ia[r0:r1]
    own_j, own_v = ja[ia[r0]:ia[r1]], val[ia[r0]:ia[r1]]
    if not sym:
        return (ia[r0:r1 + 1] - ia[r0]).copy(), own_j.copy(), own_v.copy()
    rows = np.repeat(np.arange(dim, dtype=np.int64), np.diff(ia))
    m = (ja != rows) & (ja >= r0) & (ja < r1)
    m_row, m_col, m_val = ja[m] - r0, rows[m], np.conj(val[m])
    order = np.lexsort((m_col, m_row))
    m_row, m_col, m_val = m_row[order], m_col[order], m_val[order]
    low = np.bincount(m_row, minlength=n).astype(np.int64)
    out_ia = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(low + own_len, out=out_ia[1:])
    out_ja = np.empty(int(out_ia[-1]), dtype=np.int64)
    out_val = np.empty(int(out_ia[-1]), dtype=np.complex128)
    low_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(low, out=low_start[1:])
    pos = out_ia[m_row] + (np.arange(len(m_row), dtype=np.int64) - low_start[m_row])
    out_ja[pos], out_val[pos] = m_col, m_val
    own_row = np.repeat(np.arange(n, dtype=np.int64), own_len)
    pos = out_ia[own_row] + low[own_row] + (np.arange(len(own_j), dtype=np.int64) - (ia[r0:r1] - ia[r0])[own_row])
    out_ja[pos], out_val[pos] = own_j, own_v
    return out_ia, out_ja, out_val


def mirrored_lengths(dim, ia, ja):
    """Per row c the number of host entries (r, c) with r != c: the mirrored part of device row c (Hermitian-upper input)."""
    rows = np.repeat(np.arange(dim, dtype=np.int64), np.diff(ia))
    return np.bincount(np.asarray(ja)[np.asarray(ja) != rows], minlength=dim).astype(np.int64)


def _patterns(n_bits, k):
    """All n_bits-bit integers with k bits set, ascending: the generators' colexicographic rank is the position in this list."""
    return sorted(sum(1 << s for s in comb) for comb in itertools.combinations(range(n_bits), k))


def ref_order(kind, n_sites, n_up, n_dn):
    """(perm, sign): reference row r holds the generator index perm[r]; sign[r] = +-1 is the factor its state picks up.

    Generator index (qbh_reorder.hip head): kind 0 the rank of the n_dn-bit pattern among the n_sites-bit patterns in ascending
    order; kind 1 rank(up) * C(n_sites, n_dn) + rank(down), all up operators before all down operators.  Reference: local states
    one bit per site (kind 0) or two (bit 0 up, bit 1 down), operators ordered by site, rows sorted by (sub_b, sub_a) with sub_b
    the odd sites compacted and sub_a the even ones.  Moving from "all up, then all down" to site order, the down operator of
    site i passes every up operator of a site j > i: the sign is the parity of the number of such pairs."""
    states = []
    if kind == 0:
        for g, dn in enumerate(_patterns(n_sites, n_dn)):
            states.append((g, [(dn >> s) & 1 for s in range(n_sites)], 0))
    else:
        ups, dns = _patterns(n_sites, n_up), _patterns(n_sites, n_dn)
        for iu, up in enumerate(ups):
            for idn, dn in enumerate(dns):
                pairs = 0
                for i in range(n_sites):
                    if (dn >> i) & 1:
                        for j in range(i + 1, n_sites):
                            pairs += (up >> j) & 1
                local = [((up >> s) & 1) | (((dn >> s) & 1) << 1) for s in range(n_sites)]
                states.append((iu * len(dns) + idn, local, pairs & 1))
    bps = 1 if kind == 0 else 2

    def compact(local, parity):
        out = 0
        for k, s in enumerate(range(parity, n_sites, 2)):
            out |= local[s] << (k * bps)
        return out
    keyed = sorted(((compact(loc, 1), compact(loc, 0)), g, odd) for g, loc, odd in states)
    perm = np.array([g for _, g, _ in keyed], dtype=np.int64)
    sign = np.array([-1 if odd else 1 for _, _, odd in keyed], dtype=np.int64)
    return perm, sign


def reordered(dim, ia, ja, val, perm, sign):
    """P D H D P^T as full-storage CSR with ascending columns: entry (g, c, v) of generator row g = perm[r] goes to
    (r, pos[c], sign[r] sign[pos[c]] v).  A sign flip is exact (both sign bits change), so the result is defined bit for bit."""
    ia = np.asarray(ia, dtype=np.int64)
    ja = np.asarray(ja, dtype=np.int64)
    val = np.asarray(val, dtype=np.complex128)
    pos = np.empty(dim, dtype=np.int64)
    pos[perm] = np.arange(dim, dtype=np.int64)
    lens = (ia[1:] - ia[:-1])[perm]
    out_ia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(lens, out=out_ia[1:])
    out_ja = np.empty(len(ja), dtype=np.int64)
    out_val = np.empty(len(ja), dtype=np.complex128)
    for r in range(dim):
        g = int(perm[r])
        c = pos[ja[ia[g]:ia[g + 1]]]
        v = val[ia[g]:ia[g + 1]]
        flip = sign[c] != sign[r]
        v = np.where(flip, np.negative(v), v)
        o = np.argsort(c, kind="stable")
        out_ja[out_ia[r]:out_ia[r + 1]] = c[o]
        out_val[out_ia[r]:out_ia[r + 1]] = v[o]
    return out_ia, out_ja, out_val


# --------------------------------------------------------------------------------------------------------- profiles ----
def _rng(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 31)
    return np.random.default_rng(h)


def _values(n, rng):
    """0.5 <= |a| <= 1.5, random phase."""
    return (rng.uniform(0.5, 1.5, n) * np.exp(2j * np.pi * rng.random(n))).astype(np.complex128)


def _upper_csr(dim, pairs, diag_rows, rng):
    """Sorted Hermitian-upper CSR of the strictly upper entries `pairs` (set of (r, c), r < c) plus a real diagonal on diag_rows."""
    r = np.array([p[0] for p in pairs] + list(diag_rows), dtype=np.int64)
    c = np.array([p[1] for p in pairs] + list(diag_rows), dtype=np.int64)
    assert np.all(r <= c)
    o = np.lexsort((c, r))
    r, c = r[o], c[o]
    v = _values(len(r), rng)
    d = r == c
    v[d] = np.abs(v[d]) * rng.choice([-1.0, 1.0], int(d.sum())) + 0j
    ia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=dim), out=ia[1:])
    return ia, c, v


def _targets_matrix(dim, targets, diag_rows, background, rng, forbidden=()):
    """Hermitian-upper matrix in which target row c has exactly targets[c] = (below, above) off-diagonal entries (r, c), r < c,
    and (c, c'), c' > c.  The partners r and c' are drawn among the rows that are no target (and not `forbidden`), so that no
    target row's counts drift; `background` further entries per ordinary row join ordinary rows only."""
    special = set(targets) | set(forbidden)
    plain = np.array([r for r in range(dim) if r not in special], dtype=np.int64)
    pairs = set()
    for c, (below, above) in targets.items():
        lo, hi = plain[plain < c], plain[plain > c]
        assert below <= len(lo) and above <= len(hi), (c, below, above)
        for r in rng.choice(lo, size=below, replace=False):
            pairs.add((int(r), c))
        for c2 in rng.choice(hi, size=above, replace=False):
            pairs.add((c, int(c2)))
    for i in range(len(plain) - 1):
        for k in rng.integers(i + 1, len(plain), size=background):
            pairs.add((int(plain[i]), int(plain[k])))
    return _upper_csr(dim, sorted(pairs), diag_rows, rng)


def _mirror(name, dim, ls, owns, empty_run, background):
    """The mirror_lengths family: one target row per (L, own) pair, spread over the upper half of the index range."""
    rng = _rng(name)
    combos = [(L, k) for L in ls for k in owns]
    need = max(ls) + len(combos) + len(empty_run) + 8
    assert dim % 2 == 1 and need < dim - 2
    # a diagonal on odd rows only (never inside the run of empty rows): row 0 and the last row (dim odd) have none
    diag_rows = [r for r in range(1, dim, 2) if r not in empty_run]
    # target rows: above every partner pool they need, ascending with L so that the long ones sit high; own = 0 needs an even row
    # (no diagonal), own > 0 counts the diagonal of an odd row
    targets, named = {}, {}
    taken = set(empty_run) | {0, dim - 1}
    base = np.linspace(0, 1, len(combos))
    for i, (L, k) in enumerate(sorted(combos, key=lambda t: (t[0], -t[1]))):
        lo = L + len(combos) + len(empty_run) + 4
        hi = dim - 2 - max(owns) - len(combos) - len(empty_run)
        assert lo <= hi, (L, k, lo, hi)
        c = lo + int(base[i] * (hi - lo))
        while c in taken or (k == 0 and c % 2 == 1):
            c += 1
        taken.add(c)
        above = k - (1 if (c % 2 == 1 and k > 0) else 0)
        targets[c] = (L, above)
        named[(L, k)] = c
    ia, ja, val = _targets_matrix(dim, targets, diag_rows, background, rng, forbidden=set(empty_run) | {0, dim - 1})
    # ---- the facts, asserted here
    low = mirrored_lengths(dim, ia, ja)
    own = np.diff(ia)
    for (L, k), c in named.items():
        assert low[c] == L and own[c] == k, ("target row", c, "wants", (L, k), "has", (int(low[c]), int(own[c])))
    empty = np.nonzero((low + own) == 0)[0]
    assert set(empty_run) | {0, dim - 1} <= set(empty.tolist()) and named[(0, 0)] in empty
    rows = np.repeat(np.arange(dim), own)
    d = set(rows[rows == ja].tolist())
    assert d == set(diag_rows) and all(r % 2 == 1 for r in d)
    assert np.all(val[rows == ja].imag == 0) and np.all(np.abs(val) >= 0.5) and np.all(np.abs(val) <= 1.5)
    for r in range(dim):
        assert np.all(np.diff(ja[ia[r]:ia[r + 1]]) > 0)
    facts = dict(rows=named, low=low, empty_rows=empty, empty_run=tuple(empty_run), n_long=int((low > K_SHORT_CAP).sum()),
                 full_nnz=int((low + own).sum()))
    return dim, ia, ja, val, 1, facts


def _mirror_lengths():
    # source rows of a column are spread over [0, c): with an upload chunk of ~1000 nonzeros they arrive from many chunks
    return _mirror("mirror_lengths", 4501, MIRROR_L, MIRROR_OWN, tuple(range(2200, 2205)), 3)


def _mirror_small():
    return _mirror("mirror_small", 701, (0, 1, 2, 95, 96, 97, 255, 256, 257), (0, 1, 40), (300, 301, 302), 2)


def _many_long():
    """4100 rows with 97 mirrored entries each (one more than kShortCap): more long rows than the grid of k_sort_lower_long."""
    rng = _rng("many_long")
    n_src, n_t, L = 200, 4100, K_SHORT_CAP + 1
    dim = n_src + n_t + 1
    pairs = []
    for c in range(n_src, n_src + n_t):
        pairs += [(int(r), c) for r in rng.choice(n_src, size=L, replace=False)]
    ia, ja, val = _upper_csr(dim, pairs, range(1, dim, 2), rng)
    low = mirrored_lengths(dim, ia, ja)
    assert int((low == L).sum()) == n_t and int((low > K_SHORT_CAP).sum()) == n_t > K_LONG_GRID and set(np.unique(low)) == {0, L}
    assert 3.9e5 < len(ja) < 4.1e5
    return dim, ia, ja, val, 1, dict(low=low, n_long=n_t, full_nnz=int(low.sum() + len(ja)))


SCAN_SEAMS = (0, 7, 8, 511, 512, 2047, 2048)     # lane (8 elements), wave (512) and chunk (2048) seams of k_scan_apply
SCAN_LENGTHS = {0: 3, 7: 5, 8: 2, 511: 7, 512: 300, 2047: 4, 2048: 6}


def _scan_edges(n):
    """Full storage, n rows, every row empty but those at the seams of the scan and the last one; one row of 300.  The row
    lengths are free only without a symmetric pattern: the matrix is not Hermitian (create it with check_hermitian = 0)."""
    rng = _rng("scan_edges/%d" % n)
    lens = np.zeros(n, dtype=np.int64)
    for i in SCAN_SEAMS:
        if i < n:
            lens[i] = min(SCAN_LENGTHS[i], n)
    lens[n - 1] = max(lens[n - 1], 1)
    ia = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ia[1:])
    ja = np.concatenate([np.sort(rng.choice(n, size=int(k), replace=False)) for k in lens if k]).astype(np.int64)
    val = _values(len(ja), rng)
    want = sorted({i for i in SCAN_SEAMS if i < n} | {n - 1})
    assert np.nonzero(lens)[0].tolist() == want
    assert (n < 513) or lens.max() == 300
    return n, ia, ja, val, 0, dict(nonzero_rows=want, lengths=lens, full_nnz=int(lens.sum()))


def _unsorted():
    dim, ia, ja, val, sym, facts = _mirror_small()
    rng = _rng("unsorted")
    ja, val = ja.copy(), val.copy()
    for r in range(dim):
        p = rng.permutation(int(ia[r + 1] - ia[r]))
        ja[ia[r]:ia[r + 1]] = ja[ia[r]:ia[r + 1]][p]
        val[ia[r]:ia[r + 1]] = val[ia[r]:ia[r + 1]][p]
    unsorted_rows = sum(bool(np.any(np.diff(ja[ia[r]:ia[r + 1]]) < 0)) for r in range(dim))
    assert unsorted_rows > dim // 4 and np.all(ja >= np.repeat(np.arange(dim), np.diff(ia)))
    facts = dict(facts, unsorted_rows=unsorted_rows)
    return dim, ia, ja, val, 1, facts


def _full_storage():
    dim, ia, ja, val, _, facts = _mirror_lengths()
    fia, fja, fval = expand(dim, ia, ja, val, 1)
    assert fia[-1] == facts["full_nnz"] and np.array_equal(np.diff(fia), facts["low"] + np.diff(ia))
    return dim, fia, fja, fval, 0, dict(facts, upper=(ia, ja, val))


def _conj_class(v):
    """Key under which a value and its bitwise conjugate coincide: (bits of re, bits of im without the sign)."""
    w = _bits(np.array([v], dtype=np.complex128))
    return int(w[0]), int(w[1]) & 0x7FFFFFFFFFFFFFFF


def _dict_pool(n_pairs, n_diag, real, rng):
    """n_pairs off-diagonal values, no two of them equal or conjugate by bits, and n_diag real diagonal values.  On purpose among
    the off-diagonal ones: neighbours in the last mantissa bit, a subnormal, a value near 1e300, +0.0 and -0.0 as real and as
    imaginary parts."""
    x0 = 0.6123
    special = [complex(0.7, 0.0), complex(0.9, -0.0), complex(x0, 0.0), complex(np.nextafter(x0, 1.0), 0.0), complex(0.0, 0.0),
               complex(-0.0, 0.0), complex(5e-324, 0.0), complex(1e300, 0.0)]
    if not real:
        special += [complex(0.0, 0.7), complex(-0.0, 0.7), complex(x0, 0.8), complex(x0, np.nextafter(0.8, 1.0)),
                    complex(np.nextafter(x0, 1.0), 0.8), complex(5e-324, 1e-310), complex(1e300, -3e299)]
    off, seen = [], set()
    for v in special:
        if len(off) < n_pairs and _conj_class(v) not in seen:
            seen.add(_conj_class(v))
            off.append(v)
    while len(off) < n_pairs:
        m = n_pairs - len(off)
        cand = rng.uniform(0.5, 1.5, m) * (rng.choice([-1.0, 1.0], m) if real else np.exp(2j * np.pi * rng.random(m)))
        for v in np.asarray(cand, dtype=np.complex128):
            if _conj_class(v) not in seen:
                seen.add(_conj_class(v))
                off.append(complex(v))
    diag = np.unique(rng.uniform(2.0, 3.0, 2 * n_diag + 8))[:n_diag]
    assert len(diag) == n_diag
    return np.array(off, dtype=np.complex128), rng.permutation(diag).astype(np.complex128)


def _dict(n_values, real, upper):
    """A matrix whose device copy holds exactly n_values distinct bit patterns.  An off-diagonal host value v and its mirror
    conj(v) always differ (the sign bit of the imaginary part: x + 0i mirrors to x - 0i), so n_pairs conjugate classes
    give 2 n_pairs patterns in full storage -- and in Hermitian-upper storage once the device has mirrored them, although the
    host arrays then hold only n_pairs + n_diag."""
    name = "dict_%s/%d/%d" % ("upper" if upper else "n", n_values, int(real))
    rng = _rng(name)
    n_pairs = n_values // 3
    n_diag = n_values - 2 * n_pairs
    dim = max(600, n_diag + 150)
    per_row = 4 if n_values < 1000 else 2
    pairs = set()
    for r in range(dim - 1 if n_pairs else 0):
        for c in rng.integers(r + 1, dim, size=per_row):
            pairs.add((r, int(c)))
    pairs = sorted(pairs)
    assert len(pairs) >= n_pairs
    off, diag = _dict_pool(n_pairs, n_diag, real, rng)
    r = np.array([p[0] for p in pairs] + list(range(dim)), dtype=np.int64)
    c = np.array([p[1] for p in pairs] + list(range(dim)), dtype=np.int64)
    v = np.empty(len(r), dtype=np.complex128)
    if n_pairs:
        v[:len(pairs)] = off[rng.permutation(len(pairs)) % n_pairs]            # every pool value is used
    v[len(pairs):] = diag[np.arange(dim) % n_diag]
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    ia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=dim), out=ia[1:])
    fia, fja, fval = expand(dim, ia, c, v, 1)
    # ---- the facts
    n_dev = distinct_bits(fval)
    assert n_dev == n_values, (name, n_dev)
    assert distinct_bits(v) == n_pairs + n_diag
    rows_f = np.repeat(np.arange(dim), np.diff(fia))
    # a_ji is the bitwise conjugate of a_ij: the entries in (column, row) order are the transposed partners of those in (row, column) order
    w = _bits(fval).reshape(-1, 2)
    t = np.lexsort((rows_f, fja))
    assert np.array_equal(rows_f[t], fja) and np.array_equal(fja[t], rows_f)
    flip = np.where(rows_f != fja, np.uint64(1 << 63), np.uint64(0))
    assert np.array_equal(w[t, 0], w[:, 0]) and np.array_equal(w[t, 1], w[:, 1] ^ flip)
    if n_pairs >= 8:
        offd = fval[rows_f != fja]
        sign_im = np.signbit(offd.imag) & (offd.imag == 0)
        sign_re = np.signbit(offd.real) & (offd.real == 0)
        assert sign_im.any() and sign_re.any() and (np.abs(offd) > 1e299).any() and ((np.abs(offd) < 1e-300) & (np.abs(offd) > 0)).any()
    if real:
        assert np.all(fval.imag == 0)
    facts = dict(n_values=n_values, n_host=n_pairs + n_diag, n_pairs=n_pairs, n_diag=n_diag, full=(fia, fja, fval),
                 full_nnz=int(fia[-1]))
    if upper:
        return dim, ia, c, v, 1, facts
    return dim, fia, fja, fval, 0, facts


REORDER = {"reorder_long_0": (0, 12, 0, 6, (1, 63, 64, 65, 200)), "reorder_long_1": (1, 6, 3, 3, (1, 63, 64, 65, 200)),
           "reorder_long_1odd": (1, 5, 2, 3, (1, 63, 64, 65, 90))}


def _reorder_long(name):
    """Random Hermitian full storage of the dimension of a spin-1/2 (kind 0) or electron (kind 1) basis with rows of exactly the
    named lengths -- around kRefMaxRow = 64 and far above -- row 0 and the last row among them."""
    kind, n_sites, n_up, n_dn, lengths = REORDER[name]
    dim = math.comb(n_sites, n_dn) * (math.comb(n_sites, n_up) if kind == 1 else 1)
    rng = _rng(name)
    rows = [0, dim - 1] + sorted(int(r) for r in rng.choice(np.arange(5, dim - 5), size=len(lengths) - 2, replace=False))
    order = rng.permutation(len(lengths))
    named = {rows[i]: int(lengths[order[i]]) for i in range(len(lengths))}
    targets = {}
    for c, ln in named.items():
        off = ln - 1                                     # every row has its diagonal
        below = 0 if c == 0 else off if c == dim - 1 else int(rng.integers(0, off + 1))
        below = min(below, max(0, c - len(named)))
        above = off - below
        if above > dim - 1 - c - len(named):
            above = max(0, dim - 1 - c - len(named))
            below = off - above
        targets[c] = (below, above)
    ia, ja, val = _targets_matrix(dim, targets, range(dim), 2, rng)
    fia, fja, fval = expand(dim, ia, ja, val, 1)
    lens = np.diff(fia)
    for c, ln in named.items():
        assert lens[c] == ln, (name, c, ln, int(lens[c]))
    assert {0, dim - 1} <= set(named) and sorted(named.values()) == sorted(lengths)
    assert (lens > K_REF_MAX_ROW).any() and (lens <= K_REF_MAX_ROW).any()
    return dim, fia, fja, fval, 0, dict(kind=kind, n_sites=n_sites, n_up=n_up, n_dn=n_dn, rows=named, lengths=lens,
                                         full_nnz=int(fia[-1]))


def arrow(dim=2001):
    """Hermitian-upper arrow: a dense first row and the diagonal.  Half of the full operator's nonzeros sit in row 0."""
    ia = np.concatenate([[0], dim + np.arange(dim, dtype=np.int64)])
    ja = np.concatenate([np.arange(dim), np.arange(1, dim)]).astype(np.int64)
    val = _values(len(ja), _rng("arrow"))
    val[0] = 1.0
    val[dim:] = val[dim:].real + 0j
    return dim, ia, ja, val, 1, dict(full_nnz=3 * dim - 2)


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (dim, ia, ja, val, sym, facts).  Names: mirror_lengths, mirror_small, many_long, scan_edges_<n>, unsorted, full_storage,
    dict_n_<n>[_real], dict_upper_<n>[_real], reorder_long_0 / _1 / _1odd, arrow.  The arrays are shared: do not write to them."""
    if name == "mirror_lengths":
        out = _mirror_lengths()
    elif name == "mirror_small":
        out = _mirror_small()
    elif name == "many_long":
        out = _many_long()
    elif name.startswith("scan_edges_"):
        out = _scan_edges(int(name.split("_")[2]))
    elif name == "unsorted":
        out = _unsorted()
    elif name == "full_storage":
        out = _full_storage()
    elif name.startswith("dict_"):
        tok = name.split("_")
        out = _dict(int(tok[2]), len(tok) > 3 and tok[3] == "real", tok[1] == "upper")
    elif name in REORDER:
        out = _reorder_long(name)
    elif name == "arrow":
        out = arrow()
    else:
        raise KeyError(name)
    for a in out[1:4]:
        a.setflags(write=False)
    return out


def scan_edges(n):
    return make("scan_edges_%d" % n)


def dict_n(n_values, real=False):
    return make("dict_n_%d%s" % (n_values, "_real" if real else ""))


def dict_upper(n_values, real=False):
    return make("dict_upper_%d%s" % (n_values, "_real" if real else ""))


def reorder_long(kind, odd=False):
    return make("reorder_long_1odd" if odd else "reorder_long_%d" % kind)


def probe_vector(n, seed):
    """0.25 <= |x_j| <= 1, random phase."""
    rng = np.random.default_rng(20_000 + seed)
    return (rng.uniform(0.25, 1.0, n) * np.exp(2j * np.pi * rng.random(n))).astype(np.complex128)


TRIPLE = (0.7, -1.3, 0.5)             # (alpha, beta, gamma) of the one SpMV the creation tests run


def spmv_reference(rows, x, xl, y0, triple=TRIPLE):
    """Long-double y = alpha H x + beta y0 + gamma xl of the device rows `rows` = (ia, ja, val) with the per-row bound and the
    reduction bounds of csrforms.epilogue (imported, not restated)."""
    import csrforms as cf
    ia, ja, val = rows
    s, abs_s = cf.row_sums(ia, ja, val, x)
    return cf.epilogue(s, abs_s, np.diff(ia), xl, y0, *triple)


# ------------------------------------------------------------------------------------------------------------ shards ----
def shard_cuts(name):
    """The row ranges test b. cuts a profile at, as {label: (r0, r1)}."""
    dim, ia, ja, val, sym, facts = make(name)
    cuts = {"first_row": (0, 1), "last_row": (dim - 1, dim)}
    if name in ("mirror_lengths", "full_storage"):
        t = facts["rows"]
        c1500, c600, c257 = t[(1500, 40)], t[(600, 130)], t[(257, 1)]
        e = facts["empty_run"]
        cuts.update({"long_row_first": (c600, c600 + 300), "long_row_last": (c257 - 300, c257 + 1),
                     "long_row_just_outside": (c257 + 1, c600), "one_row_1500": (c1500, c1500 + 1),
                     "empty_rows_only": (e[0], e[-1] + 1), "two_thirds": (dim // 3, dim)})
    else:
        n = dim
        cuts.update({"chunk_seam_first": (K_SCAN_CHUNK, n), "chunk_seam_last": (0, K_SCAN_CHUNK + 1),
                     "seam_just_outside": (9, 2047),"long_row_only": (512, 513), "empty_rows_only": (600, 1900)})
    return cuts
