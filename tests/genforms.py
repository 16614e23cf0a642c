"""References, comparator and case tables for the device generators (qbh_gen.hip) and the basis reordering kernels
(qbh_reorder.hip) -- plain numpy, no GPU.  Shared by tests/test_genforms.py (CPU) and tests/test_gpu_genforms.py.

* hubbard_gen / heisenberg_gen: both models assembled, vectorised, in the GENERATOR's order (include/qbhip.h); the Python loops
  of tests/fastham.py stay as the slow cross-check (test_genforms pins entry-by-entry agreement at small sizes).
* permute_expected: P D H D P^T from a generator-order CSR alone -- Lin keys and the swap-parity sign computed here, not taken
  from tests/refham.py, so that "the kernels permuted correctly" and "the conventions are the reference's" are two checks.
* assert_same_csr: ia, then ja, then values; the first differing row is printed from both sides.
* the case tables, with the properties every GPU case relies on (test_genforms asserts them on the reference).
"""
import functools

import numpy as np

import refham

EPS = float(np.finfo(np.float64).eps)
DROP = 1e-14                       # QBH_SPARSE_PRECISION: an off-diagonal |v| below it is not stored
REF_MAX_ROW = 64                   # kRefMaxRow: longer rows take k_ref_fill's insertion sort
SCAN_CHUNK = 2048                  # exclusive_scan's chunk
MAX_BONDS = 192                    # kMaxBonds of qbh_gen_heisenberg
TRIP_GEN_HUBBARD = 16384 * 8       # rows one trip of k_gen_hubbard writes (16384 blocks, 32 lanes per row)
TRIP_REF_KEYS = 2048 * 256         # k_ref_keys, k_ref_pos, k_inv_maps
TRIP_REF_FILL = 4096 * 256         # k_ref_fill
LD = np.longdouble


# ------------------------------------------------------------------------------ bases
def patterns(L, n):
    """All L-bit integers with n bits set, ascending (= colexicographic rank order), int64 (L <= 63)."""
    @functools.lru_cache(maxsize=None)
    def rec(m, k):
        if k < 0 or k > m:
            return np.zeros(0, dtype=np.int64)
        if k == 0:
            return np.zeros(1, dtype=np.int64)
        return np.concatenate([rec(m - 1, k), rec(m - 1, k - 1) | (np.int64(1) << np.int64(m - 1))])
    return rec(L, n)


def popcount(x, nbits):
    c = np.zeros(x.shape, dtype=np.int64)
    for b in range(nbits):
        c += (x >> np.int64(b)) & 1
    return c


def merge(bonds):
    """[(a, b), ...] with multiplicity -> sorted [((lo, hi), weight), ...]."""
    w = {}
    for (a, b) in bonds:
        key = (min(a, b), max(a, b))
        w[key] = w.get(key, 0.0) + 1.0
    return sorted(w.items())


def complete_bonds(n, without=()):
    gone = {(min(a, b), max(a, b)) for (a, b) in without}
    return [(a, b) for a in range(n) for b in range(a + 1, n) if (a, b) not in gone]


def _csr_from_coo(dim, rows, cols, vals):
    """Entries (unique (row, col)) -> (ia, ja, val) with columns ascending; values are only moved."""
    order = np.argsort(rows * np.int64(dim) + cols)
    ia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=dim), out=ia[1:])
    return ia, cols[order], vals[order].astype(np.complex128)


# ------------------------------------------------------------------------------ generator order
def hop_entries(L, n, bonds, t):
    """One species: (configurations, rows, cols, values) of -t w (-1)^(particles between) c+_b c_a over both directions of every
    merged bond.  A (configuration, bond, direction) names its target uniquely, so every value is the single product -t * w * sign."""
    cfg = patterns(L, n)
    idx = np.arange(len(cfg), dtype=np.int64)
    rows, cols, vals = [], [], []
    for (s0, s1), w in merge(bonds):
        between = np.int64(((1 << s1) - 1) & ~((1 << (s0 + 1)) - 1))
        sign = 1.0 - 2.0 * (popcount(cfg & between, L) & 1)
        for (a, b) in ((s0, s1), (s1, s0)):
            can = (((cfg >> np.int64(a)) & 1) == 1) & (((cfg >> np.int64(b)) & 1) == 0)
            tgt = (cfg[can] ^ (np.int64(1) << np.int64(a))) | (np.int64(1) << np.int64(b))
            v = (-t * w) * sign[can]
            keep = np.abs(v) >= DROP
            rows.append(idx[can][keep])
            cols.append(np.searchsorted(cfg, tgt)[keep])
            vals.append(v[keep])
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)       # noqa: E731
    return cfg, cat(rows, np.int64), cat(cols, np.int64), cat(vals, np.float64)


def hubbard_gen(L, n_up, n_dn, bonds, t=1.0, U=1.1):
    """index = rank(up) * C(L, n_dn) + rank(dn), all up operators before all down operators; the diagonal U * popcount(up & dn)
    is always stored.  Returns (dim, ia, ja, val)."""
    cu, ru, tu, vu = hop_entries(L, n_up, bonds, t)
    cd, rd, td, vd = hop_entries(L, n_dn, bonds, t)
    Nu, Nd = len(cu), len(cd)
    dim = Nu * Nd
    d_all, u_all = np.arange(Nd, dtype=np.int64), np.arange(Nu, dtype=np.int64)
    rows = np.concatenate([(ru[:, None] * Nd + d_all[None, :]).ravel(), (u_all[:, None] * Nd + rd[None, :]).ravel(), np.arange(dim, dtype=np.int64)])
    cols = np.concatenate([(tu[:, None] * Nd + d_all[None, :]).ravel(), (u_all[:, None] * Nd + td[None, :]).ravel(), np.arange(dim, dtype=np.int64)])
    diag = U * popcount(cu[:, None] & cd[None, :], L).astype(np.float64).ravel()
    vals = np.concatenate([np.repeat(vu, Nd), np.tile(vd, Nu), diag])
    return (dim,) + _csr_from_coo(dim, rows, cols, vals)


def heisenberg_gen(L, n_dn, bonds, J=1.0):
    """index = colexicographic rank of the down-spin pattern; off-diagonal 0.5 J w for every bond whose ends differ (not stored
    when below DROP), diagonal sum_b +-0.25 J w in merged-bond order, always stored.  Returns (dim, ia, ja, val)."""
    cfg = patterns(L, n_dn)
    dim = len(cfg)
    idx = np.arange(dim, dtype=np.int64)
    rows, cols, vals = [idx], [idx], [None]
    diag = np.zeros(dim)
    for (a, b), w in merge(bonds):
        differ = (((cfg >> np.int64(a)) ^ (cfg >> np.int64(b))) & 1) == 1
        diag += np.where(differ, -(0.25 * J * w), 0.25 * J * w)
        if abs(0.5 * J * w) < DROP:
            continue
        tgt = cfg[differ] ^ (np.int64(1) << np.int64(a)) ^ (np.int64(1) << np.int64(b))
        rows.append(idx[differ])
        cols.append(np.searchsorted(cfg, tgt))
        vals.append(np.full(len(tgt), 0.5 * J * w))
    vals[0] = diag
    return (dim,) + _csr_from_coo(dim, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def heisenberg_diag_tol(bonds, J):
    """The diagonal is a sum of n_bonds terms +-0.25 J w_b: summed in ANY order, every partial sum is bounded by S = sum_b |0.25 J w_b|
    and each of the n_bonds - 1 additions rounds by at most eps/2 * S, on either side of the comparison: n_bonds * eps * S covers both."""
    m = merge(bonds)
    return len(m) * EPS * sum(abs(0.25 * J * w) for _, w in m)


def fastham_csr(H):
    """scipy CSR of tests/fastham.py -> (dim, ia, ja, val)"""
    import fastham
    return fastham.to_ref_csr(H)


# ------------------------------------------------------------------------------ reference order
def lin_keys(kind, n, n_up, n_dn):
    """Per generator index: the reference's sort key (odd sites compacted above the even sites, src/basis.cc:1144-1190) and the
    parity of the swaps that take 'all up operators, then all down operators' to operators ordered by site (kind 1; 0 for spins)."""
    if kind == 0:
        word = patterns(n, n_dn)
        sign = np.zeros(len(word), dtype=np.int64)
        bps = 1
    else:
        up, dn = patterns(n, n_up), patterns(n, n_dn)
        U_, D_ = np.repeat(up, len(dn)), np.tile(dn, len(up))
        word = np.zeros(len(U_), dtype=np.int64)
        swaps = np.zeros(len(U_), dtype=np.int64)
        for s in range(n):
            word |= (((U_ >> np.int64(s)) & 1) << np.int64(2 * s)) | (((D_ >> np.int64(s)) & 1) << np.int64(2 * s + 1))
            swaps += ((D_ >> np.int64(s)) & 1) * popcount(U_ >> np.int64(s + 1), n)       # a down operator at s passes the up operators above s
        sign = swaps & 1
        bps = 2
    mask = np.int64((1 << bps) - 1)
    sub = [np.zeros(len(word), dtype=np.int64), np.zeros(len(word), dtype=np.int64)]
    for s in range(n):
        sub[s & 1] |= ((word >> np.int64(s * bps)) & mask) << np.int64((s // 2) * bps)
    n_even = (n + 1) // 2
    return (sub[1] << np.int64(n_even * bps)) | sub[0], sign


def lin_order(kind, n, n_up, n_dn):
    """(order, pos, sign): reference row r holds generator index order[r]; pos[g] = its reference row."""
    keys, sign = lin_keys(kind, n, n_up, n_dn)
    order = np.argsort(keys, kind="stable")
    assert np.all(np.diff(keys[order]) > 0)                      # keys are distinct: the order is a permutation, nothing is tied
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order), dtype=np.int64)
    return order, pos, sign


def permute_expected(ia, ja, val, kind, n, n_up, n_dn):
    """H_ref = P D H_gen D P^T from the generator's CSR alone: (ia, ja, val) with columns ascending.  Values are moved and
    negated, never rounded."""
    ia, ja = np.asarray(ia, dtype=np.int64), np.asarray(ja, dtype=np.int64)
    dim = len(ia) - 1
    order, pos, sign = lin_order(kind, n, n_up, n_dn)
    assert len(order) == dim
    rows = np.repeat(np.arange(dim, dtype=np.int64), np.diff(ia))
    flip = (sign[rows] ^ sign[ja]) == 1
    v = np.where(flip, -np.asarray(val), np.asarray(val))
    return _csr_from_coo(dim, pos[rows], pos[ja], v)


def full_from_upper(dim, ia, ja, val):
    """Both triangles of a Hermitian-upper CSR, every stored entry kept (explicit zero diagonals included)."""
    rows = np.repeat(np.arange(dim, dtype=np.int64), np.diff(ia))
    off = ja > rows
    return _csr_from_coo(dim, np.concatenate([rows, ja[off]]), np.concatenate([ja, rows[off]]), np.concatenate([val, np.conj(val[off])]))


def product_structure(ia, ja, order, n_minor):
    """What k_ref_precheck asks of arrays in the reference's order: with row r standing for index g = order[r], does every
    entry keep the major index g // n_minor or the minor index g % n_minor?"""
    g = np.asarray(order, dtype=np.int64)
    rows = np.repeat(np.arange(len(ia) - 1, dtype=np.int64), np.diff(ia))
    gr, gc = g[rows], g[np.asarray(ja, dtype=np.int64)]
    return bool(np.all((gr // n_minor == gc // n_minor) | (gr % n_minor == gc % n_minor)))


# ------------------------------------------------------------------------------ comparator
def _row_text(ia, ja, val, r):
    if r + 1 >= len(ia) or ia[r] < 0 or ia[r + 1] > len(ja) or ia[r + 1] < ia[r]:
        return "(row %d not addressable)" % r
    sl = slice(int(ia[r]), int(ia[r + 1]))
    return "cols %s vals %s" % (np.asarray(ja[sl]).tolist(), [complex(v) for v in np.asarray(val[sl])])


def assert_same_csr(got, want, exact, tol=None):
    """got, want = (ia, ja, val).  Row pointers, then columns, then values: exact -> no entry may differ at all (np.array_equal's
    comparison, the last bit included); otherwise |got - want| <= tol (a scalar or one figure per entry).  The failure names the
    first differing row and prints it from both sides."""
    gia, gja, gval = (np.asarray(a) for a in got)
    wia, wja, wval = (np.asarray(a) for a in want)

    def fail(what, row):
        raise AssertionError("%s: first differing row %d\n  got  %s\n  want %s" % (
            what, row, _row_text(gia, gja, gval, row), _row_text(wia, wja, wval, row)))

    if gia.shape != wia.shape:
        raise AssertionError("row pointers: %d rows, expected %d" % (len(gia) - 1, len(wia) - 1))
    bad = np.flatnonzero(gia != wia)
    if len(bad):
        fail("row pointer %d is %d, expected %d" % (bad[0], gia[bad[0]], wia[bad[0]]), max(int(bad[0]) - 1, 0))
    rows = np.repeat(np.arange(len(wia) - 1, dtype=np.int64), np.diff(wia))
    if gja.shape != wja.shape or gval.shape != wval.shape:
        raise AssertionError("%d columns and %d values, expected %d" % (len(gja), len(gval), len(wja)))
    bad = np.flatnonzero(gja != wja)
    if len(bad):
        fail("column at entry %d is %d, expected %d" % (bad[0], gja[bad[0]], wja[bad[0]]), int(rows[bad[0]]))
    if exact:
        bad = np.flatnonzero(gval != wval)
    else:
        assert tol is not None
        bad = np.flatnonzero(~(np.abs(gval - wval) <= tol))
    if len(bad):
        fail("value at entry %d is %r, expected %r" % (bad[0], complex(gval[bad[0]]), complex(wval[bad[0]])), int(rows[bad[0]]))


def shard_of(ref, r0, r1):
    """rows [r0, r1) of (dim, ia, ja, val) as a shard downloads them: local row pointers from 0, global columns"""
    _, ia, ja, val = ref
    return ia[r0:r1 + 1] - ia[r0], ja[ia[r0]:ia[r1]], val[ia[r0]:ia[r1]]


# ------------------------------------------------------------------------------ y = H x in long double
def probe_x(n, seed):
    """complex components of modulus in [0.25, 1]"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.25, 1.0, n) * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex128)


def multmv_ld(ia, ja, val, x):
    """(Re, Im, (|H||x|)_i) of H x for a real-valued full-storage CSR (every row holds its diagonal: no empty row), in long double."""
    assert not np.any(np.asarray(val).imag) and np.all(np.diff(ia) > 0)
    a = np.asarray(val).real.astype(LD)
    xs = x[ja]
    start = np.asarray(ia[:-1], dtype=np.int64)
    re = np.add.reduceat(a * xs.real.astype(LD), start)
    im = np.add.reduceat(a * xs.imag.astype(LD), start)
    ab = np.add.reduceat(np.abs(a) * np.abs(xs).astype(LD), start)
    return re, im, ab


def assert_multmv(y, ia, ja, val, x, what=""):
    """|y_i - ref_i| <= (nnz_i + 8) eps (|H||x|)_i, whatever order the row was summed in (tests/test_gpu_realforms.py)."""
    re, im, ab = multmv_ld(ia, ja, val, x)
    err = np.hypot(y.real.astype(LD) - re, y.imag.astype(LD) - im)
    bound = (np.diff(ia).astype(LD) + 8) * LD(EPS) * ab
    ratio = err / np.maximum(bound, LD(np.finfo(np.float64).tiny))
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1.0, "%s: row %d: |y - ref| = %.3e, bound %.3e; %d rows over" % (what, i, float(err[i]), float(bound[i]), int((ratio > 1).sum()))


# ------------------------------------------------------------------------------ case tables
SQ33 = refham.square_bonds(3, 3)
LONG13 = dict(L=13, n_up=6, n_dn=2, bonds=complete_bonds(13, without=[(0, 1), (2, 3), (5, 9)]))
LONG13_ROWS = {60: 3360, 61: 19824, 62: 42000, 63: 42936, 64: 21504, 65: 4224}
LONG13_DIM, LONG13_NNZ = 133848, 8370648
LONG17 = dict(L=17, n_dn=8, bonds=complete_bonds(16) + [(15, 16), (16, 0)])
LONG17_ROWS = {64: 2002, 65: 9009, 66: 10296, 67: 3003}
LONG17_DIM, LONG17_NNZ = 24310, 1594450
CHAIN23_DIM = 1352078

# id -> (L, n_up, n_dn, bonds, t, U): generator order, whole operator
HUBBARD_GEN = {
    "chain2_1+1_one_bond": (2, 1, 1, [(0, 1)], 1.0, 1.1),
    "3x3_4+3": (9, 4, 3, SQ33, 1.0, 1.1),
    "3x3_2+5": (9, 2, 5, SQ33, 1.0, 1.1),
    "3x3_4+3_t0.7_U4": (9, 4, 3, SQ33, 0.7, 4.0),
    "no_up": (6, 0, 2, refham.chain_bonds(6), 1.0, 1.1),
    "no_dn": (6, 3, 0, refham.chain_bonds(6), 1.0, 1.1),
    "up_full": (6, 6, 2, refham.chain_bonds(6), 1.0, 1.1),
    "both_empty": (4, 0, 0, refham.chain_bonds(4), 1.0, 1.1),
    "both_full": (4, 4, 4, refham.chain_bonds(4), 1.0, 1.1),
    "empty_and_full": (4, 0, 4, refham.chain_bonds(4), 1.0, 1.1),
    "weight3": (5, 2, 2, [(0, 1), (0, 1), (1, 0), (1, 2), (2, 3), (3, 4), (4, 0)], 0.7, 4.0),
    "chain31_1+1": (31, 1, 1, refham.chain_bonds(31), 1.0, 1.1),
}
# species without a hop: the diagonal is slot 0 of every row (k_gen_hubbard's nlo_u = nlo_d = 0 with nothing above either)
HUBBARD_DIAGONAL_ONLY = ["both_empty", "both_full", "empty_and_full"]
HUBBARD_DIM_ONE = HUBBARD_DIAGONAL_ONLY

BONDS21 = complete_bonds(21)                     # 210 pairs
# id -> (L, n_dn, bonds, J)
HEIS_GEN = {
    "all_up": (6, 0, refham.chain_bonds(6), 1.0),
    "all_down": (6, 6, refham.chain_bonds(6), 1.0),
    "one_down": (7, 1, refham.chain_bonds(7), 1.0),
    "L63_1": (63, 1, refham.chain_bonds(63), 1.0),
    "L63_2": (63, 2, refham.chain_bonds(63), 1.0),
    "L63_2_J0.7": (63, 2, refham.chain_bonds(63), 0.7),
    "L40_3": (40, 3, refham.chain_bonds(40), 1.0),
    "L34_33": (34, 33, refham.chain_bonds(34), 1.0),
    "repeated_bonds": (10, 4, refham.chain_bonds(10) + [(0, 1), (1, 0), (3, 7), (7, 3), (2, 9), (2, 9), (2, 9), (9, 2)], 1.0),
    "repeated_bonds_J0.7": (10, 4, refham.chain_bonds(10) + [(0, 1), (1, 0), (3, 7), (7, 3), (2, 9), (2, 9), (2, 9), (9, 2)], 0.7),
    "192_bonds": (21, 3, BONDS21[:MAX_BONDS], 1.0),
    "192_bonds_J0.7": (21, 3, BONDS21[:MAX_BONDS], 0.7),
    "long17": (17, 8, LONG17["bonds"], 1.0),
    "J0": (10, 4, refham.chain_bonds(10), 0.0),
    "J1e-15": (10, 4, refham.chain_bonds(10), 1e-15),
    "J1e-15_weight_over_the_rule": (8, 3, refham.chain_bonds(8) + [(2, 5)] * 30, 1e-15),      # 0.5 J w = 1.5e-14 for one bond: stored
}
HEIS_REFUSED_BONDS = (21, 3, BONDS21[:MAX_BONDS + 1], 1.0)

# row shards: (case id, [(r0, r1), ...])
HUBBARD_SHARD_CASE = "3x3_4+3"                    # Nu = 126 up blocks of Nd = 84 rows
HUBBARD_ND = 84
HUBBARD_SHARDS = {"first_row": (0, 1), "last_row": (10583, 10584), "inside_a_block": (84 * 3 + 10, 84 * 3 + 57),
                  "inside_to_boundary": (100, 84 * 4), "boundary_to_inside": (84 * 4, 84 * 7 + 5), "boundary_to_boundary": (84 * 9, 84 * 11)}
HEIS_SHARD_CASE = (16, 8, refham.chain_bonds(16), 0.7)       # dim 12870
HEIS_SHARD_DIM = 12870
HEIS_SHARD_START = 301
HEIS_SHARDS = {"first_row": (0, 1), "last_row": (12869, 12870), "2047": (301, 301 + 2047), "2048": (301, 301 + 2048), "2049": (301, 301 + 2049),
               "4097": (301, 301 + 4097)}

# reference order: id -> (L, n_up, n_dn, bonds); the square cases are refham.hubbard_csr's own lattices
REF_ELECTRON = {
    "3x3_4+3": (9, 4, 3, SQ33),
    "3x3_2+5": (9, 2, 5, SQ33),
    "5x1_2+3": (5, 2, 3, refham.chain_bonds(5)),       # square_bonds(5, 1) without its y-bonds (s, s), which the generators refuse and which add nothing
    "4x2_3+5": (8, 3, 5, refham.square_bonds(4, 2)),
    "chain31_1+1": (31, 1, 1, refham.chain_bonds(31)),
    "long13": (13, 6, 2, LONG13["bonds"]),
}
REF_SPIN = {
    "chain15_6": (15, 6, refham.chain_bonds(15)),
    "chain32_2": (32, 2, refham.chain_bonds(32)),
    "long17": (17, 8, LONG17["bonds"]),
    "chain23_11": (23, 11, refham.chain_bonds(23)),
}
INVERSE = ["3x3_4+3", "3x3_2+5", "5x1_2+3", "long13"]
WRONG_HINT = ("3x3_4+3", (9, 3, 4))               # the dimension of the operator, the fillings swapped


@functools.lru_cache(maxsize=None)
def hubbard_gen_case(name):
    L, nu, nd, bonds, t, U = HUBBARD_GEN[name]
    return hubbard_gen(L, nu, nd, bonds, t, U)


@functools.lru_cache(maxsize=None)
def heis_gen_case(name):
    L, nd, bonds, J = HEIS_GEN[name]
    return heisenberg_gen(L, nd, bonds, J)


@functools.lru_cache(maxsize=None)
def electron_gen(name):
    """generator order, t = 1, U = 1.1"""
    L, nu, nd, bonds = REF_ELECTRON[name]
    return hubbard_gen(L, nu, nd, bonds, 1.0, 1.1)


@functools.lru_cache(maxsize=None)
def electron_ref_upper(name):
    """refham's Hermitian-upper arrays in the reference's order: (dim, ia, ja, val)"""
    L, nu, nd, bonds = REF_ELECTRON[name]
    return refham.hubbard_csr(L, 1, nu, nd, t=1.0, U=1.1, bonds=bonds)[:4]


@functools.lru_cache(maxsize=None)
def electron_ref_full(name):
    dim, ia, ja, val = electron_ref_upper(name)
    return (dim,) + full_from_upper(dim, ia, ja, val)


@functools.lru_cache(maxsize=None)
def spin_gen(name):
    L, nd, bonds = REF_SPIN[name]
    return heisenberg_gen(L, nd, bonds, 1.0)


@functools.lru_cache(maxsize=None)
def spin_ref_full(name):
    L, nd, bonds = REF_SPIN[name]
    dim, ia, ja, val, _ = refham.heisenberg_csr(L, bonds, J=1.0, n_dn=nd)
    return (dim,) + full_from_upper(dim, ia, ja, val)


def row_histogram(ia):
    ln, cnt = np.unique(np.diff(ia), return_counts=True)
    return dict(zip(ln.tolist(), cnt.tolist()))
