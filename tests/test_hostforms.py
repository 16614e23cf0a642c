"""CPU tier of tests/hostforms.py: the profiles' facts, the expansion reference against two independent constructions, the
reference order against tests/refham.py, the comparisons of test_gpu_hostforms.py against the faults they are there to catch, and
the host-only row cuts (qbh_balanced_row_cuts).  No GPU needed."""
import numpy as np
import pytest

import csrforms as cf
import fastham
import hostforms as hf
import refham
import quantum_basis_amd as q
from quantum_basis_amd import lattices

SMALL = ["mirror_small", "unsorted", "arrow", "scan_edges_1", "scan_edges_2", "scan_edges_2047", "scan_edges_2049", "dict_n_1", "dict_n_257",
         "dict_upper_256", "dict_upper_257_real", "reorder_long_0", "reorder_long_1", "reorder_long_1odd"]
LARGE = ["mirror_lengths", "full_storage", "many_long", "scan_edges_4097", "scan_edges_6145", "dict_n_65536", "dict_upper_65537"]


def _slow_expand(dim, ia, ja, val, sym, r0, r1):
    """The layout of qbh_build.hip entry by entry: host rows in ascending order append their mirrored copies, so these arrive in
    ascending column order by themselves."""
    low = [[] for _ in range(r1 - r0)]
    own = [[] for _ in range(r1 - r0)]
    for r in range(dim):
        for p in range(int(ia[r]), int(ia[r + 1])):
            c, v = int(ja[p]), val[p]
            if r0 <= r < r1:
                own[r - r0].append((c, v))
            if sym and c != r and r0 <= c < r1:
                low[c - r0].append((r, complex(v.real, -v.imag)))
    out_ia, out_ja, out_val = [0], [], []
    for a, b in zip(low, own):
        for c, v in a + b:
            out_ja.append(c)
            out_val.append(v)
        out_ia.append(len(out_ja))
    return np.array(out_ia, dtype=np.int64), np.array(out_ja, dtype=np.int64), np.array(out_val, dtype=np.complex128)


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_expand_entry_by_entry(name):
    dim, ia, ja, val, sym, facts = hf.make(name)
    full = hf.expand(dim, ia, ja, val, sym)
    assert hf.csr_mismatch(full, _slow_expand(dim, ia, ja, val, sym, 0, dim)) is None
    assert full[0][-1] == facts["full_nnz"]
    cuts = [(0, 1), (dim - 1, dim), (dim // 3, dim // 3 + max(1, dim // 5))]
    for r0, r1 in cuts:
        part = hf.expand(dim, ia, ja, val, sym, r0, r1)
        lo, hi = full[0][r0], full[0][r1]
        assert hf.csr_mismatch(part, (full[0][r0:r1 + 1] - lo, full[1][lo:hi], full[2][lo:hi])) is None, (r0, r1)
        if name in ("mirror_small", "unsorted", "scan_edges_2049"):
            assert hf.csr_mismatch(part, _slow_expand(dim, ia, ja, val, sym, r0, r1)) is None, (r0, r1)


@pytest.mark.parametrize("name", SMALL)
def test_expand_equals_the_dense_construction(name):
    """U + U^H - diag as a mask of stored entries and an array of values (a stored zero stays a stored entry): the pattern of every
    row exactly, ascending where the host rows are sorted, the values by bits."""
    dim, ia, ja, val, sym, _ = hf.make(name)
    rows = np.repeat(np.arange(dim), np.diff(ia))
    M = np.zeros((dim, dim), dtype=bool)
    V = np.zeros((dim, dim), dtype=np.complex128)
    M[rows, ja], V[rows, ja] = True, val
    if sym:
        off = rows != ja
        assert not M[ja[off], rows[off]].any()
        M[ja[off], rows[off]], V[ja[off], rows[off]] = True, np.conj(val[off])
    fia, fja, fval = hf.expand(dim, ia, ja, val, sym)
    assert np.array_equal(np.diff(fia), M.sum(axis=1))
    frows = np.repeat(np.arange(dim), np.diff(fia))
    assert M[frows, fja].all() and hf.same_bits(fval, V[frows, fja])
    low = hf.mirrored_lengths(dim, ia, ja) if sym else np.zeros(dim, dtype=np.int64)
    for r in range(dim):
        c = fja[fia[r]:fia[r + 1]]
        assert len(set(c.tolist())) == len(c)
        assert np.all(np.diff(c[:low[r]]) > 0) and np.all(c[:low[r]] < r)
        assert np.array_equal(c[low[r]:], ja[ia[r]:ia[r + 1]])                    # the row's own entries in the order given
        if name != "unsorted":
            assert np.array_equal(c, np.nonzero(M[r])[0])


def test_profiles_hold_their_edges():
    dim, ia, ja, val, sym, f = hf.make("mirror_lengths")
    low = f["low"]
    assert sym == 1 and {int(low[c]) for c in f["rows"].values()} == set(hf.MIRROR_L) and len(f["rows"]) == 44
    assert {0, dim - 1} <= set(f["empty_rows"].tolist()) and len(f["empty_run"]) == 5
    # both sort kernels and both sides of every boundary are reached
    assert {95, 96} <= set(low[low <= hf.K_SHORT_CAP].tolist()) and {97, 255, 256, 257, 600, 1500} <= set(low[low > hf.K_SHORT_CAP].tolist())
    # the sources of a long column come from many upload chunks of 1024 nonzeros
    c = f["rows"][(1500, 40)]
    src = np.nonzero(ja == c)[0]
    assert len(np.unique(src // 1024)) >= 20
    assert dim > 2 * hf.K_SCAN_CHUNK
    _, _, _, _, _, f = hf.make("many_long")
    assert f["n_long"] == 4100 > hf.K_LONG_GRID
    for n in hf.SCAN_N:
        d, sia, _, _, ssym, f = hf.scan_edges(n)
        assert d == n and ssym == 0 and np.array_equal(np.diff(sia), f["lengths"])
    for n in hf.DICT_N:
        for prof in (hf.dict_n(n), hf.dict_upper(n)):
            f = prof[5]
            assert hf.distinct_bits(f["full"][2]) == n and f["n_host"] == n - f["n_pairs"]
            assert hf.distinct_bits(hf.expand(*prof[:5])[2]) == n
    # a real upper-triangle value contributes two patterns once it is mirrored
    assert hf.distinct_bits(np.array([0.5 + 0j])) == 1 and hf.distinct_bits(np.array([0.5 + 0j, np.conj(0.5 + 0j)])) == 2
    assert [hf.code_width(n) for n in (0, 1, 256, 257, 65536, 65537)] == [0, 1, 1, 2, 2, 0]
    for name, (kind, n_sites, n_up, n_dn, lengths) in hf.REORDER.items():
        d, ria, _, _, _, f = hf.make(name)
        assert sorted(np.diff(ria)[list(f["rows"])].tolist()) == sorted(lengths) and {0, d - 1} <= set(f["rows"])


def test_same_bits_sees_what_array_equal_does_not():
    a = np.array([1.0 + 0.0j, 0.0 + 2.0j])
    b = np.array([complex(1.0, -0.0), complex(-0.0, 2.0)])
    assert np.array_equal(a, b) and not hf.same_bits(a, b) and hf.same_bits(a, a.copy())
    assert not hf.same_bits(a, a.astype(np.complex64).astype(np.complex128)[:1])
    assert not hf.same_bits(np.array([1.0]), np.array([np.nextafter(1.0, 2.0)]))


# ---------------------------------------------------------------------------------------------------- reference order --
def _full_of(dim, ia, ja, val):
    return hf.expand(dim, ia, ja, val, 1)


def test_ref_order_reproduces_the_hubbard_order_and_signs_of_refham():
    n, nu, nd = 8, 4, 4
    perm, sign = hf.ref_order(1, n, nu, nd)
    dim, ia, ja, val, basis = refham.hubbard_csr(4, 2, nu, nd)
    ups, dns = refham.bit_patterns(n, nu), refham.bit_patterns(n, nd)
    words = []
    for g in perm:
        up, dn = int(ups[g // len(dns)]), int(dns[g % len(dns)])
        words.append(sum((((up >> s) & 1) | (((dn >> s) & 1) << 1)) << (2 * s) for s in range(n)))
    assert np.array_equal(np.array(words), basis) and sorted(perm.tolist()) == list(range(dim))
    # the generator-order operator, re-expressed, is refham's matrix entry by entry (small integers and U k: the sign flips are exact)
    gd, gia, gja, gval = fastham.to_ref_csr(fastham.hubbard_full(n, nu, nd, lattices.square(4, 2)))
    got = hf.reordered(gd, gia, gja, gval, perm, sign)
    want = _full_of(dim, ia, ja, val)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert (sign == -1).any() and (sign == 1).any()


def test_ref_order_reproduces_the_heisenberg_order_of_refham():
    L = 12
    perm, sign = hf.ref_order(0, L, 0, L // 2)
    dim, ia, ja, val, basis = refham.heisenberg_csr(L, refham.chain_bonds(L), n_dn=L // 2)
    assert np.array_equal(refham.bit_patterns(L, L // 2)[perm], basis) and np.all(sign == 1)
    gd, gia, gja, gval = fastham.to_ref_csr(fastham.heisenberg_full(L, L // 2, lattices.chain(L)))
    got = hf.reordered(gd, gia, gja, gval, perm, sign)
    want = _full_of(dim, ia, ja, val)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_ref_order_with_an_odd_number_of_sites():
    """na = (n_sites + 1) / 2 even sites: the key is sub_b * 4^na + sub_a."""
    perm, sign = hf.ref_order(1, 5, 2, 3)
    basis = refham.electron_basis(5, 2, 3)
    ups, dns = refham.bit_patterns(5, 2), refham.bit_patterns(5, 3)
    words = [sum((((int(ups[g // 10]) >> s) & 1) | (((int(dns[g % 10]) >> s) & 1) << 1)) << (2 * s) for s in range(5)) for g in perm]
    assert np.array_equal(np.array(words), basis)


# ---------------------------------------------------------------------------------------------------------- mutations --
def _copy(t):
    return tuple(a.copy() for a in t)


def test_the_download_comparison_rejects_every_plausible_fault():
    dim, ia, ja, val, sym, f = hf.make("mirror_small")
    ref = hf.expand(dim, ia, ja, val, sym)
    assert hf.csr_mismatch(_copy(ref), ref) is None
    low = f["low"]
    # two mirrored entries of one row swapped (a sort that did not finish, an unstable rank)
    for L in (2, 96, 97, 257):
        r = next(c for (l, _), c in f["rows"].items() if l == L)
        m = _copy(ref)
        p = ref[0][r] + L - 2
        for a in m[1:]:
            a[[p, p + 1]] = a[[p + 1, p]]
        assert "columns differ" in hf.csr_mismatch(m, ref)
        m = _copy(ref)                                   # the values swapped, the columns in place
        m[2][[p, p + 1]] = m[2][[p + 1, p]]
        assert "values differ" in hf.csr_mismatch(m, ref)
    # a conjugation dropped on one mirrored entry
    r = f["rows"][(95, 40)]
    m = _copy(ref)
    p = ref[0][r] + 7
    assert p < ref[0][r] + low[r] and ref[2][p].imag != 0
    m[2][p] = np.conj(m[2][p])
    assert "values differ" in hf.csr_mismatch(m, ref)
    # one value replaced by its last-bit neighbour
    m = _copy(ref)
    m[2][p] = complex(np.nextafter(m[2][p].real, 4.0), m[2][p].imag)
    assert abs(m[2][p] - ref[2][p]) < 1e-15 and "values differ" in hf.csr_mismatch(m, ref)
    # one entry dropped at the end of a row / one row pointer off by one
    m = (ref[0].copy(), ref[1], ref[2])
    m[0][r + 1] -= 1
    assert "row pointers differ" in hf.csr_mismatch(m, ref)


def test_the_download_comparison_sees_a_signed_zero_and_a_pointer_past_a_chunk_seam():
    prof = hf.dict_upper(257, real=True)
    ref = hf.expand(*prof[:5])
    neg = np.nonzero(np.signbit(ref[2].imag))[0]
    assert len(neg) > 100                                # every mirrored real value carries imaginary part -0.0
    m = _copy(ref)
    m[2][neg[3]] = complex(m[2][neg[3]].real, 0.0)
    assert np.array_equal(m[2], ref[2])                  # the comparison the older tests make cannot see it
    assert "values differ by bits" in hf.csr_mismatch(m, ref)
    prof = hf.scan_edges(4097)
    ref = hf.expand(*prof[:5])
    for k in (hf.K_SCAN_CHUNK, hf.K_SCAN_CHUNK + 1, 513, 4097):
        m = (ref[0].copy(), ref[1], ref[2])
        m[0][k] += 1
        assert "row pointers differ (first at %d" % k in hf.csr_mismatch(m, ref)


def test_the_reordered_comparison_rejects_a_dropped_sign():
    dim, ia, ja, val, _, f = hf.make("reorder_long_1")
    perm, sign = hf.ref_order(f["kind"], f["n_sites"], f["n_up"], f["n_dn"])
    ref = hf.reordered(dim, ia, ja, val, perm, sign)
    plain = hf.reordered(dim, ia, ja, val, perm, np.ones(dim, dtype=np.int64))
    assert np.array_equal(plain[0], ref[0]) and np.array_equal(plain[1], ref[1])
    flipped = np.nonzero(np.any(ref[2].view(np.uint64).reshape(-1, 2) != plain[2].view(np.uint64).reshape(-1, 2), axis=1))[0]
    assert len(flipped) > dim                            # the signs matter for this matrix
    rows = np.searchsorted(ref[0], flipped, side="right") - 1
    lens = np.diff(ref[0])[rows]
    for pick in (flipped[np.argmax(lens)], flipped[np.argmin(lens)]):       # one in a long row (the insertion-sort branch), one in a short one
        m = _copy(ref)
        m[2][pick] = -m[2][pick]
        assert "values differ by bits" in hf.csr_mismatch(m, ref)
    assert lens.max() > hf.K_REF_MAX_ROW >= lens.min()
    # and a wrong order: two reference rows exchanged
    p2 = perm.copy()
    p2[[5, 6]] = p2[[6, 5]]
    assert hf.csr_mismatch(hf.reordered(dim, ia, ja, val, p2, sign), ref) is not None


def test_the_row_bound_rejects_a_dropped_or_misplaced_term():
    """The SpMV comparison of test_gpu_hostforms.py (csrforms.worst against csrforms.epilogue): |x_j| >= 0.25 and |a_ij| >= 0.5, so
    one lost term, one term read from the neighbouring column or one missing conjugation is far outside the bound of its row."""
    dim, ia, ja, val, sym, f = hf.make("mirror_small")
    full = hf.expand(dim, ia, ja, val, sym)
    x, y0 = hf.probe_vector(dim, 1), hf.probe_vector(dim, 2)
    assert np.abs(x).min() >= 0.25 and np.abs(x).max() <= 1.0
    ref = hf.spmv_reference(full, x, x, y0)
    y = np.asarray(ref["y"], dtype=np.complex128)
    assert cf.worst(y, ref)[1] <= 1.0
    alpha = hf.TRIPLE[0]
    for (L, k), r in f["rows"].items():
        if L + k == 0:
            continue
        p = full[0][r] + (L + k) // 2
        a, c = full[2][p], full[1][p]
        for delta in (-alpha * a * x[c],                                     # term dropped
                      alpha * a * (x[(c + 1) % dim] - x[c]),                 # neighbouring column read
                      alpha * (np.conj(a) - a) * x[c]):                      # conjugation dropped
            if delta == 0:
                continue
            bad = y.copy()
            bad[r] += delta
            i, ratio, over, _ = cf.worst(bad, ref)
            assert i == r and ratio > 1e6 and over == 1, ((L, k), ratio)


# ------------------------------------------------------------------------------------------------------ row cuts --
@pytest.mark.parametrize("name", ["mirror_lengths", "many_long", "arrow"])
def test_balanced_row_cuts_follow_their_definition(name):
    """Cut p is the first row at which the running nonzero count of the FULL operator reaches p / nranks of the total
    (qbh_build.hip balanced_row_cuts), the count taken from hostforms.expand."""
    dim, ia, ja, val, sym, _ = hf.make(name)
    pre = hf.expand(dim, ia, ja, val, sym)[0]                 # pre[r]: nonzeros of the full rows before r
    total = int(pre[-1])
    for nranks in (1, 2, 3, 7, dim + 3):
        cuts = q.balanced_row_cuts(dim, ia, ja, bool(sym), nranks)
        assert len(cuts) == nranks + 1 and cuts[0] == 0 and cuts[-1] == dim and np.all(np.diff(cuts) >= 0)
        want = np.array([0] + [int(np.searchsorted(pre, total * p // nranks, side="left")) for p in range(1, nranks)] + [dim])
        assert np.array_equal(cuts, np.maximum.accumulate(want)), (name, nranks)
        same = np.nonzero(np.diff(cuts) == 0)[0]
        # a coinciding pair of cuts is an EMPTY shard, which qbh_csr_create_rows refuses: more ranks than rows must give some,
        # and so does the arrow, whose first row alone holds more than 2 / 7 of the operator
        if nranks > dim:
            assert len(same) >= nranks - dim
        elif name == "arrow" and nranks == 7:
            assert cuts[1] == cuts[2] == 1 and len(same) == 1
        else:
            assert len(same) == 0, (name, nranks, same)
