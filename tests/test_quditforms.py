"""CPU checks of tests/quditforms.py, the reference of tests/test_gpu_quditforms.py: the enumeration, rank and unrank against itertools
for every d = 2 .. 8; `assemble` against a dense operator built with np.kron and projected on the sector, and against the host
assembly of tests/test_gpu_qudit.py; the mirror's arithmetic; every case's edge on the reference alone; and the comparison
rejecting single injected faults."""
import itertools

import numpy as np
import pytest

import quditforms as qf
from test_gpu_qudit import host_sector_csr

SMALL = [(2, 10), (3, 7), (4, 6), (5, 5), (6, 5), (7, 4), (8, 4)]


def _brute(n, d, total):
    ws = [w for w in itertools.product(range(d), repeat=n) if sum(w) == total]
    return sorted(ws, key=lambda w: sum(l * d ** s for s, l in enumerate(w)))


@pytest.mark.parametrize("d,n", SMALL)
def test_words_rank_unrank_against_enumeration(d, n):
    for total in range(n * (d - 1) + 1):
        want = _brute(n, d, total)
        lv, keys = qf.words(n, d, total)
        assert [tuple(int(l) for l in w) for w in lv] == want
        cnt = qf.Counter(n, d, total)
        assert cnt.dim == len(want) == qf.qudit_dim(n, d, total)
        assert np.array_equal(qf.unpack(keys, n, d), lv)
        step = max(1, len(want) // 40)
        for r in list(range(0, len(want), step)) + [len(want) - 1]:
            assert cnt.rank(want[r]) == r and tuple(cnt.unrank(r)) == want[r]
        assert np.array_equal(cnt.rank_many(lv), np.arange(len(want), dtype=np.uint64))


def test_rank_of_sectors_too_large_to_enumerate():
    """Python-integer counts: the last word of (2, 64, 32) and rows of the spin-1 chain of 24 sites round-trip."""
    cnt = qf.Counter(64, 2, 32)
    assert cnt.dim == 1832624140942590534 < 1 << 62
    assert cnt.unrank(cnt.dim - 1) == [0] * 32 + [1] * 32 and cnt.unrank(0) == [1] * 32 + [0] * 32
    c3 = qf.Counter(24, 3, 24)
    assert c3.dim == 27948336381
    for r in (0, 27_000_000_000, 27_000_004_095, c3.dim - 1):
        w = c3.unrank(r)
        assert c3.rank(w) == r and int(c3.rank_many(np.array([w]))[0]) == r
    r0, r1 = qf._alt_rows()
    assert qf.Counter(32, 2, 16).unrank(r0 + 2048) == qf.ALTERNATING and 0 < r0 and r1 < 601080390


def _dense(n, d, pairs, singles):
    """sum of the pair and single-site operators on the full space, index = sum_s l_s d^s, from np.kron"""
    N = d ** n
    H = np.zeros((N, N), dtype=np.complex128)

    def embed(op, sites):
        k = len(sites)
        rest = [s for s in range(n) if s not in sites]
        T = np.kron(op, np.eye(d ** (n - k))).reshape([d] * (2 * n))         # axes: (sites, rest) out, (sites, rest) in
        order = list(sites) + rest
        pos = [order.index(s) for s in range(n - 1, -1, -1)]                   # site n-1 most significant
        return T.transpose(pos + [n + p for p in pos]).reshape(N, N)

    for (i, j, M) in pairs:
        H += embed(np.asarray(M).reshape(d * d, d * d), [i, j])
    for (s, dg) in singles:
        H += embed(np.diag(np.asarray(dg, dtype=np.complex128)), [s])
    return H


@pytest.mark.parametrize("d,n", [(2, 8), (3, 6), (4, 5), (5, 4), (6, 4), (7, 3), (8, 3)])
def test_assemble_against_dense_kron_and_host_sector_csr(d, n):
    sites = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pairs, singles = qf.draw_operator(100 + d, n, d, sites, real=False, p_zero=0.2)
    pairs.append((pairs[0][1], pairs[0][0], qf.draw_pair(np.random.default_rng(d), d)))       # a repeat, the other way round
    H = _dense(n, d, pairs, singles)
    assert np.abs(H - H.conj().T).max() < 1e-14
    for total in sorted({1, n * (d - 1) // 2, n * (d - 1) - 1}):
        lv, keys = qf.words(n, d, total)
        idx = (lv.astype(np.int64) * d ** np.arange(n)).sum(axis=1)
        want = H[np.ix_(idx, idx)]
        asm = qf.assemble(n, d, total, pairs, singles)
        got = np.zeros_like(want)
        rows = np.repeat(np.arange(asm.nrows), np.diff(asm.ia))
        got[rows, asm.ja] = asm.val
        assert np.abs(got - want).max() < 1e-13
        assert np.array_equal(got != 0, (want != 0) | np.eye(len(idx), dtype=bool))
        _, Hs = host_sector_csr(n, d, total, pairs, singles)
        assert np.abs(Hs.toarray() - got).max() < 1e-13
        # a shard assembled through unrank / rank_many equals the rows of the whole
        r0, r1 = len(idx) // 3, len(idx) // 3 + min(9, len(idx) - len(idx) // 3)
        sh = qf.assemble(n, d, total, pairs, singles, rows=(r0, r1))
        assert np.array_equal(sh.ja, asm.ja[asm.ia[r0]:asm.ia[r1]]) and np.array_equal(sh.val, asm.val[asm.ia[r0]:asm.ia[r1]])
        assert np.array_equal(sh.terms, asm.terms[r0:r1])
        # the unmerged terms add up to the merged entries
        assert np.array_equal(np.diff(asm.t_ia), asm.terms)


def test_mirror_arithmetic():
    assert qf.gen_fill_lds(240, 64, 64) == 155648 <= qf.LDS_DEVICE
    assert qf.gen_fill_lds(240, 32, 17) == 4352 + 122880
    lay = qf.layout_of("d8_n12_q5_15cls")
    # (12 x 6 + 12 x 8) x 8 + 112 slots x 8 + (64 + 15 x 7 x 64) x 20 + 15 x 64 x 8
    assert lay.lds_bytes(True) == 1344 + 896 + 6784 * 20 + 7680 and lay.lds_bytes(False) == 1344 + 896
    assert lay.bytes_matrix == 576 + 15 * 4 + 15 * 64 * 4 + 224 * 4 + 768 + 15 * 64 * 8 + 6784 * 20


def test_every_case_has_the_edge_it_claims():
    seen = set()
    for name, c in qf.CASES.items():
        asm, lay = qf.reference_of(name), qf.layout_of(name)
        n, d, total = c["n"], c["d"], c["total"]
        assert asm.dim == c["dim"] == qf.qudit_dim(n, d, total), name
        assert lay.values_real == c["real"], name
        lens = np.diff(asm.ia)
        for e in c["edge"]:
            seen.add(e)
            if e == "bit63":
                assert np.any(asm.keys >> np.uint64(63)), name
            elif e == "nb64":
                assert n * qf.bits_per_level(d) == 64 and any(j == n - 1 for (_, j), _ in asm.merged), name
            elif e == "w64":
                assert n * qf.bits_per_level(d) == 64 and int(asm.keys.max()) >> 32, name
            elif e == "top_full":
                assert np.all(asm.levels[:, n - 2:] >= d - 3) and np.any(asm.levels[:, n - 1] == d - 1), name
            elif e == "bits3":
                assert qf.bits_per_level(d) == 3 and (n < 21 or int(asm.keys.max()) >> 60), name     # 21 sites: 63-bit words
            elif e == "blocks":
                assert asm.nrows > 16 * qf.MF_BLOCK, name                  # several workgroups of every kernel
            elif e == "max_row240":
                assert lay.max_row == 240 == qf.MAX_ROW and qf.gen_fill_lds(lay.max_row, n, total + 1) <= qf.LDS_DEVICE, name
            elif e == "max_row239":
                assert lay.max_row == 239 and set(lay.maxk) == {7}, name
            elif e == "row240":
                mid = asm.nrows // 2
                assert lens[mid] == 240 == lens.max() and (lens >= 200).sum() >= 32 and lens.min() > 100, name       # 51 rows of 200 and more; none short
                assert asm.levels[mid].tolist() == qf.ALTERNATING
            elif e == "tlds_on":
                assert lay.tables_lds == 1, name
            elif e == "tlds_off":
                assert lay.tables_lds == 0, name
            elif e == "boundary":
                assert abs(lay.lds_bytes(True) - qf.LDS_CAP) < max(lay.lds_per_class), name
            elif e == "dim1":
                assert asm.dim == 1 and lens.tolist() == [1], name
            elif e == "grid_stride":
                assert asm.dim > 3 * qf.GRID_ROWS and asm.dim % qf.MF_BLOCK != 0, name
            elif e == "maxk0":
                assert 0 in lay.maxk and lay.raw_slots == sum(max(1, lay.maxk[k]) for k in lay.cls), name
            elif e == "diag_operator":
                assert lay.maxk == [0] and lens.max() == 1, name
            elif e == "shared":
                assert lay.n_cls < lay.n_pairs and lay.cls.count(0) == 3, name
            elif e == "cancelled":
                M = dict(asm.merged)[(1, 3)]
                r, cc = qf.CANCEL_AT
                assert M[r, cc] == 0 and M[cc, r] == 0, name
                once = qf.assemble(n, d, total, qf.operator(name)[0][:-1], qf.operator(name)[1])
                assert dict(once.merged)[(1, 3)][r, cc] != 0 and once.ia[-1] > asm.ia[-1], name
            elif e == "no_single":
                assert lay.has_single == 0, name
            else:
                raise KeyError(e)
        if "no_single" not in c["edge"]:
            assert lay.has_single == 1, name
        if lay.max_row <= qf.MAX_ROW and c["gen"]:
            assert lens.max() <= lay.max_row
    assert any(qf.layout_of(n).padding > 0 for n in qf.CASES) and any(qf.layout_of(n).padding == 0 for n in qf.CASES)
    for a, b in qf.BOUNDARY_PAIRS:
        la, lb = qf.layout_of(a), qf.layout_of(b)
        assert la.n_cls + 1 == lb.n_cls and la.tables_lds == 1 and lb.tables_lds == 0 and la.lds_bytes(True) <= qf.LDS_CAP < lb.lds_bytes(True)
    inst = set().union(*(qf.instances(n) for n in qf.CASES))
    assert inst == {(False, False), (False, True), (True, False), (True, True)}
    assert seen >= {"bit63", "nb64", "max_row240", "max_row239", "row240", "tlds_on", "tlds_off", "boundary", "dim1", "grid_stride", "maxk0",
                    "shared", "cancelled", "no_single", "top_full", "bits3", "blocks"}


# ---------------------------------------------------------------------------------------------------- injected faults --
def _good(asm):
    val = asm.val.copy()
    val[asm.is_diag] = asm.diag.astype(np.float64)
    return asm.ia, asm.ja, val


def _rejects(asm, got):
    with pytest.raises(AssertionError):
        qf.assert_same_csr(got, asm)


@pytest.mark.parametrize("name", ["d3_n32_q62", "d8_n21_q145", "slots_cancelled"])
def test_the_comparison_rejects_single_faults(name):
    asm = qf.reference_of(name)
    assert qf.assert_same_csr(_good(asm), asm) <= 1.0
    for how in ("dropped", "flipped", "column", "diagonal_term"):
        _rejects(asm, qf.tampered(asm, how))
    ia, ja, val = _good(asm)
    k = np.nonzero(~asm.is_diag)[0][3]
    val = val.copy()
    val[k] = complex(np.nextafter(val[k].real, 2.0), val[k].imag)             # one bit of one off-diagonal value
    _rejects(asm, (ia, ja, val))
    x = qf.probe_vector(asm.dim, 1)
    sums = qf.row_sums(asm, x)
    ref = qf.reference(asm, sums, x, x, 1.0, 0.0, 0.0)
    assert qf.worst(ref["y"].astype(np.complex128), ref)[1] <= 1.0
    for how in ("dropped", "flipped", "column"):                              # the applied row: far outside its bound
        tia, tja, tval = qf.tampered(asm, how)
        y = np.array([np.dot(tval[tia[r]:tia[r + 1]], x[tja[tia[r]:tia[r + 1]]]) for r in range(asm.nrows)])
        assert qf.worst(y, ref)[1] > 1e6, how


def test_transposition_not_applied_is_rejected():
    name = "d6_n21_q3"
    c, asm = qf.CASES[name], qf.reference_of(name)
    pairs, sg = qf.operator(name)
    assert any(i > j for i, j, _ in pairs)
    wrong = qf.assemble(c["n"], c["d"], c["total"], [(min(i, j), max(i, j), M) for i, j, M in pairs], sg)
    with pytest.raises(AssertionError):
        qf.assert_same_csr(_good(wrong), asm)


def test_wrong_field_width_is_rejected():
    """levels read with 2-bit fields from words packed with 3: the diagonal a kernel would form from them"""
    name = "d8_n21_q145"
    c, asm = qf.CASES[name], qf.reference_of(name)
    lv = np.minimum(qf.unpack(asm.keys, c["n"], c["d"], bits=2), c["d"] - 1).astype(np.int64)
    assert not np.array_equal(lv, asm.levels)
    dg = sum(asm.sdiag[s][lv[:, s]] for s in range(c["n"]))
    for (i, j), M in asm.merged:
        dg = dg + M.real[lv[:, i] * c["d"] + lv[:, j], lv[:, i] * c["d"] + lv[:, j]]
    ia, ja, val = _good(asm)
    val = val.copy()
    val[asm.is_diag] = dg
    _rejects(asm, (ia, ja, val))


def test_words_compared_as_signed_are_rejected():
    """(2, 64, 63): every word but one has bit 63 set; ordered as int64 the one without it moves from the front to the back."""
    asm = qf.reference_of("d2_n64_q63")
    order = np.argsort(asm.keys.view(np.int64), kind="stable")
    assert not np.array_equal(order, np.arange(asm.nrows))
    pos = np.empty_like(order)
    pos[order] = np.arange(len(order))
    ia, ja, val = _good(asm)
    rows = np.repeat(np.arange(asm.nrows), np.diff(ia))
    got = qf.gf._csr_from_coo(asm.nrows, pos[rows], pos[ja], val)
    _rejects(asm, got)
    # the unsigned search finds every word; a signed one would look for the last words before the first
    assert np.array_equal(np.searchsorted(asm.keys, asm.keys), np.arange(asm.nrows))
