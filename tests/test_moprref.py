"""Pins tests/moprref.py, the host reference of the full-space operator-times-vector step, and the comparison the GPU tests of
tests/test_gpu_moprforms.py share: every function against dense operators built by Kronecker products on the whole product
space and restricted to the sectors (the builders of test_gpu_mopr.py for spins and fermions, one written here for d levels),
the enumeration against counting, and compare() against a float64 re-evaluation (accepted) and seven injected faults (each
rejected)."""
import functools
import math

import numpy as np
import pytest

import moprref
from test_gpu_mopr import _dense_fermion_ops, _dense_spin_ops

LD, CLD = np.longdouble, np.clongdouble
EPS = np.finfo(LD).eps / 2                               # unit roundoff of the long double the reference accumulates in


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=n) + 1j * rng.normal(size=n)) * 1.3).astype(np.complex128)


def _agree(want, scale, k, dense_rows, x):
    """the reference against a dense longdouble product (dense_rows is clongdouble: products of the elementary matrices are
    exact in double, weights and sums are not); both sides sum the same <= k_i products, the dense one zeros besides"""
    ref = dense_rows.astype(CLD) @ x.astype(CLD)
    n = dense_rows.shape[1]
    tol = 8 * (n + 4) * EPS * np.maximum(scale, np.abs(dense_rows) @ np.abs(x.astype(CLD)))
    assert np.all(np.abs(want - ref) <= tol)
    assert np.all(want[k == 0] == 0) and np.all(ref[k == 0] == 0)
    # scale is sum |entry| |x|: the dense operator has the merged entries, so it can only be smaller
    assert np.all(np.abs(dense_rows) @ np.abs(x.astype(CLD)) <= scale * (1 + 64 * EPS))


# ---------------------------------------------------------------------------------------------- enumeration --
def test_enumeration_counts_order_and_charge():
    for n, d in ((1, 2), (6, 2), (9, 2), (5, 3), (4, 4), (3, 5), (3, 8)):
        seen = 0
        for total in range(n * (d - 1) + 1):
            w = moprref.words(n, d, total)
            brute = [v for v in range(d ** n) if sum((v // d ** s) % d for s in range(n)) == total]
            assert w.dtype == np.uint64 and w.tolist() == brute, (n, d, total)
            seen += len(w)
        assert seen == d ** n
        assert len(moprref.words(n, d, -1)) == 0 and len(moprref.words(n, d, n * (d - 1) + 1)) == 0
    # the sizes the GPU suite relies on, bit 63 and the mirrored (more than half filled) branch
    assert len(moprref.patterns(22, 11)) == math.comb(22, 11) == 705432
    assert len(moprref.patterns(40, 5)) == math.comb(40, 5) == 658008
    assert len(moprref.patterns(34, 32)) == 561 and len(moprref.patterns(34, 31)) == 5984
    p = moprref.patterns(64, 2)
    assert len(p) == 2016 and int(p[-1]) == 3 << 62 and int(p[0]) == 3
    assert moprref.patterns(64, 64).tolist() == [2 ** 64 - 1] and moprref.patterns(64, 63).tolist()[0] == 2 ** 63 - 1
    assert len(moprref.words(14, 3, 14)) == 616227
    assert moprref.words(32, 4, 96).tolist() == [4 ** 32 - 1] and moprref.words(21, 8, 147).tolist() == [8 ** 21 - 1]
    for w in (moprref.patterns(40, 5), moprref.words(14, 3, 15), moprref.words(21, 8, 3), moprref.words(32, 4, 94), moprref.patterns(34, 31)):
        assert np.all(w[1:] > w[:-1])
    assert all(sum((v // 8 ** s) % 8 for s in range(21)) == 144 for v in moprref.words(21, 8, 144).tolist())


# ------------------------------------------------------------------------------------- against dense operators --
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_spin_against_dense_operators(n):
    ops = _dense_spin_ops(n)
    rng = np.random.default_rng(n)
    coef = rng.normal(size=n) + 1j * rng.normal(size=n)
    for n_dn in range(n + 1):
        old = moprref.patterns(n, n_dn).astype(np.int64)
        x = _rand(len(old), 10 * n + n_dn)
        for kind, name in ((0, "Sz"), (-1, "S-"), (+1, "S+")):
            if not 0 <= n_dn - kind <= n:
                continue
            new = moprref.patterns(n, n_dn - kind).astype(np.int64)
            dense = sum(CLD(coef[s]) * ops[(name, s)].astype(CLD) for s in range(n))[np.ix_(new, old)]
            want, scale, k = moprref.spin(n, n_dn, kind, coef, x)
            assert len(want) == math.comb(n, n_dn - kind)
            _agree(want, scale, k, dense, x)
            assert np.all(k == (n if kind == 0 else n_dn - kind if kind < 0 else n - (n_dn - kind)))


SPIN_NAMES = {"Sz": 0, "S+": 1, "S-": 2}
FERMI_NAMES = {"n": 0, "c+": 1, "c": 2}


def _spin_products(n, tail):
    named = [(0.7 + 0.2j, [("S+", 2), ("S-", 5), ("Sz", 1)] + tail), (-1.3j, [("S-", 0), ("S+", n - 1)] + tail), (0.4, [("Sz", 3), ("Sz", 3)] + tail),
             (1.1, tail + [("Sz", n - 2)]), (0.25 - 0.5j, [("S+", 4), ("S-", 4), ("S-", 1), ("S+", 0)] + tail), (0.6j, [("S+", 3), ("S+", 3), ("S-", 3), ("S-", 0)] + tail)]
    if not tail:
        named.append((-0.9 + 0.3j, []))                                    # the identity: a product of no factor
    return named


@pytest.mark.parametrize("delta", [0, 1, -1])
def test_spin_products_against_dense_operators(delta):
    n, nd = 7, 3
    ops = _dense_spin_ops(n)
    tail = {0: [], 1: [("S-", 6)], -1: [("S+", 2)]}[delta]
    named = _spin_products(n, tail)
    dense = sum(CLD(c) * np.linalg.multi_dot([ops[f] for f in fs] + [np.eye(1 << n), np.eye(1 << n)]).astype(CLD) for c, fs in named)
    old, new = moprref.patterns(n, nd).astype(np.int64), moprref.patterns(n, nd + delta).astype(np.int64)
    x = _rand(len(old), 3 + delta)
    want, scale, k = moprref.terms(0, n, nd, 0, [(c, [(SPIN_NAMES[nm], s, 0) for nm, s in fs]) for c, fs in named], x)
    _agree(want, scale, k, dense[np.ix_(new, old)], x)
    assert k.max() >= 3


def _fermion_cases(n):
    return {
        "number_conserving": ([(0.8, [("c+", 1, 0), ("c", n - 1, 0)]), (-0.6j, [("c+", n - 1, 1), ("c", 0, 1)]), (1.5, [("n", 2, 0), ("n", 2, 1)]),
                               (0.3 + 0.1j, [("c+", 0, 0), ("c+", 1, 1), ("c", n - 1, 1), ("c", 2, 0)]), (2.0, [("c", 1, 0), ("c+", 1, 0)]),
                               (0.7, [("c+", 1, 0), ("c+", 1, 0), ("c", 1, 0), ("c", 0, 0)])], (0, 0)),
        "spin_flip": ([(1.0 + 0.1 * s, [("c+", s, 0), ("c", s, 1)]) for s in range(n)] + [(0.5j, [("c+", 0, 0), ("c", n - 1, 1), ("n", 2, 1)])], (1, -1)),
        "remove_up": ([(np.exp(2j * np.pi * s / n), [("c", s, 0)]) for s in range(n)], (-1, 0)),
        "add_dn": ([(np.exp(2j * np.pi * s / n), [("c+", s, 1)]) for s in range(n)], (0, 1)),
        "add_pair": ([(1.0 + 0.5 * s, [("c+", s, 0), ("c+", s, 1)]) for s in range(n)], (1, 1)),
    }


@functools.lru_cache(maxsize=None)
def _fermi_ops(n):
    return _dense_fermion_ops(2 * n)


def _fermi_index(n, nu, nd):
    return np.array([int(u) | (int(d) << n) for u in moprref.patterns(n, nu) for d in moprref.patterns(n, nd)], dtype=np.int64)


@pytest.mark.parametrize("case", ["number_conserving", "spin_flip", "remove_up", "add_dn", "add_pair"])
@pytest.mark.parametrize("shape", [(4, 2, 1), (4, 1, 3), (4, 0, 2), (4, 4, 1), (3, 1, 1)])
def test_fermion_products_against_jordan_wigner(shape, case):
    n, nu, nd = shape
    ops = _fermi_ops(n)
    named, (dnu, dnd) = _fermion_cases(n)[case]
    if not (0 <= nu + dnu <= n and 0 <= nd + dnd <= n):
        return                                                             # no such target sector
    eye = np.eye(1 << (2 * n))
    dense = sum(CLD(c) * np.linalg.multi_dot([ops[(nm, s + sp * n)] for nm, s, sp in fs] + [eye, eye]).astype(CLD) for c, fs in named)
    old, new = _fermi_index(n, nu, nd), _fermi_index(n, nu + dnu, nd + dnd)
    x = _rand(len(old), 7 + nu)
    want, scale, k = moprref.terms(1, n, nu, nd, [(c, [(FERMI_NAMES[nm], s, sp) for nm, s, sp in fs]) for c, fs in named], x)
    assert len(want) == len(new)
    _agree(want, scale, k, dense[np.ix_(new, old)], x)


@pytest.mark.parametrize("shape", [(4, 2, 1), (4, 0, 3), (4, 4, 1), (2, 1, 1)])
def test_onebody_against_jordan_wigner(shape):
    n, nu, nd = shape
    ops = _fermi_ops(n)
    rng = np.random.default_rng(n + nu)
    terms = [(a, b, sp, complex(rng.normal(), rng.normal())) for a in range(n) for b in range(n) for sp in (0, 1)]
    terms.append(terms[3])                                                 # one term listed twice
    dense = sum(CLD(w) * (ops[("c+", a + sp * n)] @ ops[("c", b + sp * n)]).astype(CLD) for a, b, sp, w in terms)
    idx = _fermi_index(n, nu, nd)
    x = _rand(len(idx), 1)
    want, scale, k = moprref.onebody(n, nu, nd, terms, x)
    _agree(want, scale, k, dense[np.ix_(idx, idx)], x)


def _dense_qudit(n, d, coef, loc):
    """sum_s coef_s O_s on the d^n product space, state index sum_s l_s d^s (site n-1 most significant); the Kronecker products
    only copy entries, the weighted sum is formed in longdouble like everything it is compared with"""
    full = np.zeros((d ** n, d ** n), dtype=CLD)
    for s in range(n):
        m = np.array([[1.0 + 0j]])
        for t in reversed(range(n)):
            m = np.kron(m, loc if t == s else np.eye(d))
        full += CLD(coef[s]) * m.astype(CLD)
    return full


def local_matrix(d, dq, seed):
    """random complex entries on the dq diagonal (<l'|O|l>, l' = l + dq), one of them exactly zero where there are two"""
    rng = np.random.default_rng(seed)
    loc = np.zeros((d, d), dtype=np.complex128)
    ls = [l for l in range(d) if 0 <= l + dq < d]
    for l in ls:
        loc[l + dq, l] = complex(rng.normal(), rng.normal())
    if len(ls) >= 2:
        loc[ls[len(ls) // 2] + dq, ls[len(ls) // 2]] = 0.0
    return loc


@pytest.mark.parametrize("shape", [(2, 6), (3, 6), (4, 5), (5, 4), (8, 3)])
def test_qudit_against_dense_operators(shape):
    d, n = shape
    assert d ** n <= 4096
    rng = np.random.default_rng(d)
    coef = rng.normal(size=n) + 1j * rng.normal(size=n)
    charge = np.array([sum((v // d ** s) % d for s in range(n)) for v in range(d ** n)])
    top = n * (d - 1)
    for dq in sorted({0, 1, -1, 2, -2, d - 1, 1 - d} & set(range(1 - d, d))):
        loc = local_matrix(d, dq, 50 + dq)
        dense = _dense_qudit(n, d, coef, loc)
        for total in sorted({0, 1, top // 2, top - 1, top}):
            if not 0 <= total + dq <= top:
                continue
            old, new = np.flatnonzero(charge == total), np.flatnonzero(charge == total + dq)
            assert moprref.words(n, d, total).tolist() == old.tolist()
            x = _rand(len(old), total)
            want, scale, k = moprref.qudit(n, d, total, dq, coef, loc.ravel(), x)
            assert len(want) == len(new)
            _agree(want, scale, k, dense[np.ix_(new, old)], x)


# --------------------------------------------------------------------------------------- the comparison function --
def _spin_flip_terms(n):
    return [(0.6 + 0.1 * s - 0.2j, [(1, s, 0), (2, s, 1)]) for s in range(n)]


@functools.lru_cache(maxsize=None)
def _fault_case():
    """The named shape of the injected faults: S^+_q = sum_s c^dag_{s,up} c_{s,down} from (9, 3, 5) to (9, 4, 4), 84 x 126 ->
    126 x 126 rows.  Term s reaches the target rows with an up and no down electron on site s, so k_i runs from 0 (the up
    electrons sit on the sites of the down electrons: the row must vanish exactly) to 4."""
    n, nu, nd = 9, 3, 5
    x = _rand(math.comb(n, nu) * math.comb(n, nd), 99)
    tm = _spin_flip_terms(n)
    return n, nu, nd, tm, x, moprref.terms(1, n, nu, nd, tm, x), list(moprref.terms_contribs(1, n, nu, nd, tm))


def _float64_result():
    n, nu, nd, tm, x, _, _ = _fault_case()
    return moprref.terms(1, n, nu, nd, tm, x, dtype=np.complex128)[0]


def test_compare_accepts_a_float64_reevaluation():
    n, nu, nd, tm, x, (want, scale, k), _ = _fault_case()
    got = _float64_result()
    assert got.dtype == np.complex128
    v = moprref.compare(got, want, scale, k)
    assert v.ok and v.worst <= 1.0 and len(v.bad) == 0
    assert k.min() == 0 and k.max() >= 3                   # the shape has rows that must vanish and rows with several terms
    # ... and of every function, at a shape with more than one term per row
    rng = np.random.default_rng(4)
    coef = rng.normal(size=12) + 1j * rng.normal(size=12)
    for kind in (0, -1, 1):
        xs = _rand(math.comb(12, 6), kind + 2)
        w, s, kk = moprref.spin(12, 6, kind, coef, xs)
        v = moprref.compare(moprref.spin(12, 6, kind, coef, xs, dtype=np.complex128)[0], w, s, kk)
        assert v.ok and 0 < v.worst <= 1.0
    ob = [(a, b, sp, complex(rng.normal(), rng.normal())) for a in range(6) for b in range(6) for sp in (0, 1)]
    xs = _rand(20 * 15, 8)
    w, s, kk = moprref.onebody(6, 3, 2, ob, xs)
    assert moprref.compare(moprref.onebody(6, 3, 2, ob, xs, dtype=np.complex128)[0], w, s, kk).ok
    loc = local_matrix(4, -1, 2)
    xs = _rand(len(moprref.words(6, 4, 9)), 9)
    w, s, kk = moprref.qudit(6, 4, 9, -1, coef[:6], loc.ravel(), xs)
    assert moprref.compare(moprref.qudit(6, 4, 9, -1, coef[:6], loc.ravel(), xs, dtype=np.complex128)[0], w, s, kk).ok


def _one_contribution(min_terms=2):
    """(term, row, source, weight) of one contribution to a row that at least min_terms terms reach"""
    _, _, _, _, _, (_, _, k), contribs = _fault_case()
    for t, (rows, cols, weight) in enumerate(contribs):
        for m in range(len(rows)):
            if k[rows[m]] >= min_terms:
                return t, int(rows[m]), int(cols[m]), complex(weight[m])
    raise AssertionError("no such row")


def _fault_fermion_sign(got, want, scale, k, x):
    t, i, j, w = _one_contribution()
    got[i] -= 2 * w * x[j]
    return [i]


def _fault_source_off_by_one(got, want, scale, k, x):
    t, i, j, w = _one_contribution()
    j2 = j + 1 if j + 1 < len(x) else j - 1
    got[i] += w * (x[j2] - x[j])
    return [i]


def _fault_term_dropped(got, want, scale, k, x):
    t, i, j, w = _one_contribution()
    got[i] -= w * x[j]
    return [i]


def _fault_last_row_sentinel(got, want, scale, k, x):
    got[-1] = complex(moprref.SENTINEL, moprref.SENTINEL)
    return [len(got) - 1]


def _fault_exact_zero(got, want, scale, k, x):
    i = int(np.flatnonzero(k == 0)[0])
    assert want[i] == 0 and scale[i] == 0
    got[i] = 1e-300
    return [i]


def _fault_rows_swapped(got, want, scale, k, x):
    i = int(np.flatnonzero(k >= 2)[0])
    j = int(np.flatnonzero((k >= 2) & (np.arange(len(k)) > i))[0])
    got[i], got[j] = got[j], got[i]
    return [i, j]


FAULTS = [_fault_fermion_sign, _fault_source_off_by_one, _fault_term_dropped, _fault_last_row_sentinel, _fault_exact_zero,
          _fault_rows_swapped]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f.__name__[7:])
def test_compare_rejects_an_injected_fault(fault):
    n, nu, nd, tm, x, (want, scale, k), _ = _fault_case()
    got = _float64_result().copy()
    assert moprref.compare(got, want, scale, k).ok
    rows = fault(got, want, scale, k, x)
    v = moprref.compare(got, want, scale, k)
    assert not v.ok and v.worst > 1.0
    assert v.bad.tolist() == sorted(rows)                  # exactly the rows touched, no other


def test_compare_rejects_a_relative_error_of_1e_12_on_a_row_of_eight_terms():
    """S^-_q on 16 sites into n_dn = 8: every target row gathers k_i = 8 terms.  bound_i = 4 * 12 * 2^-53 scale_i = 5.3e-15
    scale_i, so a relative error of 1e-12 is caught wherever |want_i| > 5.3e-3 scale_i; the row is chosen with |want_i| >=
    0.1 scale_i (no cancellation), as most rows of a random vector are."""
    rng = np.random.default_rng(12)
    coef = rng.normal(size=16) + 1j * rng.normal(size=16)
    x = _rand(math.comb(16, 7), 16)
    want, scale, k = moprref.spin(16, 7, -1, coef, x)
    got = moprref.spin(16, 7, -1, coef, x, dtype=np.complex128)[0]
    assert np.all(k == 8) and moprref.compare(got, want, scale, k).ok
    i = int(np.flatnonzero(np.abs(want) >= 0.1 * scale)[0])
    got[i] *= 1 + 1e-12
    v = moprref.compare(got, want, scale, k)
    assert not v.ok and v.bad.tolist() == [i]


def test_compare_rejects_nan_a_wrong_length_and_a_negative_zero_is_a_zero():
    n, nu, nd, tm, x, (want, scale, k), _ = _fault_case()
    got = _float64_result().copy()
    i = int(np.flatnonzero(k == 0)[0])
    got[i] = complex(-0.0, 0.0)
    assert moprref.compare(got, want, scale, k).ok
    got[3] = complex(np.nan, 0.0)
    v = moprref.compare(got, want, scale, k)
    assert not v.ok and v.bad.tolist() == [3] and v.worst == float("inf")
    assert not moprref.compare(got[:-1], want, scale, k).ok
