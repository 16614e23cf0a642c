"""tests/quditcorrref.py (the host reference of qbh_corr_qudit_dev) pinned against dense np.kron operators restricted to the
sector, for every total of (d, n) = (2,4), (3,4), (4,3), (5,3), (8,2); and the faults the comparison must reject."""
import functools

import numpy as np
import pytest

import quditcorrref as ref
import quditforms as qf

SHAPES = [(2, 4), (3, 4), (4, 3), (5, 3), (8, 2)]


def _tables(d, seed):
    rng = np.random.default_rng(seed)
    return dict(diag=rng.uniform(-1.5, 1.5, size=(2, d)), string=(rng.uniform(-1.5, 1.5, size=d), rng.uniform(-1.2, 1.2, size=d)),
                lower=np.append(0.0, rng.uniform(0.3, 1.7, size=d - 1)))


def _site_op(n, d, site, M):
    """M at `site` in the full d^n space, index = sum_s l_s d^s (site 0 least significant)"""
    out = np.ones((1, 1))
    for s in range(n - 1, -1, -1):
        out = np.kron(out, M if s == site else np.eye(d))
    return out


def _dense(n, d, total, psi, tabs):
    levels, _ = qf.words(n, d, total)
    pos = (levels.astype(np.int64) * (d ** np.arange(n))[None, :]).sum(axis=1)
    full = np.zeros(d ** n, dtype=np.complex128)
    full[pos] = psi
    ev = lambda O: np.vdot(full, O @ full)                                        # noqa: E731
    f, (h, g), A = tabs["diag"], tabs["string"], ref.lowering(tabs["lower"])
    op = functools.partial(_site_op, n, d)
    out = {"norm2": np.vdot(full, full).real, "pop": np.zeros((n, d)), "dd": np.zeros((2, 2, n, n)), "str": np.zeros((n, n)),
           "aa": np.zeros((n, n), dtype=np.complex128)}
    for s in range(n):
        for l in range(d):
            e = np.zeros(d)
            e[l] = 1.0
            out["pop"][s, l] = ev(op(s, np.diag(e))).real
    for i in range(n):
        for j in range(n):
            for a in range(2):
                for b in range(2):
                    out["dd"][a, b, i, j] = ev(op(i, np.diag(f[a])) @ op(j, np.diag(f[b]))).real
            lo, hi = min(i, j), max(i, j)
            S = op(lo, np.diag(h)) @ op(hi, np.diag(h))
            for k in range(lo + 1, hi):
                S = S @ op(k, np.diag(g))
            out["str"][i, j] = ev(S).real
            out["aa"][i, j] = ev(op(i, A) @ op(j, A.T))
    return out


@functools.lru_cache(maxsize=None)
def _case(d, n, total):
    dim = len(qf.words(n, d, total)[1])
    rng = np.random.default_rng(1000 * d + 100 * n + total)
    psi = (rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 1.3
    tabs = _tables(d, 17 * d + n)
    return psi, tabs, ref.correlations(n, d, total, psi, **tabs)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_n%d" % s)
def test_reference_against_kronecker_operators_in_every_sector(shape):
    d, n = shape
    for total in range(n * (d - 1) + 1):
        psi, tabs, got = _case(d, n, total)
        want = _dense(n, d, total, psi, tabs)
        for k in want:
            scale = max(1.0, float(np.max(np.abs(want[k]))))
            assert np.max(np.abs(np.asarray(got[k]).astype(np.complex128) - want[k])) <= 1e-12 * scale, (shape, total, k)


def test_a_zero_amplitude_row_is_skipped_without_changing_the_sums():
    d, n, total = 3, 4, 4
    psi, tabs, _ = _case(d, n, total)
    sparse = psi.copy()
    sparse[::3] = 0.0
    got = ref.correlations(n, d, total, sparse, **tabs)
    want = _dense(n, d, total, sparse, tabs)
    for k in want:
        assert np.max(np.abs(np.asarray(got[k]).astype(np.complex128) - want[k])) <= 1e-12 * max(1.0, float(np.max(np.abs(want[k]))))


def _as_got(r):
    return {k: np.asarray(v).astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in r.items()}


def test_the_comparison_accepts_the_rounded_reference_and_rejects_the_faults():
    d, n, total = 3, 4, 4
    psi, tabs, r = _case(d, n, total)
    sec = ref.Sector(n, d, total)
    W = ref.weights(n, **tabs)
    ref.compare("rounded reference", _as_got(r), r, sec.dim, n, W)
    # one entry off by twice the bound
    for k, at in (("pop", (1, 2)), ("dd", (1, 0, 2, 3)), ("str", (0, 3)), ("aa", (2, 1)), ("norm2", ())):
        g = _as_got(r)
        g[k] = np.array(g[k])
        g[k][at] += 2.0 * ref.bound(sec.dim, n, r["norm2"], W[k])
        with pytest.raises(AssertionError):
            ref.compare("off by twice the bound in %s" % k, g, r, sec.dim, n, W)
    # i and j swapped in aa; aa conjugated
    for name, fault in (("swapped", lambda a: a.T.copy()), ("conjugated", np.conj)):
        g = _as_got(r)
        g["aa"] = fault(g["aa"])
        with pytest.raises(AssertionError):
            ref.compare("aa " + name, g, r, sec.dim, n, W)
    # A+_i A_j in place of A_i A+_j: the diagonal changes too
    g = _as_got(r)
    A = ref.lowering(tabs["lower"])
    g["aa"] = np.array([[complex(ref.expect(sec, psi, [(i, A.T), (j, A)])) for j in range(n)] for i in range(n)])
    with pytest.raises(AssertionError):
        ref.compare("aa with the raising operator first", g, r, sec.dim, n, W)
    # the string running one site too far (g also at site j)
    g = _as_got(r)
    h, gm = tabs["string"]
    for i in range(n):
        for j in range(i + 1, n):
            g["str"][i, j] = g["str"][j, i] = float(ref.expect(sec, psi, ref.string_ops(h, gm, i, j, last=j + 1)).real)
    with pytest.raises(AssertionError):
        ref.compare("string one site too far", g, r, sec.dim, n, W)
    # an entry that must vanish exactly: in a sector with every site at level 0 nothing can be lowered
    psi0, tabs0, r0 = _case(3, 4, 0)
    assert np.all(r0["aa"][~np.eye(4, dtype=bool)] == 0)
    g = _as_got(r0)
    g["aa"][0, 1] = 1e-300
    with pytest.raises(AssertionError):
        ref.compare("a tiny value where zero is exact", g, r0, 1, 4, ref.weights(4, **tabs0))
