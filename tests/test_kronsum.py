"""CPU tier: the synthetic Kronecker-sum builder (tests/kronsum.py) against a dense np.kron, and the long-double row sums
the element-wise SpMV checks of test_gpu_realforms.py compare with, against exact rational sums."""
from fractions import Fraction

import numpy as np
import pytest

import kronsum


def _to_dense(K):
    n = K["dim"]
    M = np.zeros((n, n))
    ia, ja, val = K["ia"], K["ja"], K["val"]
    for r in range(n):
        M[r, ja[ia[r]:ia[r + 1]]] = val[ia[r]:ia[r + 1]]
    return M


@pytest.mark.parametrize("kw", [dict(NU=5, S=7), dict(NU=9, S=6, wu=6, band=1, far=1, n_amp=5, n_diag=7),
                                dict(NU=8, S=12, wu=4, band=3, far=2, n_amp=16, n_diag=30, empty_t=3),
                                dict(NU=1, S=9, wu=1, band=2, n_amp=2, n_diag=3), dict(NU=4, S=2, wu=1, band=1, n_amp=1, n_diag=1)])
def test_builder_equals_dense_kronecker_sum(kw):
    K = kronsum.kronsum(seed=3, **kw)
    NU, S = kw["NU"], kw["S"]
    ia, ja = K["ia"], K["ja"]
    assert K["dim"] == NU * S and ia.dtype == np.int64 and ja.dtype == np.int64 and ia[0] == 0 and ia[-1] == len(ja)
    for r in range(K["dim"]):                                           # sorted columns, diagonal stored, no duplicates
        c = ja[ia[r]:ia[r + 1]]
        assert np.all(np.diff(c) > 0) and r in c
    M = _to_dense(K)
    assert np.array_equal(M, kronsum.dense(K)) and np.array_equal(M, M.T)
    T = np.zeros((NU, NU))
    for u in range(NU):
        T[u, K["T"][1][K["T"][0][u]:K["T"][0][u + 1]]] = K["T"][2][K["T"][0][u]:K["T"][0][u + 1]]
    assert np.all(np.diag(T) == 0.0)
    # what the table route sees: the widest live T row, the hop amplitudes, the dictionary
    assert K["wu"] == int((T != 0).sum(axis=1).max())
    if kw.get("wu", 3) > 1:
        assert K["wu"] == kw.get("wu", 3)
    hops = M[~np.eye(K["dim"], dtype=bool)]
    assert K["n_amp"] == len(np.unique(hops[hops != 0])) == kw.get("n_amp", 3)
    assert K["n_dict"] == len(np.unique(K["val"])) == K["n_amp"] + kw.get("n_diag", 4)
    e = kw.get("empty_t", 0)
    if e:
        assert np.all(T[NU - e:] == 0) and np.all(T[:, NU - e:] == 0)


def test_far_hops_reach_half_the_minor_range():
    K = kronsum.kronsum(NU=2, S=40, wu=1, band=1, far=2)
    ia, ja = K["ia"], K["ja"]
    rows = np.repeat(np.arange(K["dim"]), np.diff(ia))
    near = (rows // 40) == (ja // 40)
    dist = np.abs((rows % 40) - (ja % 40))[near]
    assert dist.max() >= 40 // 2 - 2 and set(np.unique(dist)) <= {0, 1, 18, 19, 21, 22}


def test_longdouble_row_sums_equal_exact_rational_sums():
    """The reference of the element-wise checks: np.add.reduceat in long double, empty rows (and a trailing empty row) giving
    0, against fractions.Fraction sums of the same products on a sample of rows."""
    K = kronsum.kronsum(NU=6, S=50, wu=4, band=3, far=1, n_amp=7, n_diag=9, empty_t=1, seed=5)
    ia, ja, val = K["ia"].copy(), K["ja"], K["val"].copy()
    val[ia[3]:ia[4]] = 0.0
    # rows 10 and the last one empty
    keep = np.ones(len(ja), dtype=bool)
    keep[ia[10]:ia[11]] = False
    keep[ia[-2]:ia[-1]] = False
    ja, val = ja[keep], val[keep]
    lens = np.diff(ia)
    lens[10] = 0
    lens[-1] = 0
    ia = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = kronsum.probe_vector(K["dim"], 9)
    ref, absref = kronsum.row_sums(ia, ja, val, x)
    assert ref[10] == 0 and absref[10] == 0 and ref[-1] == 0 and absref[-1] == 0 and ref[3] == 0
    eps_ld = Fraction(*np.finfo(np.longdouble).eps.as_integer_ratio())

    def frac(v):
        return Fraction(*np.longdouble(v).as_integer_ratio())
    for r in [0, 1, 3, 10, 49, 50, 151, K["dim"] - 2, K["dim"] - 1]:
        exact = sum((Fraction(float(val[p])) * Fraction(float(x[ja[p]])) for p in range(ia[r], ia[r + 1])), Fraction(0))
        babs = sum((abs(Fraction(float(val[p])) * Fraction(float(x[ja[p]]))) for p in range(ia[r], ia[r + 1])), Fraction(0))
        assert abs(frac(ref[r]) - exact) <= (lens[r] + 1) * eps_ld * babs, r
        assert abs(frac(absref[r]) - babs) <= (lens[r] + 1) * eps_ld * babs, r
        # and far below what the double-precision bound allows
        assert float(abs(frac(ref[r]) - exact)) <= 1e-3 * np.finfo(np.float64).eps * float(babs), r


def test_probe_vector_entries():
    x = kronsum.probe_vector(1000, 1)
    a = np.abs(x) * np.sqrt(1000)
    assert abs(np.linalg.norm(x) - 1.0) < 1e-15 and a.max() / a.min() <= 4.0 + 1e-12 and (x > 0).any() and (x < 0).any()
