"""Pins tests/corrreprref.py (the longdouble reference of qbh_corr_spin_repr_dev, from representatives) against the explicit
route: unfold the sector state to the full space, column by column, and evaluate the operator definitions of tests/corrref.py
there.  Both sides are longdouble; they share the basis bookkeeping (which word is a representative) and nothing of the
formulas.  Also pins that the comparison rejects the three faults a sector formula invites."""
import numpy as np
import pytest

import corrreprref as rr

TOL = 1e-15                  # both routes sum a few hundred longdouble terms of a vector of norm about 1

CASES = {
    # name: (n_sites, n_dn, (perms, chars), zero-norm representatives)
    "chain8_k1": (8, 4, rr.chain(8, 1), 2),
    "chain8_k4": (8, 4, rr.chain(8, 4), None),
    "cells4x2_k1": (8, 3, rr.cells_chain(4, 2, 1), None),
    "torus3x2_k11": (6, 2, rr.torus(3, 2, 1, 1), 1),
    "no_symmetry": (7, 3, (np.arange(7, dtype=np.int32)[None, :], np.ones(1, dtype=np.complex128)), 0),
}


def _vector(dim, seed, keep_zero_rows, zero):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=dim) + 1j * rng.normal(size=dim)
    x /= np.linalg.norm(x)
    if not keep_zero_rows:
        x[zero] = 0.0
    return x


def _worst(a, b):
    return max(float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))) for k in ("norm2", "sz", "zz", "pm"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_the_unfolded_state(name):
    N, n_dn, (perms, chars), n_zero = CASES[name]
    S = rr.sector(N, n_dn, perms, chars)
    if n_zero is not None:
        assert int(S.zero.sum()) == n_zero
    x = _vector(S.dim, 5, True, S.zero)                      # garbage at the zero-norm representatives: ignored by both routes
    ref, exp = rr.spin_repr(N, n_dn, perms, chars, x), rr.explicit(N, n_dn, perms, chars, x)
    err = _worst(ref, exp)
    print("%s: dim %d, %d zero-norm, worst |reference - explicit| = %.3g" % (name, S.dim, int(S.zero.sum()), err))
    assert err < TOL
    # what the call promises of its arrays
    assert np.max(np.abs(ref["pm"] - ref["pm"].conj().T)) < TOL and np.max(np.abs(ref["zz"] - ref["zz"].T)) < TOL
    for g in range(len(perms)):
        pg = perms[g]
        assert np.max(np.abs(ref["pm"][np.ix_(pg, pg)] - ref["pm"])) < TOL and np.max(np.abs(ref["zz"][np.ix_(pg, pg)] - ref["zz"])) < TOL
    assert np.max(np.abs(np.diag(ref["zz"]) - ref["norm2"] / 4)) < TOL
    for k in ("sz", "zz", "pm"):
        assert np.all(np.abs(ref[k]) <= ref["A"][k] * (1 + 1e-15))


def test_pair_classes_of_the_two_sublattice_chain():
    N, n_dn, (perms, chars), _ = CASES["cells4x2_k1"]
    x = _vector(rr.sector(N, n_dn, perms, chars).dim, 6, True, None)
    pm = rr.spin_repr(N, n_dn, perms, chars, x)["pm"]
    distinct = {complex(np.round(complex(v), 12)) for v in pm.reshape(-1)}
    assert len(distinct) == 16                               # 64 ordered pairs (the diagonal included) / 4 translations


@pytest.mark.parametrize("fault,name", [("chi_not_conjugated", "chain8_k1"), ("no_sqrt", "chain8_k4"), ("zero_norm_counted", "chain8_k1"),
                                        ("zero_norm_counted", "torus3x2_k11")])
def test_comparison_rejects_the_faults(fault, name):
    N, n_dn, (perms, chars), _ = CASES[name]
    S = rr.sector(N, n_dn, perms, chars)
    x = _vector(S.dim, 9, True, S.zero)
    exp = rr.explicit(N, n_dn, perms, chars, x)
    bad = rr.spin_repr(N, n_dn, perms, chars, x, fault=fault)
    assert _worst(bad, exp) > 1e-4                           # an error of the size of the values, not of their rounding
