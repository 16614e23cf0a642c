"""CPU checks of the d-level all-pair correlation entry point qbh_corr_qudit_dev: it is exported and bound, every invalid
argument is refused with a message that names it BEFORE the device is looked for (so these run without a GPU; the vector pointer
below is never dereferenced), and the host arithmetic of the three Python helpers on hand-made arrays."""
import ctypes as C

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import _lib, correlations

EINVAL, ENODEVICE, EUNSUPP = -1, -2, -9
X = C.c_void_p(0x1000)           # stands for a device vector
D3 = np.array([1.0, 0.0, -1.0, 1.0, 0.0, 1.0])             # two diagonal tables of d = 3
T3 = np.array([1.0, 0.5, -1.0])
NAN3 = np.array([1.0, np.nan, -1.0])
INF0 = np.array([np.inf, 1.0, 1.0])                        # lower[0] is ignored


def _msg():
    return _lib.lib().qbh_last_error().decode()


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_the_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert "qbh_corr_qudit_dev" in _lib.EXPORTS and hasattr(L, "qbh_corr_qudit_dev")
    assert len(L.qbh_corr_qudit_dev.argtypes) == 16
    for name in ("qudit_correlations", "spin_s_correlations", "bose_correlations"):
        assert hasattr(q, name)
    assert L.qbh_version() == 601


OUT = np.zeros(4 * 64 * 64 * 2)                            # room for any output array asked for below
# (n_sites, d, total, d_vec, d_vec_re, n_diag, diag, string_end, string_mid, lower, wanted outputs), code, text in the message
BAD = [
    ((0, 3, 0, X, None, 0, None, None, None, None, ()), EINVAL, "n_sites"),
    ((4, 1, 0, X, None, 0, None, None, None, None, ()), EINVAL, "d >= 2"),
    ((4, 9, 4, X, None, 0, None, None, None, None, ()), EUNSUPP, "at most 8"),
    ((33, 3, 4, X, None, 0, None, None, None, None, ()), EUNSUPP, "64 bits"),
    ((22, 8, 4, X, None, 0, None, None, None, None, ()), EUNSUPP, "64 bits"),
    ((4, 3, -1, X, None, 0, None, None, None, None, ()), EINVAL, "total"),
    ((4, 3, 9, X, None, 0, None, None, None, None, ()), EINVAL, "total"),
    ((4, 3, 4, X, X, 0, None, None, None, None, ()), EINVAL, "exactly one"),
    ((4, 3, 4, None, None, 0, None, None, None, None, ()), EINVAL, "exactly one"),
    ((4, 3, 4, X, None, -1, D3, None, None, None, ()), EINVAL, "n_diag"),
    ((4, 3, 4, X, None, 5, D3, None, None, None, ()), EINVAL, "n_diag"),
    ((4, 3, 4, X, None, 2, None, None, None, None, ()), EINVAL, "diag is NULL"),
    ((4, 3, 4, X, None, 0, None, T3, None, None, ()), EINVAL, "string_end and string_mid"),
    ((4, 3, 4, None, X, 0, None, None, T3, None, ()), EINVAL, "string_end and string_mid"),
    ((4, 3, 4, X, None, 0, None, None, None, None, ("dd",)), EINVAL, "dd is wanted"),
    ((4, 3, 4, X, None, 2, D3, None, None, None, ("str",)), EINVAL, "str is wanted"),
    ((4, 3, 4, X, None, 2, D3, T3, T3, None, ("aa",)), EINVAL, "aa is wanted"),
    ((4, 3, 4, X, None, 2, np.append(D3[:5], np.inf), None, None, None, ()), EINVAL, "diag[5]"),
    ((4, 3, 4, X, None, 0, None, NAN3, T3, None, ()), EINVAL, "string_end[1]"),
    ((4, 3, 4, X, None, 0, None, T3, NAN3, None, ()), EINVAL, "string_mid[1]"),
    ((4, 3, 4, X, None, 0, None, None, None, NAN3, ()), EINVAL, "lower[1]"),
    # the order of the checks: the shape before the charge, the charge before the vectors, the vectors before the tables
    ((0, 3, -1, X, X, 9, None, None, None, None, ()), EINVAL, "n_sites"),
    ((4, 3, -1, X, X, 9, None, None, None, None, ()), EINVAL, "total"),
    ((4, 3, 4, X, X, 9, None, None, None, None, ()), EINVAL, "exactly one"),
    ((4, 3, 4, X, None, 9, None, T3, None, None, ("dd",)), EINVAL, "n_diag"),
    ((4, 3, 4, X, None, 0, None, T3, None, None, ("dd",)), EINVAL, "string_end and string_mid"),
    ((4, 3, 4, X, None, 0, None, NAN3, T3, None, ("dd",)), EINVAL, "dd is wanted"),
]


def _call(args, n2):
    n, d, total, xv, xr, K, diag, he, gm, low, want = args
    o = {k: (_p(OUT) if k in want else None) for k in ("pop", "dd", "str", "aa")}
    return _lib.lib().qbh_corr_qudit_dev(n, d, total, xv, xr, K, _p(diag), _p(he), _p(gm), _p(low), C.byref(n2), o["pop"], o["dd"], o["str"],
                                         o["aa"], None)


@pytest.mark.parametrize("args,code,text", BAD, ids=lambda v: v if isinstance(v, str) else None)
def test_arguments_are_checked_before_the_device(args, code, text):
    n2 = C.c_double(-7.0)
    OUT[:] = -7.0
    assert _call(args, n2) == code
    assert "qbh_corr_qudit_dev" in _msg() and text in _msg(), _msg()
    assert n2.value == -7.0 and np.all(OUT == -7.0)        # nothing was written


def test_valid_arguments_without_a_device_fail_loudly():
    L = _lib.lib()
    if L.qbh_device_count() > 0:
        return                                             # with a device the call would run: tests/test_gpu_qudit_corr.py
    n2 = C.c_double(-7.0)
    assert _call((4, 3, 4, X, None, 2, D3, T3, T3, INF0, ("pop", "dd", "str", "aa")), n2) == ENODEVICE      # lower[0] is ignored
    assert _call((64, 2, 32, None, X, 0, None, None, None, None, ()), n2) == ENODEVICE                      # the largest tables fit LDS
    assert _call((21, 8, 147, None, X, 0, None, None, None, None, ()), n2) == ENODEVICE
    assert n2.value == -7.0
    with pytest.raises(_lib.QbhError):
        q.spin_s_correlations(4, 1, 0, X)
    with pytest.raises(_lib.QbhError):
        q.bose_correlations(4, 4, 2, X, real=True)


def test_spin_s_host_arithmetic():
    # two spins 1 (levels l = 1 - m), hand-made raw arrays with norm2 = 2
    pop = np.array([[1.0, 0.5, 0.5], [0.25, 0.75, 1.0]])
    zz = np.array([[1.5, -0.4], [-0.4, 1.25]])
    pm = np.array([[2.0, 0.3 + 0.1j], [0.3 - 0.1j, 1.0]])
    st = np.array([[1.5, -0.2], [-0.2, 1.25]])
    raw = {"norm2": 2.0, "pop": pop, "dd": zz[None, None], "aa": pm, "str": st}
    c = correlations._spin_s_from_raw(1, raw)
    assert np.array_equal(c["sz"], [0.5, -0.75]) and np.array_equal(c["sz2"], [1.5, 1.25])
    assert c["zz"] is not None and np.array_equal(c["pm"], pm) and np.array_equal(c["string"], st)
    assert np.array_equal(c["ss"], [[4.0, -0.4 + 0.3], [-0.4 + 0.3, 4.0]])               # S(S+1) norm2 on the diagonal
    assert q.energy_from_correlations(c, [(0, 1)], J=2.0) == pytest.approx(2.0 * (-0.4 + 0.3))
    half = correlations._spin_s_from_raw(0.5, {"norm2": 1.0, "pop": np.array([[0.25, 0.75]]), "dd": np.array([[[[0.25]]]]),
                                               "aa": np.array([[0.25 + 0j]])})
    assert half["string"] is None and np.array_equal(half["sz"], [-0.25]) and half["ss"][0, 0] == 0.75


def test_bose_host_arithmetic():
    # two sites, at most 2 bosons each, norm2 = 2
    pop = np.array([[0.5, 1.0, 0.5], [1.0, 0.5, 0.5]])
    nn = np.array([[3.0, 0.7], [0.7, 2.5]])
    aa = np.array([[4.0, 0.3 + 0.2j], [0.3 - 0.2j, 3.5]])                                 # <b_i b+_j>
    par = np.array([[2.0, -0.5], [-0.5, 2.0]])
    c = correlations._bose_from_raw(2, {"norm2": 2.0, "pop": pop, "dd": nn[None, None], "aa": aa, "str": par})
    assert np.array_equal(c["dens"], [2.0, 1.5]) and np.array_equal(c["nn"], nn) and np.array_equal(c["parity"], par)
    assert np.array_equal(c["obdm"], [[2.0, 0.3 - 0.2j], [0.3 + 0.2j, 1.5]])              # aa[j][i] off the diagonal, <b b+> - norm2 on it
    nk = q.momentum_distribution(c["obdm"], [0.0, 1.0], [0.0, np.pi])
    assert np.allclose(nk, [(3.5 + 0.6) / 2, (3.5 - 0.6) / 2], atol=1e-15)
    assert np.allclose(q.structure_factor(c["nn"], [0.0, 1.0], [0.0]), [(5.5 + 1.4) / 2], atol=1e-15)


def test_the_thin_wrapper_shapes_its_tables():
    with pytest.raises(ValueError):
        q.qudit_correlations(4, 3, 4, X, diag=([1.0, 2.0],))          # a table of the wrong length
    with pytest.raises(_lib.QbhError) as e:
        q.qudit_correlations(4, 3, 9, X)
    assert "total" in str(e.value)
