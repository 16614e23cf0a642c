"""CPU checks of the Kondo all-pair correlation entry point qbh_corr_kondo_dev: it is exported and bound, every invalid argument is
refused with a message that names it BEFORE the device is looked for and in the documented order (so these run without a GPU; the
vector pointer below is never dereferenced), nothing is written on a refusal, and the host arithmetic of the derived quantities
and of kondo_energy_from_correlations on hand-made arrays."""
import ctypes as C

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import _lib, correlations, kondo

EINVAL, ENODEVICE, EUNSUPP = -1, -2, -9
X = C.c_void_p(0x1000)           # stands for a device vector
GROUPS = ("site", "nn", "zn", "zz", "hop", "ee", "ll", "le")
OUT = {k: np.zeros(4 * 21 * 21 * 2) for k in GROUPS}       # room for any output array


def _msg():
    return _lib.lib().qbh_last_error().decode()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(n, ne, tz, xv, xr, n2, want=GROUPS):
    o = [(_p(OUT[k]) if k in want else None) for k in GROUPS]
    return _lib.lib().qbh_corr_kondo_dev(n, ne, tz, xv, xr, C.byref(n2) if n2 is not None else None, *o, None)


def test_the_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert "qbh_corr_kondo_dev" in _lib.EXPORTS and hasattr(L, "qbh_corr_kondo_dev")
    assert len(L.qbh_corr_kondo_dev.argtypes) == 15
    for name in ("kondo_correlations", "kondo_energy_from_correlations"):
        assert hasattr(q, name)
    assert L.qbh_version() == 601


NO_N2 = "no norm2"
# (n_sites, n_elec, two_sz, d_vec, d_vec_re, norm2 given), code, text in the message
BAD = [
    ((0, 0, 0, X, None, True), EINVAL, "n_sites"),
    ((22, 22, 0, X, None, True), EINVAL, "n_sites"),
    ((4, -1, 1, X, None, True), EINVAL, "n_elec"),
    ((4, 9, 1, X, None, True), EINVAL, "n_elec"),
    ((4, 4, 1, X, None, True), EINVAL, "odd"),
    ((2, 0, 4, X, None, True), EUNSUPP, "empty"),
    ((4, 4, 0, X, X, True), EINVAL, "exactly one"),
    ((4, 4, 0, None, None, True), EINVAL, "exactly one"),
    ((4, 4, 0, X, None, False), EINVAL, "norm2"),
    ((4, 4, 0, None, X, False), EINVAL, "norm2"),
    # the order of the checks: shape, empty sector, vector pointers, norm2
    ((0, -1, 1, X, X, False), EINVAL, "n_sites"),
    ((4, 9, 0, X, X, False), EINVAL, "n_elec"),
    ((4, 4, 1, X, X, False), EINVAL, "odd"),
    ((2, 0, 4, X, X, False), EUNSUPP, "empty"),
    ((2, 0, 4, None, None, False), EUNSUPP, "empty"),
    ((4, 4, 0, X, X, False), EINVAL, "exactly one"),
    ((4, 4, 0, None, None, False), EINVAL, "exactly one"),
]


@pytest.mark.parametrize("args,code,text", BAD, ids=lambda v: v if isinstance(v, str) else None)
def test_arguments_are_checked_before_the_device(args, code, text):
    n, ne, tz, xv, xr, with_n2 = args
    n2 = C.c_double(-7.0)
    for a in OUT.values():
        a[:] = -7.0
    assert _call(n, ne, tz, xv, xr, n2 if with_n2 else None) == code
    assert "qbh_corr_kondo_dev" in _msg() and text in _msg(), _msg()
    assert n2.value == -7.0 and all(np.all(a == -7.0) for a in OUT.values())        # nothing was written


def test_valid_arguments_without_a_device_fail_loudly():
    L = _lib.lib()
    if L.qbh_device_count() > 0:
        return                                             # with a device the call would run: tests/test_gpu_kondo_corr.py
    n2 = C.c_double(-7.0)
    for a in OUT.values():
        a[:] = -7.0
    assert _call(21, 21, 0, None, X, n2, want=()) == ENODEVICE                     # the largest shape: no 2^31 or 2^40 limit
    assert _call(1, 1, 0, X, None, n2, want=()) == ENODEVICE
    assert _call(4, 4, 0, X, None, n2) == ENODEVICE                                # every group wanted
    assert n2.value == -7.0 and all(np.all(a == -7.0) for a in OUT.values())
    with pytest.raises(_lib.QbhError):
        q.kondo_correlations(4, 4, 0, X)
    with pytest.raises(_lib.QbhError):
        q.kondo_correlations(4, 4, 0, X, real=True, want=("hop", "pm_le"))


def test_the_wrapper_refuses_before_the_device():
    with pytest.raises(ValueError):
        q.kondo_correlations(4, 4, 0, X, want=("hop", "flip"))                     # a group of another family
    with pytest.raises(_lib.QbhError) as e:
        q.kondo_correlations(4, 4, 1, X)
    assert "odd" in str(e.value)


def test_derived_quantities_host_arithmetic():
    # two sites, hand-made raw arrays (not a physical state: the arithmetic alone is checked)
    out = {
        "norm2": 2.0,
        "dens": np.array([[1.0, 0.5], [0.25, 0.75]]),
        "nn": np.array([[[1.0, 0.5], [0.5, 0.5]], [[0.25, 0.125], [0.0, 0.25]], [[0.25, 0.0], [0.125, 0.25]], [[0.25, 0.75], [0.75, 0.75]]]),
        "zn": np.array([[[0.5, -0.25], [0.125, 0.25]], [[0.0, 0.25], [-0.125, 0.5]]]),
        "zz_ll": np.array([[0.5, -0.25], [-0.25, 0.5]]),
        "pm_ee": np.array([[0.75, 0.5 + 0.25j], [0.5 - 0.25j, 0.25]]),
        "pm_ll": np.array([[1.0, -0.5 + 0.125j], [-0.5 - 0.125j, 1.0]]),
        "pm_le": np.array([[-0.5 + 1j, 0.25 - 2j], [0.125 + 3j, -0.75 - 4j]]),
    }
    c = correlations._kondo_derived(dict(out))
    assert np.array_equal(c["sz_elec"], [0.375, -0.125])
    assert np.array_equal(c["zz_le"], [[0.25, -0.25], [0.125, -0.125]])
    assert np.array_equal(c["zz_ee"], 0.25 * np.array([[0.75, 1.125], [1.125, 0.75]]))
    assert np.array_equal(c["ss_ll"], [[1.5, -0.75], [-0.75, 1.5]])
    assert np.array_equal(c["ss_ee"], c["zz_ee"] + np.array([[0.75, 0.5], [0.5, 0.25]]))
    assert np.array_equal(c["ss_le"], [[-0.25, 0.0], [0.25, -0.875]])              # not symmetric: S_i . s_j
    assert c["total_spin"] == np.sum(c["ss_ll"]) + np.sum(c["ss_ee"]) + 2.0 * np.sum(c["ss_le"])
    # each derived quantity only where its inputs are present
    part = correlations._kondo_derived({"norm2": 2.0, "zn": out["zn"], "pm_le": out["pm_le"]})
    assert set(part) == {"norm2", "zn", "pm_le", "zz_le", "ss_le"}
    assert "total_spin" not in correlations._kondo_derived({k: v for k, v in out.items() if k != "pm_ee"})


def test_energy_from_correlations_host_arithmetic():
    hop = np.array([[[1.0, 0.5 + 0.25j], [0.5 - 0.25j, 0.5]], [[0.25, -0.125 + 1j], [-0.125 - 1j, 0.75]]])
    corr = {"hop": hop, "docc": np.array([0.25, 0.5]), "zz_le": np.array([[0.25, 9.0], [9.0, -0.125]]),
            "pm_le": np.array([[-0.5 + 1j, 9.0], [9.0, -0.75 - 4j]]), "zz_ll": np.array([[0.5, -0.25], [-0.25, 0.5]]),
            "pm_ll": np.array([[1.0, -0.5 + 0.125j], [-0.5 - 0.125j, 1.0]])}
    t = kondo.Terms([(0, 1, 2.0 - 1j, -0.5), (1, 0, 2.0 + 1j, -0.5), (0, 0, 0.5, 0.25)], [1.0, 2.0], [4.0, -2.0], [(0, 1, 3.0, 0.5)])
    want = ((2.0 - 1j) * hop[0][0, 1] + (2.0 + 1j) * hop[0][1, 0] - 0.5 * (hop[1][0, 1] + hop[1][1, 0]) + 0.5 * 1.0 + 0.25 * 0.25).real
    want += 1.5 * 0.75                                      # U sum docc
    want += 1.0 * 0.25 + 2.0 * -0.125 + 4.0 * -0.5 + -2.0 * -0.75
    want += 3.0 * -0.25 + 0.5 * -0.5
    assert q.kondo_energy_from_correlations(corr, t, U=1.5) == pytest.approx(want, abs=1e-15)
    only_spins = kondo.Terms([], [0.0, 0.0], [0.0, 0.0], [(0, 1, 1.0, 1.0)])
    assert q.kondo_energy_from_correlations({"zz_ll": corr["zz_ll"], "pm_ll": corr["pm_ll"]}, only_spins) == -0.75
