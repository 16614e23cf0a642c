"""CPU checks of the all-pair correlation entry points (qbh_corr_spin_dev, qbh_corr_hubbard_dev): both are exported and declared,
and every invalid argument is refused with a message BEFORE the device is looked for -- so these run without a GPU.  The vector
pointers below are never dereferenced: every call here fails in the argument checks (or, on a host without a device, at the
device check)."""
import ctypes as C

import pytest

import quantum_basis_amd as q
from quantum_basis_amd import _lib

EINVAL, ENODEVICE, EUNSUPP = -1, -2, -9
X = C.c_void_p(0x1000)           # stands for a device vector


def _msg():
    return _lib.lib().qbh_last_error().decode()


def test_both_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in ("qbh_corr_spin_dev", "qbh_corr_hubbard_dev"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    for name in ("spin_correlations", "hubbard_correlations", "structure_factor", "momentum_distribution", "energy_from_correlations"):
        assert hasattr(q, name)
    assert L.qbh_version() == 601


SPIN_BAD = [
    ((0, 0, X, None), EINVAL, "n_sites"),
    ((-3, 0, X, None), EINVAL, "n_sites"),
    ((63, 3, X, None), EINVAL, "n_sites"),                 # qbh_mf_heisenberg accepts 1 .. 62
    ((10, -1, X, None), EINVAL, "n_dn"),
    ((10, 11, X, None), EINVAL, "n_dn"),
    ((62, 34, X, None), EINVAL, "n_dn"),                   # ... and at most 33 down spins
    ((10, 5, X, X), EINVAL, "exactly one"),
    ((10, 5, None, None), EINVAL, "exactly one"),
    ((62, 31, X, None), EUNSUPP, "do not fit LDS"),        # 11 chunks x 32 particle counts x 64 x 8 bytes
    ((62, 31, None, X), EUNSUPP, "do not fit LDS"),
    ((60, 30, X, None), EUNSUPP, "do not fit LDS"),
]


@pytest.mark.parametrize("args,code,text", SPIN_BAD)
def test_spin_arguments_are_checked_before_the_device(args, code, text):
    n2 = C.c_double(-7.0)
    rc = _lib.lib().qbh_corr_spin_dev(args[0], args[1], args[2], args[3], C.byref(n2), None, None, None, None)
    assert rc == code
    assert "qbh_corr_spin_dev" in _msg() and text in _msg()
    assert n2.value == -7.0                                # nothing was written


HUB_BAD = [
    ((0, 0, 0, X, None), EINVAL, "n_sites"),
    ((32, 2, 2, X, None), EINVAL, "n_sites"),              # qbh_mf_hubbard accepts 1 .. 31
    ((8, -1, 2, X, None), EINVAL, "n_up"),
    ((8, 9, 2, X, None), EINVAL, "n_up"),
    ((8, 2, -1, X, None), EINVAL, "n_up"),
    ((8, 2, 9, X, None), EINVAL, "n_up"),
    ((8, 4, 4, X, X), EINVAL, "exactly one"),
    ((8, 4, 4, None, None), EINVAL, "exactly one"),
]


@pytest.mark.parametrize("args,code,text", HUB_BAD)
def test_hubbard_arguments_are_checked_before_the_device(args, code, text):
    n2 = C.c_double(-7.0)
    rc = _lib.lib().qbh_corr_hubbard_dev(args[0], args[1], args[2], args[3], args[4], C.byref(n2), None, None, None, None, None)
    assert rc == code
    assert "qbh_corr_hubbard_dev" in _msg() and text in _msg()
    assert n2.value == -7.0


def test_python_layer_refuses_what_it_cannot_translate():
    class Info:
        basis_internal = 2

    class Handle:                                          # a handle that keeps another order internally
        def info(self):
            return Info()

    with pytest.raises(ValueError):
        q.spin_correlations(8, 4, X, real=True, source=Handle())
    with pytest.raises(ValueError):
        q.hubbard_correlations(4, 2, 2, X, real=True, source=Handle())
    with pytest.raises(ValueError):
        q.hubbard_correlations(4, 2, 2, X, want=("dens", "pairing"))


def test_valid_arguments_without_a_device_fail_loudly():
    L = _lib.lib()
    if L.qbh_device_count() > 0:
        return                                             # with a device the call would run: tests/test_gpu_corr.py
    n2 = C.c_double()
    assert L.qbh_corr_spin_dev(10, 5, X, None, C.byref(n2), None, None, None, None) == ENODEVICE
    assert L.qbh_corr_hubbard_dev(8, 4, 4, None, X, C.byref(n2), None, None, None, None, None) == ENODEVICE
    with pytest.raises(_lib.QbhError):
        q.spin_correlations(10, 5, X)


def test_host_helpers():
    import numpy as np
    # two sites in a singlet: ss = -3/4 off the diagonal, S(pi) = (3/4 + 3/4 + 3/4 + 3/4) / 2, S(0) = 0
    ss = np.array([[0.75, -0.75], [-0.75, 0.75]])
    s = q.structure_factor(ss, [0.0, 1.0], [0.0, np.pi])
    assert np.allclose(s, [0.0, 1.5], atol=1e-15)
    # one particle in the k = 0 orbital of a 4-site ring: <c+_i c_j> = 1/4, n(0) = 1, n(k != 0) = 0
    hop = np.full((4, 4), 0.25, dtype=complex)
    nk = q.momentum_distribution(np.stack([hop, 0 * hop]), np.arange(4.0), 2 * np.pi * np.arange(4) / 4)
    assert nk.shape == (2, 4) and np.allclose(nk[0], [1, 0, 0, 0], atol=1e-15) and np.allclose(nk[1], 0)
    pos2 = [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert np.allclose(q.momentum_distribution(hop, pos2, [(0, 0), (np.pi, 0), (np.pi, np.pi)]), [1, 0, 0], atol=1e-15)
    # energies
    corr = {"zz": np.array([[0.25, -0.25], [-0.25, 0.25]]), "pm": np.array([[0.5, -0.5], [-0.5, 0.5]], dtype=complex)}
    assert q.energy_from_correlations(corr, [(0, 1)], J=2.0) == pytest.approx(-1.5)
    corr = {"hop": np.stack([hop, hop]), "nn": np.stack([np.eye(4)] * 4) * 0.3}
    assert q.energy_from_correlations(corr, [(0, 1), (1, 2), (2, 3), (3, 0)], t=1.0, U=2.0) == pytest.approx(-4.0 + 2.4)
