"""CPU checks of qbh_corr_spin_repr_dev (all-pair correlations of a spin-1/2 momentum-sector state): the symbol is exported,
declared and bound, and every invalid argument is refused with its code BEFORE the device is looked for -- so these run without a
GPU.  The vector pointers below are never dereferenced: every call here fails in the argument checks (or, on a host without a
device, at the device check)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import _lib

EINVAL, ENODEVICE, EUNSUPP = -1, -2, -9
X = C.c_void_p(0x1000)           # stands for a device vector
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qbhip.h")


def _msg():
    return _lib.lib().qbh_last_error().decode()


def _chain(n, k=0):
    perms = np.array([[(s + g) % n for s in range(n)] for g in range(n)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * k * np.arange(n) / n).astype(np.complex128)
    return perms, chars


def _call(n_sites, n_dn, perms, chars, vec, vec_re, n_trans=None):
    p = None if perms is None else np.ascontiguousarray(perms, dtype=np.int32)
    c = None if chars is None else np.ascontiguousarray(chars, dtype=np.complex128)
    n2, dim = C.c_double(-7.0), C.c_int64(-7)
    rc = _lib.lib().qbh_corr_spin_repr_dev(n_sites, n_dn, (len(p) if n_trans is None else n_trans),
                                           None if p is None else p.ctypes.data_as(C.c_void_p),
                                           None if c is None else c.ctypes.data_as(C.c_void_p), vec, vec_re, C.byref(n2), None, None, None,
                                           C.byref(dim), None)
    return rc, n2.value, dim.value


def test_symbol_is_exported_declared_and_bound():
    L = _lib.lib()
    assert "qbh_corr_spin_repr_dev" in _lib.EXPORTS and hasattr(L, "qbh_corr_spin_repr_dev")
    assert len(L.qbh_corr_spin_repr_dev.argtypes) == 13
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"\bint\s+qbh_corr_spin_repr_dev\s*\(\s*int n_sites, int n_dn, int n_trans, const int32_t \*perms, const double \*chars,", text)
    assert hasattr(q, "spin_repr_correlations")
    assert L.qbh_version() == 601


P8, C8 = _chain(8)
_, C8K1 = _chain(8, 1)
NOT_A_PERMUTATION = P8.copy()
NOT_A_PERMUTATION[3, 2] = NOT_A_PERMUTATION[3, 5]            # translation 3 sends two sites to one
OUT_OF_RANGE = P8.copy()
OUT_OF_RANGE[2, 0] = 8
SHIFTED = np.roll(P8, 1, axis=0)                             # translation 0 is not the identity

BAD = [
    ("n_sites 0", (0, 0, P8, C8, X, None), {}, EINVAL, "invalid argument"),
    ("n_sites 63", (63, 3, P8, C8, X, None), {}, EINVAL, "invalid argument"),
    ("n_dn negative", (8, -1, P8, C8, X, None), {}, EINVAL, "invalid argument"),
    ("n_dn above n_sites", (8, 9, P8, C8, X, None), {}, EINVAL, "invalid argument"),
    ("n_dn above 33", (62, 34, _chain(62)[0], _chain(62)[1], X, None), {}, EINVAL, "invalid argument"),
    ("no translations", (8, 4, P8, C8, X, None), {"n_trans": 0}, EINVAL, "invalid argument"),
    ("65 translations", (8, 4, P8, C8, X, None), {"n_trans": 65}, EINVAL, "invalid argument"),
    ("perms NULL", (8, 4, None, C8, X, None), {"n_trans": 8}, EINVAL, "invalid argument"),
    ("chars NULL", (8, 4, P8, None, X, None), {}, EINVAL, "invalid argument"),
    ("both vectors", (8, 4, P8, C8, X, X), {}, EINVAL, "exactly one"),
    ("neither vector", (8, 4, P8, C8, None, None), {}, EINVAL, "exactly one"),
    ("not a permutation", (8, 4, NOT_A_PERMUTATION, C8, X, None), {}, EINVAL, "translation 3 is not a site permutation"),
    ("image out of range", (8, 4, OUT_OF_RANGE, C8, X, None), {}, EINVAL, "translation 2 is not a site permutation"),
    ("translation 0 not the identity", (8, 4, SHIFTED, C8, X, None), {}, EINVAL, "translation 0 must be the identity"),
    ("packed real with a complex character", (8, 4, P8, C8K1, None, X), {}, EINVAL, "real characters"),
    ("2^40 words", (46, 23, _chain(46)[0], _chain(46)[1], X, None), {}, EUNSUPP, "too large to enumerate"),
]


@pytest.mark.parametrize("label,args,kw,code,text", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_arguments_are_checked_before_the_device(label, args, kw, code, text):
    rc, n2, dim = _call(*args, **kw)
    assert rc == code, label
    assert "qbh_corr_spin_repr_dev" in _msg() and text in _msg(), _msg()
    assert n2 == -7.0 and dim == -7                          # nothing was written


def test_rounding_of_a_real_character_is_not_a_complex_character():
    L = _lib.lib()
    if L.qbh_device_count() > 0:
        return
    perms, chars = _chain(8, 4)                              # exp(-i pi g): imaginary parts of 1e-16, the rounding of sin(pi g)
    assert np.any(chars.imag != 0.0) and np.max(np.abs(chars.imag)) < 1e-14
    assert _call(8, 4, perms, chars, None, X)[0] == ENODEVICE


def test_valid_arguments_without_a_device_fail_loudly():
    L = _lib.lib()
    if L.qbh_device_count() > 0:
        return                                               # with a device the call would run: tests/test_gpu_corr_repr.py
    assert _call(8, 4, P8, C8, X, None)[0] == ENODEVICE
    assert _call(8, 4, P8, C8, None, X)[0] == ENODEVICE
    assert _call(8, 4, P8, C8K1, X, None)[0] == ENODEVICE
    p62, c62 = _chain(62)                                    # 62 translations x 11 chunks: no refusal for the size of the tables
    assert _call(62, 2, p62, c62, X, None)[0] == ENODEVICE
    with pytest.raises(_lib.QbhError):
        q.spin_repr_correlations(8, 4, P8, C8, X)


def test_python_layer_checks_its_arguments():
    class Info:
        basis_internal = 2

    class Handle:                                            # a handle that keeps another order internally
        def info(self):
            return Info()

    with pytest.raises(ValueError):
        q.spin_repr_correlations(8, 4, P8, C8, X, real=True, source=Handle())
    with pytest.raises(ValueError):
        q.spin_repr_correlations(8, 4, P8, C8[:4], X)        # four characters for eight translations
