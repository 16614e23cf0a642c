"""CPU checks of qbh_corr_hubbard_repr_dev (all-pair correlations of a two-species fermion momentum-sector state): the symbol is
exported, declared and bound, and every invalid argument is refused with its code and a message that names it BEFORE the device is
looked for, in the documented order -- so these run without a GPU.  The vector pointers below are never dereferenced: every call
here fails in the argument checks (or, on a host without a device, at the device check)."""
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
WHO = "qbh_corr_hubbard_repr_dev"


def _msg():
    return _lib.lib().qbh_last_error().decode()


def _ring(n, k=0):
    perms = np.array([[(s + g) % n for s in range(n)] for g in range(n)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * k * np.arange(n) / n).astype(np.complex128)
    return perms, chars


def _call(n_sites, n_up, n_dn, perms, chars, vec, vec_re, n_trans=None, no_double=0):
    p = None if perms is None else np.ascontiguousarray(perms, dtype=np.int32)
    c = None if chars is None else np.ascontiguousarray(chars, dtype=np.complex128)
    N = max(n_sites, 1)
    n2, dim = C.c_double(-7.0), C.c_int64(-7)
    out = {"dens": np.full((2, N), -7.0), "nn": np.full((4, N, N), -7.0), "hop": np.full((2, N, N), -7.0 - 7.0j),
           "flip": np.full((N, N), -7.0 - 7.0j)}
    ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()}
    rc = _lib.lib().qbh_corr_hubbard_repr_dev(n_sites, n_up, n_dn, no_double, (len(p) if n_trans is None else n_trans),
                                              None if p is None else p.ctypes.data_as(C.c_void_p),
                                              None if c is None else c.ctypes.data_as(C.c_void_p), vec, vec_re, C.byref(n2),
                                              ptr["dens"], ptr["nn"], ptr["hop"], ptr["flip"], C.byref(dim), None)
    untouched = n2.value == -7.0 and dim.value == -7 and all(np.all(v.view(np.float64) == -7.0) for v in out.values())
    return rc, untouched


def test_symbol_is_exported_declared_and_bound():
    L = _lib.lib()
    assert WHO in _lib.EXPORTS and hasattr(L, WHO)
    vp = C.c_void_p
    assert L.qbh_corr_hubbard_repr_dev.argtypes == [C.c_int] * 5 + [vp] * 9 + [C.POINTER(C.c_int64), vp]
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"\bint\s+qbh_corr_hubbard_repr_dev\s*\(\s*int n_sites, int n_up, int n_dn, int no_double, int n_trans, "
                     r"const int32_t \*perms,\s*const double \*chars,\s*const qbh_z \*d_vec, const double \*d_vec_re, double \*norm2,", text)
    assert hasattr(q, "hubbard_repr_correlations")


P8, C8 = _ring(8)
_, C8K1 = _ring(8, 1)
NOT_A_PERMUTATION = P8.copy()
NOT_A_PERMUTATION[3, 2] = NOT_A_PERMUTATION[3, 5]            # translation 3 sends two sites to one
OUT_OF_RANGE = P8.copy()
OUT_OF_RANGE[2, 0] = 8
SHIFTED = np.roll(P8, 1, axis=0)                             # translation 0 is not the identity
P31, C31 = _ring(31)

# in the documented order of the checks; a case that breaks several rules names the FIRST one
BAD = [
    ("perms NULL", (8, 4, 4, None, C8, X, None), {"n_trans": 8}, EINVAL, "perms and chars"),
    ("chars NULL and n_sites 0", (0, 4, 4, P8, None, X, None), {}, EINVAL, "perms and chars"),
    ("n_sites 0", (0, 0, 0, P8, C8, X, None), {}, EINVAL, "n_sites = 0"),
    ("n_sites 32", (32, 3, 3, P8, C8, X, None), {}, EINVAL, "n_sites = 32"),
    ("n_sites 32 and n_up negative", (32, -1, 3, P8, C8, X, None), {}, EINVAL, "n_sites = 32"),
    ("n_up negative", (8, -1, 4, P8, C8, X, None), {}, EINVAL, "(n_up, n_dn) = (-1, 4)"),
    ("n_up above n_sites", (8, 9, 4, P8, C8, X, None), {}, EINVAL, "(n_up, n_dn) = (9, 4)"),
    ("n_dn negative", (8, 4, -2, P8, C8, X, None), {}, EINVAL, "(n_up, n_dn) = (4, -2)"),
    ("n_dn above n_sites and no translations", (8, 4, 9, P8, C8, X, None), {"n_trans": 0}, EINVAL, "(n_up, n_dn) = (4, 9)"),
    ("no translations", (8, 4, 4, P8, C8, X, None), {"n_trans": 0}, EINVAL, "n_trans = 0"),
    ("65 translations and no_double 2", (8, 4, 4, P8, C8, X, None), {"n_trans": 65, "no_double": 2}, EINVAL, "n_trans = 65"),
    ("no_double 2 and both vectors", (8, 4, 4, P8, C8, X, X), {"no_double": 2}, EINVAL, "no_double = 2"),
    ("both vectors", (8, 4, 4, P8, C8, X, X), {}, EINVAL, "exactly one"),
    ("neither vector and not a permutation", (8, 4, 4, NOT_A_PERMUTATION, C8, None, None), {}, EINVAL, "exactly one"),
    ("not a permutation", (8, 4, 4, NOT_A_PERMUTATION, C8, X, None), {}, EINVAL, "translation 3 is not a site permutation"),
    ("image out of range", (8, 4, 4, OUT_OF_RANGE, C8, X, None), {}, EINVAL, "translation 2 is not a site permutation"),
    ("translation 0 not the identity", (8, 4, 4, SHIFTED, C8K1, None, X), {}, EINVAL, "translation 0 must be the identity"),
    ("packed real with a complex character", (8, 5, 5, P8, C8K1, None, X), {"no_double": 1}, EINVAL, "real characters"),
    ("no_double with more particles than sites", (8, 5, 4, P8, C8, X, None), {"no_double": 1}, EINVAL, "the space is empty"),
    ("2^40 words", (31, 15, 15, P31, C31, X, None), {}, EUNSUPP, "too large to enumerate"),
]


@pytest.mark.parametrize("label,args,kw,code,text", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_arguments_are_checked_before_the_device_in_the_documented_order(label, args, kw, code, text):
    rc, untouched = _call(*args, **kw)
    assert rc == code, label
    assert WHO in _msg() and text in _msg(), _msg()
    assert untouched                                         # nothing was written


def test_rounding_of_a_real_character_is_not_a_complex_character():
    if _lib.lib().qbh_device_count() > 0:
        return
    perms, chars = _ring(8, 4)                               # exp(-i pi g): imaginary parts of 1e-16, the rounding of sin(pi g)
    assert np.any(chars.imag != 0.0) and np.max(np.abs(chars.imag)) < 1e-14
    assert _call(8, 4, 4, perms, chars, None, X)[0] == ENODEVICE


def test_valid_arguments_without_a_device_fail_last_and_loudly():
    if _lib.lib().qbh_device_count() > 0:
        return                                               # with a device the call would run: tests/test_gpu_corr_hubrepr.py
    for args, kw in [((8, 4, 4, P8, C8, X, None), {}), ((8, 4, 4, P8, C8, None, X), {}), ((8, 4, 4, P8, C8K1, X, None), {}),
                     ((8, 4, 4, P8, C8, X, None), {"no_double": 1}), ((8, 0, 0, P8, C8, X, None), {}),
                     ((31, 2, 1, P31, C31, X, None), {})]:
        rc, untouched = _call(*args, **kw)
        assert rc == ENODEVICE and untouched
    # 62 group elements x 6 chunks of tables (186 KB): no refusal for the size of the tables
    rot = [[(s + t) % 31 for s in range(31)] for t in range(31)]
    ref = [[(t - s) % 31 for s in range(31)] for t in range(31)]
    assert _call(31, 2, 1, np.array(rot + ref, dtype=np.int32), np.ones(62, dtype=np.complex128), X, None)[0] == ENODEVICE
    with pytest.raises(_lib.QbhError):
        q.hubbard_repr_correlations(8, 4, 4, P8, C8, X)


def test_python_layer_checks_its_arguments():
    class Info:
        basis_internal = 2

    class Handle:                                            # a handle that keeps another order internally
        def info(self):
            return Info()

    with pytest.raises(ValueError):
        q.hubbard_repr_correlations(8, 4, 4, P8, C8, X, real=True, source=Handle())
    with pytest.raises(ValueError):
        q.hubbard_repr_correlations(8, 4, 4, P8, C8[:4], X)  # four characters for eight translations
    with pytest.raises(ValueError):
        q.hubbard_repr_correlations(8, 4, 4, P8, C8, X, want=("dens", "pm"))
