"""CPU checks of the matrix-free Kondo-lattice operator qbh_mf_kondo: the C ABI declares and exports it, every shape and term
check that tests/test_kondo_cpu.py exercises for qbh_gen_kondo returns the same code from it before the device is looked for,
and the limits of the stored form that it drops (int32 columns, 160 entries per row) are not refused.  kondo.rank /
kondo.unrank, the host's way from an index of such a sector to its word and back, against the enumerated basis."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quantum_basis_amd import _lib, kondo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE, ENOTHERM, EUNSUPP = -1, -2, -5, -9
OK_HERE = (0, ENODEVICE)                     # ok on a GPU box, no device here


def test_header_declares_and_library_exports_qbh_mf_kondo():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qbhip.h")).read(), flags=re.S)
    assert re.search(r"\bqbh_mf_kondo\s*\(", text)
    assert "qbh_mf_kondo" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "qbh_mf_kondo")
    assert _lib.lib().qbh_version() == 601


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def _call(name, n_sites, n_elec, two_sz, T, U=0.0, rows=(0, -1)):
    """qbh_gen_kondo or qbh_mf_kondo on host arrays; returns (rc, dim_out)."""
    hops, sb = list(T.hops), list(T.sbonds)
    a = [np.ascontiguousarray(np.array([[h[0], h[1]] for h in hops], dtype=np.int32).reshape(-1, 2)),
         np.ascontiguousarray(np.array([h[2] for h in hops], dtype=np.complex128)),
         np.ascontiguousarray(np.array([h[3] for h in hops], dtype=np.complex128)),
         np.ascontiguousarray(T.kz, dtype=np.float64), np.ascontiguousarray(T.kxy, dtype=np.float64),
         np.ascontiguousarray(np.array([[b[0], b[1]] for b in sb], dtype=np.int32).reshape(-1, 2)),
         np.ascontiguousarray(np.array([b[2] for b in sb], dtype=np.float64)),
         np.ascontiguousarray(np.array([b[3] for b in sb], dtype=np.float64))]
    h = C.c_void_p()
    dim = C.c_int64(-1)
    rc = getattr(_lib.lib(), name)(C.byref(h), n_sites, n_elec, two_sz, len(hops), a[0].ctypes.data, a[1].ctypes.data,
                                   a[2].ctypes.data, U, a[3].ctypes.data, a[4].ctypes.data, len(sb), a[5].ctypes.data,
                                   a[6].ctypes.data, a[7].ctypes.data, rows[0], rows[1], C.byref(dim), None)
    assert rc != 0 or h.value
    if rc == 0:
        _lib.lib().qbh_csr_destroy(h)
    return rc, dim.value


def _mf(*a, **k):
    return _call("qbh_mf_kondo", *a, **k)


def _err():
    return _lib.lib().qbh_last_error().decode()


def _same_refusal(code, *a, **k):
    """Both entry points refuse the call with `code` (and report the same dimension); the last error is qbh_mf_kondo's."""
    want = _call("qbh_gen_kondo", *a, **k)
    got = _mf(*a, **k)
    assert got == want and got[0] == code, (got, want, code)
    assert "qbh_mf_kondo" in _err()
    return got


def test_shape_refusals():
    T = lambda n: kondo.terms(n, chain(n), 1.0, 1.1)
    _same_refusal(EINVAL, 0, 0, 0, kondo.Terms([], [1.0], [1.0], []))
    assert "n_sites" in _err()
    _same_refusal(EINVAL, 22, 22, 0, kondo.Terms([], [1.0] * 22, [1.0] * 22, []))
    assert "n_sites" in _err()
    _same_refusal(EINVAL, 4, -1, 1, T(4))
    assert "n_elec" in _err()
    _same_refusal(EINVAL, 4, 9, 1, T(4))
    assert "n_elec" in _err()
    _same_refusal(EINVAL, 4, 4, 1, T(4))                                  # 4 electrons + 4 spins: two_sz is even
    assert "odd" in _err()
    _same_refusal(EINVAL, 4, 3, 0, T(4))
    assert "odd" in _err()
    _same_refusal(EUNSUPP, 4, 4, 10, T(4))                                # right parity, |two_sz| beyond n_elec + n_sites
    assert "empty" in _err()
    assert _mf(4, 3, 1, T(4))[0] in OK_HERE
    dim = C.c_int64(0)
    assert _lib.lib().qbh_mf_kondo(None, 4, 4, 0, 0, None, None, None, 0.0, None, None, 0, None, None, None, 0, -1, C.byref(dim),
                                   None) == EINVAL


def test_term_refusals():
    L = 6
    good = kondo.terms(L, chain(L), 1.0, 1.1, 0.2)
    _same_refusal(EINVAL, L, L, 0, good._replace(hops=good.hops + [(0, L, -1.0, -1.0)]))
    assert "outside the lattice" in _err()
    _same_refusal(EINVAL, L, L, 0, good._replace(sbonds=good.sbonds + [(2, 2, 1.0, 1.0)]))
    assert "two different sites" in _err()
    # a one-way hop, and a flux whose return amplitude is not the conjugate
    _same_refusal(ENOTHERM, L, L, 0, good._replace(hops=[(i, (i + 1) % L, -1.0, -1.0) for i in range(L)]))
    assert "Hermitian" in _err()
    ph = np.exp(0.3j)
    _same_refusal(ENOTHERM, L, L, 0,
                  good._replace(hops=[h for i in range(L) for h in ((i, (i + 1) % L, -ph, -ph), ((i + 1) % L, i, -ph, -ph))]))
    ok = good._replace(hops=[h for i in range(L) for h in ((i, (i + 1) % L, -ph, -ph), ((i + 1) % L, i, -np.conj(ph), -np.conj(ph)))])
    assert _mf(L, L, 0, ok)[0] in OK_HERE
    _same_refusal(ENOTHERM, L, L, 0, good._replace(hops=good.hops + [(1, 1, 0.5j, 0.0)]))     # an imaginary number operator


def test_bad_row_range_is_refused():
    T = kondo.terms(4, chain(4), 1.0, 4.0)
    assert _same_refusal(EINVAL, 4, 4, 0, T, rows=(0, 1000))[1] == 346
    for rows in ((-1, 5), (5, 5), (7, 3), (346, -1), (0, 347)):
        rc, dim = _mf(4, 4, 0, T, rows=rows)
        assert rc == EINVAL and dim == 346 and "row range" in _err(), rows


def test_the_limits_of_the_stored_form_are_not_refused():
    """dim >= 2^31 and a worst row above 160 entries pass every check: the call gets as far as looking for the device."""
    T = kondo.terms(13, chain(13))
    rc, dim = _call("qbh_gen_kondo", 13, 13, 0, T)
    assert rc == EUNSUPP and "int32" in _err()
    rc, dim = _mf(13, 13, 0, T, rows=(15_000_000_000, 15_000_004_096))
    assert rc in OK_HERE and dim == 15_148_345_760 == kondo.sector_dim(13, 13, 0)
    # all-to-all hops on 13 sites: 2 * 78 + 13 + 1 = 170 entries in the worst row
    bonds = [(i, j) for i in range(13) for j in range(i + 1, 13)]
    dense = kondo.terms(13, bonds, 1.0, 1.1)
    assert _call("qbh_gen_kondo", 13, 2, 1, dense)[0] == EUNSUPP and "a row may hold 170" in _err()
    assert _mf(13, 2, 1, dense)[0] in OK_HERE


def test_a_valid_call_without_a_device_fails_loudly():
    if _lib.lib().qbh_device_count() > 0:
        return                               # a GPU is present: tests/test_gpu_kondo_mf.py covers the call
    T = kondo.terms(6, chain(6), 1.0, 1.1, 0.3)
    got = _mf(6, 5, 1, T, U=2.0, rows=(10, 200))
    assert got == _call("qbh_gen_kondo", 6, 5, 1, T, U=2.0, rows=(10, 200)) == (ENODEVICE, kondo.sector_dim(6, 5, 1))
    assert "no HIP device" in _err()


@pytest.mark.parametrize("shape", [(6, 6, 0), (6, 5, -1), (3, 6, -1), (5, 6, -1)])
def test_rank_and_unrank_agree_with_the_enumerated_words(shape):
    n = shape[0]
    w = kondo.words(*shape)
    assert len(w) == kondo.sector_dim(*shape) > 0
    for r, word in enumerate(w):
        u, d, s = kondo.unrank(*shape, r)
        assert u | (d << n) | (s << (2 * n)) == int(word), r
        assert kondo.rank(*shape, u, d, s) == r
    fu, fd, fs = kondo.fields(w, n)
    assert [kondo.rank(*shape, a, b, c) for a, b, c in zip(fu[::7], fd[::7], fs[::7])] == list(range(0, len(w), 7))


def test_unrank_beyond_the_enumerable_sizes():
    shape = (13, 13, 0)
    dim = kondo.sector_dim(*shape)
    assert dim == 15_148_345_760
    u, d, s = kondo.unrank(*shape, dim - 1)
    assert s == (1 << 13) - 1 and bin(u).count("1") == 13 and d == 0          # the last word: every local spin down, all electrons up
    assert kondo.rank(*shape, u, d, s) == dim - 1
    assert kondo.unrank(*shape, 0) == (0, (1 << 13) - 1, 0)
    prev = -1
    for r in (0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 33 + 12345, 15_000_000_000, dim - 2):
        u, d, s = kondo.unrank(*shape, r)
        n_up = bin(u).count("1")
        assert n_up + bin(d).count("1") == 13 and (n_up - bin(d).count("1")) + (13 - 2 * bin(s).count("1")) == 0
        assert kondo.rank(*shape, u, d, s) == r
        word = u | (d << 13) | (s << 26)
        assert word > prev                                                     # ascending words
        prev = word
