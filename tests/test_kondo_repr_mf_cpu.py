"""CPU checks of the matrix-free Kondo momentum sector qbh_mf_kondo_repr: the C ABI declares and exports it, a valid call
passes every check and then asks for the device (QBH_ENODEVICE = -2 here), every refusal of qbh_gen_kondo_repr comes back with
the same code from the same arguments, a row range that the word count excludes is refused, and the limit of 160 entries per
row of the stored form is not."""
import ctypes as C
import os
import re

import numpy as np

from quantum_basis_amd import _lib, kondo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE, ENOTHERM, EUNSUPP = -1, -2, -5, -9
OK_HERE = (0, ENODEVICE)                     # ok on a GPU box, no device here


def test_header_declares_and_library_exports_qbh_mf_kondo_repr():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qbhip.h")).read(), flags=re.S)
    assert re.search(r"\bqbh_mf_kondo_repr\s*\(", text)
    assert "qbh_mf_kondo_repr" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "qbh_mf_kondo_repr")
    assert _lib.lib().qbh_version() == 601


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def translations(L, n=None):
    n = L if n is None else n
    perms = np.array([[(s + t) % L for s in range(L)] for t in range(n)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * np.arange(n) / L)
    return perms, chars


def _call(name, n_sites, n_elec, two_sz, T, perms=None, chars=None, U=0.0, rows=(0, -1)):
    """qbh_gen_kondo_repr (whole sector) or qbh_mf_kondo_repr (rows) on host arrays; returns rc."""
    if perms is None:
        perms, chars = translations(n_sites)
    hops, sb = list(T.hops), list(T.sbonds)
    a = [np.ascontiguousarray(np.array([[h[0], h[1]] for h in hops], dtype=np.int32).reshape(-1, 2)),
         np.ascontiguousarray(np.array([h[2] for h in hops], dtype=np.complex128)),
         np.ascontiguousarray(np.array([h[3] for h in hops], dtype=np.complex128)),
         np.ascontiguousarray(T.kz, dtype=np.float64), np.ascontiguousarray(T.kxy, dtype=np.float64),
         np.ascontiguousarray(np.array([[b[0], b[1]] for b in sb], dtype=np.int32).reshape(-1, 2)),
         np.ascontiguousarray(np.array([b[2] for b in sb], dtype=np.float64)),
         np.ascontiguousarray(np.array([b[3] for b in sb], dtype=np.float64))]
    p = np.ascontiguousarray(perms, dtype=np.int32)
    c = np.ascontiguousarray(chars, dtype=np.complex128)
    h = C.c_void_p()
    dim = C.c_int64(-1)
    head = (C.byref(h), n_sites, n_elec, two_sz, len(hops), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, U,
            a[3].ctypes.data, a[4].ctypes.data, len(sb), a[5].ctypes.data, a[6].ctypes.data, a[7].ctypes.data, len(c), p.ctypes.data,
            c.ctypes.data, 100.0)
    if name == "qbh_gen_kondo_repr":
        rc = _lib.lib().qbh_gen_kondo_repr(*head, 0, 1, C.byref(dim), None)
    else:
        rc = _lib.lib().qbh_mf_kondo_repr(*head, rows[0], rows[1], C.byref(dim), None)
    assert rc != 0 or h.value
    if rc == 0:
        _lib.lib().qbh_csr_destroy(h)
    return rc


def _mf(*a, **k):
    return _call("qbh_mf_kondo_repr", *a, **k)


def _err():
    return _lib.lib().qbh_last_error().decode()


def _same_refusal(code, *a, **k):
    """Both entry points refuse the call with `code`, and each names itself in its message."""
    want = _call("qbh_gen_kondo_repr", *a, **k)
    assert "qbh_gen_kondo_repr" in _err()
    got = _mf(*a, **k)
    assert got == want == code, (got, want, code, _err())
    assert "qbh_mf_kondo_repr" in _err()


def ring_terms(n):
    return kondo.terms(n, chain(n), 1.0, 1.1)


def all_to_all_terms(n):
    """Hops between every pair of a ring of n sites with the amplitude -1/r of the ring distance r, both directions (Hermitian,
    translation invariant), and J_K = 1.1 on every site."""
    dist = lambda i, j: min((j - i) % n, (i - j) % n)
    hops = [(i, j, -1.0 / dist(i, j), -1.0 / dist(i, j)) for i in range(n) for j in range(n) if i != j]
    return kondo.Terms(hops, [1.1] * n, [1.1] * n, [])


def test_a_valid_call_passes_every_check():
    assert _mf(6, 6, 0, kondo.terms(6, chain(6), 1.0, 1.1, 0.3)) in OK_HERE
    assert _mf(6, 6, 0, ring_terms(6), U=2.0, rows=(10, 200)) in OK_HERE
    assert _mf(4, 3, 1, ring_terms(4)) in OK_HERE
    if _lib.lib().qbh_device_count() <= 0:
        assert _mf(6, 6, 0, ring_terms(6)) == ENODEVICE and "no HIP device" in _err()
        assert _call("qbh_gen_kondo_repr", 6, 6, 0, ring_terms(6)) == ENODEVICE


def test_null_output_is_einval():
    dim = C.c_int64(0)
    assert _lib.lib().qbh_mf_kondo_repr(None, 4, 4, 0, 0, None, None, None, 0.0, None, None, 0, None, None, None, 1, None, None, 100.0, 0,
                                        -1, C.byref(dim), None) == EINVAL


def test_bad_shape_and_parity_with_no_block():
    T = ring_terms
    _same_refusal(EINVAL, 0, 0, 0, kondo.Terms([], [1.0], [1.0], []), perms=[[0]], chars=[1.0])
    assert "n_sites" in _err()
    _same_refusal(EINVAL, 22, 22, 0, kondo.Terms([], [1.0] * 22, [1.0] * 22, []))
    assert "n_sites" in _err()
    _same_refusal(EINVAL, 4, -1, 1, T(4))
    _same_refusal(EINVAL, 4, 9, 1, T(4))
    assert "n_elec" in _err()
    _same_refusal(EINVAL, 4, 4, 1, T(4))                                   # 4 electrons + 4 spins: two_sz is even
    assert "odd" in _err()
    _same_refusal(EINVAL, 4, 3, 0, T(4))
    _same_refusal(EUNSUPP, 4, 4, 10, T(4))                                 # right parity, |two_sz| beyond n_elec + n_sites
    assert "empty" in _err()


def test_term_outside_the_lattice_and_non_hermitian_hops():
    L = 6
    good = kondo.terms(L, chain(L), 1.0, 1.1, 0.2)
    _same_refusal(EINVAL, L, L, 0, good._replace(hops=good.hops + [(0, L, -1.0, -1.0)]))
    assert "outside the lattice" in _err()
    _same_refusal(EINVAL, L, L, 0, good._replace(sbonds=good.sbonds + [(2, 2, 1.0, 1.0)]))
    assert "two different sites" in _err()
    _same_refusal(ENOTHERM, L, L, 0, good._replace(hops=[(i, (i + 1) % L, -1.0, -1.0) for i in range(L)]))     # one-way hops
    assert "Hermitian" in _err()
    ph = np.exp(0.3j)
    bad = good._replace(hops=[h for i in range(L) for h in ((i, (i + 1) % L, -ph, -ph), ((i + 1) % L, i, -ph, -ph))])
    _same_refusal(ENOTHERM, L, L, 0, bad)
    ok = good._replace(hops=[h for i in range(L) for h in ((i, (i + 1) % L, -ph, -ph), ((i + 1) % L, i, -np.conj(ph), -np.conj(ph)))])
    assert _mf(L, L, 0, ok) in OK_HERE
    _same_refusal(ENOTHERM, L, L, 0, good._replace(hops=good.hops + [(1, 1, 0.5j, 0.0)]))


def test_terms_that_are_not_translation_invariant_are_einval():
    L = 6
    good = kondo.terms(L, chain(L), 1.0, 1.1, 0.2)
    _same_refusal(EINVAL, L, L, 0, kondo.terms(L, chain(L)[:-1], 1.0, 1.1))                      # open chain
    assert "not invariant" in _err()
    _same_refusal(EINVAL, L, L, 0, good._replace(kxy=[1.1, 1.1, 1.1, 0.9, 1.1, 1.1]))
    assert "Kondo couplings" in _err()
    _same_refusal(EINVAL, L, L, 0, good._replace(sbonds=good.sbonds[:-1]))
    assert "local-spin bonds" in _err()
    _same_refusal(EINVAL, L, L, 0, good._replace(hops=good.hops + [(2, 2, 0.3, 0.3)]))           # a potential on one site
    assert "not invariant" in _err()


def test_bad_permutations_and_too_many_translations():
    L = 6
    good = kondo.terms(L, chain(L), 1.0, 1.1, 0.2)
    perms, chars = translations(L)
    p2 = perms.copy()
    p2[0] = p2[1]                            # translation 0 is not the identity
    _same_refusal(EINVAL, L, L, 0, good, p2, chars)
    assert "identity" in _err()
    p2 = perms.copy()
    p2[2, 0] = p2[2, 1]                      # two sites onto one
    _same_refusal(EINVAL, L, L, 0, good, p2, chars)
    assert "not a site permutation" in _err()
    p2 = perms.copy()
    p2[3, 0] = L                             # out of range
    _same_refusal(EINVAL, L, L, 0, good, p2, chars)
    # 65 translations (a ring of 13 walked five times round)
    p65, c65 = translations(13, 65)
    _same_refusal(EUNSUPP, 13, 13, 0, ring_terms(13), p65, c65)
    assert "65 translations" in _err()
    assert _mf(13, 13, 0, ring_terms(13), p65[:64], c65[:64]) in OK_HERE
    # a sector of 2^40 words or more cannot be enumerated
    _same_refusal(EUNSUPP, 16, 16, 0, ring_terms(16))
    assert "too large" in _err()


def test_bad_row_range_against_the_word_count_is_einval():
    """The ring of 4 sites at half filling, S^z = 0, has 346 words: these ranges lie in no sector of it."""
    L = 4
    assert kondo.sector_dim(L, L, 0) == 346
    for rows in ((-1, 5), (5, 5), (7, 3), (0, -2), (346, -1), (0, 347), (0, 100000)):
        rc = _mf(L, L, 0, ring_terms(L), rows=rows)
        assert rc == EINVAL and "row range" in _err() and "qbh_mf_kondo_repr" in _err(), rows
    assert _mf(L, L, 0, ring_terms(L), rows=(0, 5)) in OK_HERE
    assert _mf(L, L, 0, ring_terms(L), rows=(3, -1)) in OK_HERE
    # the chain L = 13 at half filling: 1.5e10 words, the size the full-sector handle was made for, passes every check
    assert kondo.sector_dim(13, 13, 0) >= 2 ** 31
    assert _mf(13, 13, 0, ring_terms(13)) in OK_HERE


def test_the_row_limit_of_the_stored_form_is_not_refused():
    """All-to-all hops on a ring: 2 moves per site pair + one Kondo flip per site + the diagonal.  12 sites count
    2 * 66 + 12 + 1 = 145 entries and the stored form takes them; 13 sites count 2 * 78 + 13 + 1 = 170 > 160: the stored call
    refuses them, the matrix-free call passes every check."""
    assert _call("qbh_gen_kondo_repr", 12, 2, 0, all_to_all_terms(12)) in OK_HERE
    assert _mf(12, 2, 0, all_to_all_terms(12)) in OK_HERE
    T = all_to_all_terms(13)
    assert _call("qbh_gen_kondo_repr", 13, 2, 11, T) == EUNSUPP and "a row may hold 170" in _err()
    assert _mf(13, 2, 11, T) in OK_HERE
    assert _mf(13, 2, 11, T, rows=(5, 60)) in OK_HERE
    if _lib.lib().qbh_device_count() <= 0:
        assert _mf(13, 2, 11, T) == ENODEVICE
    # the invariance check still applies to it: one pair stronger than its images
    bad = T._replace(hops=[(i, j, 2 * a if {i, j} == {0, 5} else a, b) for (i, j, a, b) in T.hops])
    assert _mf(13, 2, 11, bad) == EINVAL and "not invariant" in _err()
