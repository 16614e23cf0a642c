"""CPU checks of the matrix-free d-level operator qbh_mf_qudit: the C ABI declares and exports it, and every argument and term
check that tests/test_qudit_cpu.py exercises for qbh_gen_qudit returns the same code from it before the device is looked for.
The limits of the stored form that it drops (int32 columns, 240 entries per row) are not refused."""
import ctypes as C
import os
import re

import numpy as np

from quantum_basis_amd import _lib, qudit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE, ENOTHERM, EUNSUPP = -1, -2, -5, -9


def test_header_declares_and_library_exports_qbh_mf_qudit():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qbhip.h")).read(), flags=re.S)
    assert re.search(r"\bqbh_mf_qudit\s*\(", text)
    assert "qbh_mf_qudit" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "qbh_mf_qudit")


def _call(name, n_sites, d, total, pairs=(), singles=(), rows=(0, -1)):
    """Call qbh_gen_qudit or qbh_mf_qudit on host arrays; returns (rc, dim_out)."""
    ps = np.ascontiguousarray(np.array([(p[0], p[1]) for p in pairs], dtype=np.int32).reshape(-1, 2))
    pm = np.ascontiguousarray(np.array([np.asarray(p[2], dtype=np.complex128) for p in pairs], dtype=np.complex128).reshape(-1))
    ss = np.ascontiguousarray(np.array([s[0] for s in singles], dtype=np.int32))
    sd = np.ascontiguousarray(np.array([s[1] for s in singles], dtype=np.float64).reshape(-1))
    h = C.c_void_p()
    dim = C.c_int64(-1)
    rc = getattr(_lib.lib(), name)(C.byref(h), n_sites, d, total, len(pairs), ps.ctypes.data, pm.ctypes.data, len(singles),
                                   ss.ctypes.data, sd.ctypes.data, rows[0], rows[1], C.byref(dim), None)
    assert rc != 0 or h.value
    if rc == 0:
        _lib.lib().qbh_csr_destroy(h)
    return rc, dim.value


def _mf(*a, **k):
    return _call("qbh_mf_qudit", *a, **k)


def _err():
    return _lib.lib().qbh_last_error().decode()


def _same_refusal(code, *a, **k):
    """Both entry points refuse the call with `code` (and report the same dimension); the last error is qbh_mf_qudit's."""
    want = _call("qbh_gen_qudit", *a, **k)
    got = _mf(*a, **k)
    assert got == want and got[0] == code, (got, want, code)
    return got


def test_d_out_of_range_and_shape():
    _same_refusal(EUNSUPP, 4, 9, 4)
    assert "at most 8" in _err()
    _same_refusal(EINVAL, 4, 1, 0)
    _same_refusal(EINVAL, 0, 3, 0)
    _same_refusal(EUNSUPP, 22, 5, 20)                                          # 22 sites x 3 bits
    assert "64 bits" in _err()
    _same_refusal(EINVAL, 4, 3, 9)                                             # charge above n (d - 1)
    _same_refusal(EINVAL, 4, 3, -1)
    L = _lib.lib()
    dim = C.c_int64(0)
    assert L.qbh_mf_qudit(None, 4, 3, 4, 0, None, None, 0, None, None, 0, -1, C.byref(dim), None) == EINVAL


def test_charge_violating_pair_is_einval():
    M = np.zeros((9, 9), dtype=np.complex128)
    M[1 * 3 + 1, 0 * 3 + 1] = 1.0            # |0 1> -> |1 1>: charge 1 -> 2
    M[0 * 3 + 1, 1 * 3 + 1] = 1.0
    _same_refusal(EINVAL, 4, 3, 4, [(0, 1, M)])
    assert "charge" in _err() and "qbh_mf_qudit" in _err()


def test_non_hermitian_merged_pair_is_enotherm():
    sz, sp, sm = qudit.spin_matrices(1)
    M = np.kron(sp, sm)                      # S+_i S-_j alone is not Hermitian
    _same_refusal(ENOTHERM, 4, 3, 4, [(0, 1, M)])
    assert _mf(4, 3, 4, [(0, 1, M), (1, 0, M)])[0] in (0, ENODEVICE)          # Hermitian once (1, 0) is transposed and merged
    assert _mf(4, 3, 4, [(0, 1, np.kron(sp, sm)), (0, 1, np.kron(sm, sp))])[0] in (0, ENODEVICE)
    D = np.zeros((9, 9), dtype=np.complex128)
    D[4, 4] = 1j                             # an imaginary diagonal
    _same_refusal(ENOTHERM, 4, 3, 4, [(0, 1, D)])


def test_bad_sites_and_too_many_pairs():
    M = qudit.heisenberg_terms(1, [(0, 1)])[0][2]
    _same_refusal(EINVAL, 4, 3, 4, [(0, 4, M)])                                # site out of range
    _same_refusal(EINVAL, 4, 3, 4, [(2, 2, M)])
    _same_refusal(EINVAL, 4, 3, 4, [(-1, 2, M)])
    _same_refusal(EINVAL, 4, 3, 4, singles=[(5, np.zeros(3))])
    many = [(i, j) for i in range(50) for j in range(i + 1, 50)][:1100]
    _same_refusal(EUNSUPP, 50, 2, 25, [(i, j, np.eye(4)) for i, j in many])
    assert "1024" in _err()


def test_bad_row_range_is_refused():
    M = qudit.heisenberg_terms(1, [(0, 1)])[0][2]
    assert _same_refusal(EINVAL, 4, 3, 4, [(0, 1, M)], rows=(0, 100))[1] == 19
    for rows in ((-1, 5), (5, 5), (7, 3), (19, -1), (0, 20)):
        rc, dim = _mf(4, 3, 4, [(0, 1, M)], rows=rows)
        assert rc == EINVAL and dim == 19 and "row range" in _err(), rows


def test_the_limits_of_the_stored_form_are_not_refused():
    """dim >= 2^31 and a worst row above 240 entries pass every check: the call gets as far as looking for the device."""
    M = qudit.heisenberg_terms(1, [(0, 1)])[0][2]
    bonds = [(i, (i + 1) % 22) for i in range(22)]
    rc, dim = _mf(22, 3, 22, [(i, j, M) for i, j in bonds], rows=(3_000_000_000, 3_000_004_096))
    assert rc in (0, ENODEVICE) and dim == qudit.qudit_dim(22, 3, 22) == 3_241_135_527
    Mk = qudit.heisenberg_terms(1, [(0, 1)], K=0.5)[0][2]
    dense = [(i, j, Mk) for i in range(16) for j in range(i + 1, 16)]         # 120 pairs x 2 + 1 > 240
    assert _call("qbh_gen_qudit", 16, 3, 16, dense)[0] == EUNSUPP
    assert _mf(16, 3, 16, dense, rows=(1000, 5000))[0] in (0, ENODEVICE)


def test_a_valid_call_without_a_device_fails_loudly():
    if _lib.lib().qbh_device_count() > 0:
        return                               # a GPU is present: tests/test_gpu_qudit_mf.py covers the call
    M = qudit.heisenberg_terms(1, [(0, 1)])[0][2]
    got = _mf(4, 3, 4, [(0, 1, M), (1, 2, M)], singles=[(0, np.ones(3))])
    assert got == _call("qbh_gen_qudit", 4, 3, 4, [(0, 1, M), (1, 2, M)], singles=[(0, np.ones(3))]) == (ENODEVICE, 19)
    assert "no HIP device" in _err()


def test_row_capacity_241_and_the_largest_sector_are_accepted():
    """A longest row of 241 entries (240 pairs at d = 2) is QBH_EUNSUPP from qbh_gen_qudit and passes qbh_mf_qudit's checks.
    qbh_mf_qudit refuses dim >= 2^62, but no shape that packs into 64 bits has such a sector: the largest, C(64, 32) for 64 sites
    of 2 levels, is 1.83e18 < 2^62 = 4.61e18 (the other widths hold 4^32 and 8^21 words in all, their largest sectors smaller still),
    so the refusal cannot be reached through the interface and the largest sector is accepted."""
    X = np.zeros((4, 4))
    X[1, 2] = X[2, 1] = 0.5
    sites = [(i, j) for i in range(64) for j in range(i + 1, 64)][:240]
    assert _call("qbh_gen_qudit", 64, 2, 63, [(i, j, X) for i, j in sites])[0] == EUNSUPP
    assert _mf(64, 2, 63, [(i, j, X) for i, j in sites])[0] in (0, ENODEVICE)
    shapes = [(d, n) for d in range(2, 9) for n in (64 // (1 if d <= 2 else 2 if d <= 4 else 3),)]
    largest = max(qudit.qudit_dim(n, d, n * (d - 1) // 2) for d, n in shapes)
    assert largest == qudit.qudit_dim(64, 2, 32) == 1832624140942590534 < 2 ** 62
    rc, dim = _mf(64, 2, 32, [(0, 63, X)], rows=(largest - 4096, largest))
    assert rc in (0, ENODEVICE) and dim == largest
