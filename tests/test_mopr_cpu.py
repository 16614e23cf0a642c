"""CPU checks of the full-space operator-times-vector entry points qbh_mopr_spin_dev, qbh_mopr_onebody_dev and qbh_mopr_terms_dev:
every argument check comes before the device is looked for, so a refused call returns QBH_EINVAL (-1) with a message that names
the entry point, and a call that passes every check returns QBH_ENODEVICE (-2) on a machine without a device.  The vector
addresses are fake and never dereferenced.  Where there IS a device an accepted call would run its kernel on them (and over
C(64, 32) rows), so the accepted calls are made only without one; there the GPU suite (test_gpu_moprforms.py) makes accepted
calls with real vectors.  qbh_mopr_qudit_dev has its refusals in test_qudit_cpu.py."""
import ctypes as C
from math import comb

import numpy as np
import pytest

from quantum_basis_amd import _lib

EINVAL, ENODEVICE = -1, -2
FAKE = C.c_void_p(64)


def _L():
    return _lib.lib()


def _err():
    return _L().qbh_last_error().decode()


def _no_device():
    return _L().qbh_device_count() <= 0


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _refused(rc, who, *words):
    assert rc == EINVAL, (rc, _err())
    msg = _err()
    assert who in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _accepted(call):
    """call() passes every check: QBH_ENODEVICE here; not made where a device would run it on the fake addresses"""
    if not _no_device():
        print("a device is present: the accepted call is not made here (test_gpu_moprforms.py makes accepted calls with real vectors)")
        return
    rc = call()
    assert rc == ENODEVICE, (rc, _err())
    assert "no HIP device" in _err()


# ------------------------------------------------------------------------------------------------------- spin --
def _spin(n_sites=6, n_dn_old=3, kind=0, coef=True, vec_old=FAKE, vec_new=FAKE):
    c = np.ones(64, dtype=np.complex128) if coef else None
    return _L().qbh_mopr_spin_dev(n_sites, n_dn_old, kind, _p(c), vec_old, vec_new, None)


def test_spin_null_arguments():
    for kw in (dict(coef=False), dict(vec_old=None), dict(vec_new=None)):
        _refused(_spin(**kw), "qbh_mopr_spin_dev", "invalid argument")
    _accepted(lambda: _spin())


@pytest.mark.parametrize("kw", [dict(n_sites=0, n_dn_old=0), dict(n_sites=65, n_dn_old=3), dict(kind=2), dict(kind=-2), dict(n_dn_old=-1),
                                dict(n_dn_old=7), dict(n_dn_old=0, kind=+1), dict(n_dn_old=6, kind=-1),
                                dict(n_sites=40, n_dn_old=33, kind=0), dict(n_sites=40, n_dn_old=32, kind=-1),
                                dict(n_sites=40, n_dn_old=33, kind=+1)], ids=lambda kw: "_".join("%s%d" % (k[:4], v) for k, v in kw.items()))
def test_spin_refusals(kw):
    _refused(_spin(**kw), "qbh_mopr_spin_dev", "invalid argument")


@pytest.mark.parametrize("shape", [(64, 32, 0), (40, 31, -1), (40, 32, +1), (64, 1, +1), (1, 0, 0)])
def test_spin_accepted_at_the_limits(shape):
    n, nd, kind = shape
    _accepted(lambda: _spin(n_sites=n, n_dn_old=nd, kind=kind))


# ---------------------------------------------------------------------------------------------------- one-body --
def _onebody(n_sites=6, n_up=3, n_dn=2, n_terms=None, a=(0, 5), b=(1, 5), spin=(0, 1), w=True, vec_old=FAKE, vec_new=FAKE):
    arr = lambda v: None if v is None else np.asarray(v, dtype=np.int32)
    a, b, spin = arr(a), arr(b), arr(spin)
    wz = np.ones(8, dtype=np.complex128) if w else None
    nt = 2 if n_terms is None else n_terms
    return _L().qbh_mopr_onebody_dev(n_sites, n_up, n_dn, nt, _p(a), _p(b), _p(spin), _p(wz), vec_old, vec_new, None)


def test_onebody_null_arguments():
    for kw in (dict(a=None), dict(b=None), dict(spin=None), dict(w=False), dict(vec_old=None), dict(vec_new=None)):
        _refused(_onebody(**kw), "qbh_mopr_onebody_dev", "invalid argument")
    _accepted(lambda: _onebody())


@pytest.mark.parametrize("kw,word", [(dict(n_sites=32), "invalid argument"), (dict(n_sites=0, n_up=0, n_dn=0), "invalid argument"),
                                     (dict(n_terms=0), "invalid argument"), (dict(n_up=7), "invalid argument"), (dict(n_dn=7), "invalid argument"),
                                     (dict(n_up=-1), "invalid argument"), (dict(a=(0, 6)), "term 1"), (dict(b=(6, 5)), "term 0"),
                                     (dict(a=(-1, 5)), "term 0"), (dict(spin=(0, 2)), "term 1"), (dict(spin=(-1, 1)), "term 0")])
def test_onebody_refusals(kw, word):
    _refused(_onebody(**kw), "qbh_mopr_onebody_dev", word)


def test_onebody_accepted_at_31_sites():
    _accepted(lambda: _onebody(n_sites=31, n_up=1, n_dn=1, a=(30, 0), b=(0, 30)))
    _accepted(lambda: _onebody(n_sites=31, n_up=31, n_dn=0, a=(30, 0), b=(0, 30)))


# ------------------------------------------------------------------------------------------------------- terms --
class Terms:
    """qbh_mopr_terms_dev with valid defaults: S^+_0 S^-_1 + S^z_2 on (6, 3), resp. c^dag_{0,up} c_{1,up} + n_{2,down} on (6, 3, 2);
    keyword arguments replace single ones (None: a null pointer)"""

    def __init__(self, family):
        self.d = dict(family=family, n_sites=6, n_a=3, n_b=2 if family else 0, n_terms=None, term_ptr=[0, 2, 3], kind=[1, 2, 0], site=[0, 1, 2],
                      species=[0, 0, 1] if family else None, coef=True, vec_old=FAKE, vec_new=FAKE, dim=True)
        self.dim = C.c_int64(-1)

    def __call__(self, **kw):
        a = dict(self.d, **kw)
        arr = lambda v: None if v is None else np.asarray(v, dtype=np.int32)
        ptr, kind, site, sp = arr(a["term_ptr"]), arr(a["kind"]), arr(a["site"]), arr(a["species"])
        nt = a["n_terms"] if a["n_terms"] is not None else len(ptr) - 1
        coef = (np.ones(max(nt, 1), dtype=np.complex128) * (0.5 - 1j)) if a["coef"] else None
        self.dim = C.c_int64(-1)
        return _L().qbh_mopr_terms_dev(a["family"], a["n_sites"], a["n_a"], a["n_b"], nt, _p(ptr), _p(kind), _p(site), _p(sp), _p(coef),
                                          a["vec_old"], a["vec_new"], C.byref(self.dim) if a["dim"] else None, None)


WHO = "qbh_mopr_terms_dev"


@pytest.mark.parametrize("family", [0, 1])
def test_terms_null_arguments(family):
    call = Terms(family)
    for key in ("term_ptr", "kind", "site", "vec_old", "vec_new"):
        _refused(call(**{key: None, "n_terms": 2}), WHO, "invalid argument")
    _refused(call(coef=False), WHO, "invalid argument")
    if family == 1:
        _refused(call(species=None), WHO, "invalid argument")               # the fermions need the species of every factor
    else:
        _accepted(lambda: call(species=None))                                # the spins do not
    _accepted(lambda: call(dim=False))                                       # dim_new_out may be null
    _accepted(lambda: call())


@pytest.mark.parametrize("family", [0, 1])
def test_terms_shape_and_list_refusals(family):
    call = Terms(family)
    _refused(call(family=2), WHO, "invalid argument")
    _refused(call(family=-1), WHO, "invalid argument")
    for kw in (dict(n_sites=0), dict(n_sites=65 if family == 0 else 32), dict(n_a=-1), dict(n_a=7), dict(n_b=-1), dict(n_b=7), dict(n_terms=0),
               dict(term_ptr=[1, 2, 3])):
        _refused(call(**kw), WHO, "invalid argument")
    _refused(call(term_ptr=[0, 3, 2], n_terms=2), WHO, "not ascending")
    _refused(call(term_ptr=[0, 0], n_terms=1), WHO, "0 elementary factors")             # nothing but the identity
    _refused(call(kind=[1, 2, 3]), WHO, "factor 0 of term 1")
    _refused(call(kind=[1, -1, 0]), WHO, "factor 1 of term 0")
    _refused(call(site=[0, 6, 2]), WHO, "factor 1 of term 0")
    _refused(call(site=[-1, 1, 2]), WHO, "factor 0 of term 0")
    if family == 1:
        _refused(call(species=[0, 0, 2]), WHO, "factor 0 of term 1")
        _refused(call(species=[-1, 0, 1]), WHO, "factor 0 of term 0")


@pytest.mark.parametrize("family", [0, 1])
def test_terms_at_most_4096_factors(family):
    call = Terms(family)
    many = dict(term_ptr=list(range(4098)), kind=[0] * 4097, site=[s % 6 for s in range(4097)], species=[s % 2 for s in range(4097)] if family else None)
    _refused(call(**many), WHO, "4097 elementary factors", "4096")
    full = dict(term_ptr=list(range(4097)), kind=[0] * 4096, site=[s % 6 for s in range(4096)], species=[s % 2 for s in range(4096)] if family else None)
    _accepted(lambda: call(**full))
    four = dict(term_ptr=list(range(0, 4097, 4)), kind=[1, 2, 0, 0] * 1024, site=[0, 1, 2, 3] * 1024, species=[0] * 4096 if family else None)
    _accepted(lambda: call(**four))
    _refused(call(**dict(four, term_ptr=list(range(0, 4097, 4)) + [4097], kind=[1, 2, 0, 0] * 1024 + [0], site=[0, 1, 2, 3] * 1024 + [0],
                         species=[0] * 4097 if family else None)), WHO, "4097")


def test_terms_must_share_one_target_sector():
    # fermions: term 0 removes an up electron, term 1 a down electron
    _refused(Terms(1)(term_ptr=[0, 1, 2], kind=[2, 2], site=[0, 0], species=[0, 1]), WHO, "term 1", "(0, -1)", "(-1, 0)", "one target sector")
    # spins: S^- adds a down spin, S^+ removes one
    _refused(Terms(0)(term_ptr=[0, 1, 2], kind=[2, 1], site=[0, 0]), WHO, "term 1", "(-1, 0)", "(1, 0)")
    _refused(Terms(0)(term_ptr=[0, 1, 1], kind=[2], site=[0]), WHO, "term 1", "(0, 0)", "(1, 0)")        # ... and the identity none


def test_terms_target_sector_must_exist():
    one = lambda kind, sp=0: dict(term_ptr=[0, 1], kind=[kind], site=[0], species=[sp])
    _refused(Terms(0)(n_a=0, **dict(one(1), species=None)), WHO, "(-1, 0)", "does not exist")            # S^+ out of no down spin
    _refused(Terms(0)(n_a=6, **dict(one(2), species=None)), WHO, "(7, 0)", "does not exist")
    _refused(Terms(1)(n_a=0, **one(2)), WHO, "(-1, 2)", "does not exist")
    _refused(Terms(1)(n_a=6, **one(1)), WHO, "(7, 2)", "does not exist")
    _refused(Terms(1)(n_b=0, **one(2, 1)), WHO, "(3, -1)", "does not exist")
    _refused(Terms(1)(n_b=6, **one(1, 1)), WHO, "(3, 7)", "does not exist")
    # 33 down spins on either side of a spin operator
    sz = dict(term_ptr=[0, 1], kind=[0], site=[39], species=None)
    _refused(Terms(0)(n_sites=40, n_a=33, **sz), WHO, "does not exist")
    _refused(Terms(0)(n_sites=40, n_a=32, **dict(sz, kind=[2])), WHO, "does not exist")
    _refused(Terms(0)(n_sites=40, n_a=33, **dict(sz, kind=[1])), WHO, "does not exist")
    for n_a, kind in ((32, 0), (31, 2), (32, 1)):
        _accepted(lambda: Terms(0)(n_sites=40, n_a=n_a, **dict(sz, kind=[kind])))


DIM_CASES = [
    # family, n_sites, n_a, n_b, terms as lists of (kind, site, species), dimension of the target sector
    (0, 6, 3, 0, [[(1, 0, 0), (2, 5, 0)], [(0, 0, 0)]], comb(6, 3)),
    (0, 6, 3, 0, [[(2, 0, 0)], [(2, 5, 0)]], comb(6, 4)),                        # S^- adds a down spin
    (0, 64, 2, 0, [[(1, 0, 0)], [(1, 63, 0)]], 64),                             # S^+ removes one
    (0, 64, 32, 0, [[(1, 0, 0), (2, 63, 0)], [(0, 31, 0)]], comb(64, 32)),
    (0, 64, 31, 0, [[(2, 63, 0)]], comb(64, 32)),
    (0, 1, 0, 0, [[(0, 0, 0)]], 1),
    (1, 6, 3, 2, [[(1, 0, 0), (2, 5, 0)], [(0, 2, 1)]], comb(6, 3) * comb(6, 2)),
    (1, 6, 3, 2, [[(2, 0, 0)], [(2, 5, 0)]], comb(6, 2) * comb(6, 2)),
    (1, 6, 3, 2, [[(1, 0, 0), (2, 0, 1)], [(1, 5, 0), (2, 5, 1)]], comb(6, 4) * comb(6, 1)),
    (1, 31, 15, 16, [[(1, 30, 0), (2, 0, 0)], [(0, 30, 1)]], comb(31, 15) * comb(31, 16)),
    (1, 31, 0, 31, [[(1, 0, 0)], [(1, 30, 0)]], 31),
    (1, 8, 8, 1, [[(2, 7, 0)]], 8 * 8),
]


@pytest.mark.parametrize("case", DIM_CASES, ids=lambda c: "f%d_n%d_a%d_b%d_to%d" % (c[0], c[1], c[2], c[3], c[5]))
def test_terms_accepted_calls_report_the_dimension(case):
    """the dimension of the target sector is the caller's before the device is looked for: a binomial for the spins (up to 64
    sites), a product of two for the fermions (up to 31)"""
    family, n, n_a, n_b, tm, dim = case
    flat = [f for fs in tm for f in fs]
    call = Terms(family)
    kw = dict(n_sites=n, n_a=n_a, n_b=n_b, term_ptr=list(np.cumsum([0] + [len(fs) for fs in tm])), kind=[f[0] for f in flat],
              site=[f[1] for f in flat], species=[f[2] for f in flat] if family else None)
    _accepted(lambda: call(**kw))
    if _no_device():
        assert call.dim.value == dim


def test_terms_refuses_32_sites_of_fermions_and_takes_64_of_spins():
    _refused(Terms(1)(n_sites=32), WHO, "invalid argument")
    _accepted(lambda: Terms(1)(n_sites=31, site=[0, 30, 30]))
    _accepted(lambda: Terms(0)(n_sites=64, site=[0, 63, 63]))
    _refused(Terms(0)(n_sites=64, site=[0, 64, 63]), WHO, "factor 1 of term 0")
