"""CPU tier of tests/csrforms.py: the long-double reference against exact sums, the geometry mirror's buckets and coverage, the
error bounds.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

import csrforms as cf


def _F(v):
    """Exact Fraction of a long double (two doubles hold its 64-bit mantissa)."""
    v = np.longdouble(v)
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - np.longdouble(hi)))


@pytest.mark.parametrize("case", [("n63", "complex"), ("n65", "real"), ("n2", "complex"), ("sym_rand", "few")])
def test_reference_row_sums_match_exact_fractions(case):
    d = cf.make(*case)
    ia, ja, val = d["full"]
    n = min(d["n"], 80)
    ia = ia[:n + 1]
    x = cf.probe_vector(d["n"], 7)
    s, abs_s = cf.row_sums(ia, ja, val, x, chunk=64)        # small chunks: the chunk seams are exercised too
    exact = cf.exact_row_sums(ia, ja, val, x)
    for i, (re, im) in enumerate(exact):
        tol = Fraction(float(abs_s[i])) * Fraction(1, 2 ** 60) + Fraction(1, 2 ** 1000)
        assert abs(_F(s[i].real) - re) <= tol and abs(_F(s[i].imag) - im) <= tol, i
        # |a||x| sums are an upper bound of the modulus of the row sum
        assert float(abs_s[i]) >= abs(complex(float(s[i].real), float(s[i].imag))) * (1 - 1e-15)


def test_reference_epilogue_and_reductions_match_exact_fractions():
    d = cf.make("n63", "few")
    ia, ja, val = d["full"]
    x, y0 = cf.probe_vector(63, 1), cf.probe_vector(63, 2)
    s, abs_s = cf.row_sums(ia, ja, val, x)
    ex = cf.exact_row_sums(ia, ja, val, x)
    alpha, beta, gamma = 0.7, -1.3, 1.75
    ref = cf.epilogue(s, abs_s, np.diff(ia), x, y0, alpha, beta, gamma)
    F = Fraction
    dot_re = dot_im = nrm = F(0)
    for i, (re, im) in enumerate(ex):
        yr = F(alpha) * re + F(beta) * F(float(y0[i].real)) + F(gamma) * F(float(x[i].real))
        yi = F(alpha) * im + F(beta) * F(float(y0[i].imag)) + F(gamma) * F(float(x[i].imag))
        assert abs(_F(ref["y"][i].real) - yr) < F(1, 2 ** 58) and abs(_F(ref["y"][i].imag) - yi) < F(1, 2 ** 58)
        xr, xi = F(float(x[i].real)), F(float(x[i].imag))
        dot_re += xr * yr + xi * yi
        dot_im += xr * yi - xi * yr
        nrm += yr * yr + yi * yi
    assert abs(_F(ref["dot"].real) - dot_re) < F(1, 2 ** 54) and abs(_F(ref["dot"].imag) - dot_im) < F(1, 2 ** 54)
    assert abs(_F(ref["nrm"]) - nrm) < F(1, 2 ** 52)


def test_bounds_are_finite_and_nonzero_on_nonempty_rows():
    for case in [("empty_runs", "complex"), ("long_rows", "few"), ("const1", "real"), ("sym_wide", "complex")]:
        d = cf.make(*case)
        ia, ja, val = d["full"]
        x, y0 = cf.probe_vector(d["n"], 1), cf.probe_vector(d["n"], 2)
        s, abs_s = cf.row_sums(ia, ja, val, x)
        for a, b, g in [(1.0, 0.0, 0.0), (0.7, -1.3, 0.5)]:
            ref = cf.epilogue(s, abs_s, np.diff(ia), x, y0, a, b, g)
            e = ref["bound"]
            assert np.all(np.isfinite(e)) and np.all(e >= 0)
            nonempty = np.diff(ia) > 0
            assert np.all(e[nonempty] > 0), case
            # far below any single term (|a_ij| |x_j| >= 0.25): a dropped or doubled term cannot hide
            assert np.all(e[nonempty] < 1e-6 * 0.25 * abs(a))
            assert 0 < float(ref["t_dot"]) < 1e-6 * float(np.sum(np.abs(x) * np.abs(ref["y"]))) + 1e-300
            assert 0 < float(ref["t_nrm"]) < 1e-6 * float(ref["nrm"])


@pytest.mark.parametrize("name,kernel,vd,npb,key", [
    ("const1", cf.KERNEL_STREAM, 0, 0, ("stream", 2048, 1, 0)),
    ("const6", cf.KERNEL_STREAM, 1, 1024, ("stream", 1024, 2, 0)),     # every value distinct: not coded
    ("const20", cf.KERNEL_STREAM, 0, 4096, ("stream", 4096, 4, 0)),
    ("const80", cf.KERNEL_STREAM, 0, 0, ("stream", 2048, 8, 0)),
    ("const200", cf.KERNEL_STREAM, 0, 0, ("stream", 2048, 16, 0)),
    ("const20", cf.KERNEL_VECTOR, 0, 0, ("vector", 2, 0)),
    ("const40", cf.KERNEL_VECTOR, 0, 0, ("vector", 4, 0)),
    ("const112", cf.KERNEL_VECTOR, 0, 0, ("vector", 8, 0)),
    ("const400", cf.KERNEL_VECTOR, 0, 0, ("vector", 16, 0)),
    ("const1000", cf.KERNEL_VECTOR, 0, 0, ("vector", 32, 0)),
    ("const2100", cf.KERNEL_VECTOR, 0, 0, ("vector", 64, 0)),
    ("const6", cf.KERNEL_ROWS, 0, 0, ("rows", 2048, 1, 0)),
    ("const20", cf.KERNEL_ROWS, 0, 0, ("rows", 2048, 4, 0)),
    ("const112", cf.KERNEL_ROWS, 0, 0, ("rows", 2048, 8, 0)),
    ("const112", cf.KERNEL_ROWS, 1, 0, ("rows", 2048, 8, 0)),     # 134400 distinct values: more than 2-byte codes hold
    ("const6", cf.KERNEL_WAVE, 0, 0, ("wave", 2, 0)),
    ("const40", cf.KERNEL_WAVE, 0, 0, ("wave", 4, 0)),
    ("const80", cf.KERNEL_WAVE, 0, 0, ("wave", 8, 0)),
    ("const200", cf.KERNEL_WAVE, 0, 0, ("wave", 16, 0)),
])
def test_profiles_land_in_the_bucket_the_mirror_claims(name, kernel, vd, npb, key):
    d = cf.make(name, "complex")
    ia, _, val = d["full"]
    r = cf.route(kernel, vd, ia, val, npb_opt=npb)
    assert r["key"] == key


@pytest.mark.parametrize("kind,kernel,vd,dict_mode,info_kernel", [
    ("few", cf.KERNEL_WAVE, 1, 1, cf.KERNEL_ROWS),       # value_dict = 1 turns WAVE into the coded row kernel
    ("mid", cf.KERNEL_WAVE, 1, 2, cf.KERNEL_ROWS),
    ("many", cf.KERNEL_ROWS, 1, 3, cf.KERNEL_ROWS),
    ("many", cf.KERNEL_ROWS, 2, 0, cf.KERNEL_ROWS),       # 1-byte codes only: > 256 values stay uncoded
    ("mid", cf.KERNEL_STREAM, 1, 0, cf.KERNEL_STREAM),    # stream / vector: <= 256 values only
    ("few", cf.KERNEL_VECTOR, 1, 1, cf.KERNEL_VECTOR),
    ("complex", cf.KERNEL_WAVE, 1, 3, cf.KERNEL_ROWS),    # 59980 distinct values still fit 2-byte codes
])
def test_coding_mirror(kind, kernel, vd, dict_mode, info_kernel):
    d = cf.make("const20", kind)
    ia, _, val = d["full"]
    r = cf.route(kernel, vd, ia, val)
    assert (r["dict_mode"], r["info_kernel"]) == (dict_mode, info_kernel)


def test_sweep_covers_every_route_and_path():
    """The GPU sweep (test_gpu_csrforms.test_every_form_on_every_profile) runs exactly cf.sweep() per profile and asserts each
    route on the device: the union of what it reaches must be every template instance and block path the mirror enumerates."""
    keys, paths = set(), set()
    for name, kind in cf.all_profile_cases():
        d = cf.make(name, kind)
        ia, _, val = d["full"]
        for f, r in cf.sweep(ia, val):
            keys.add(r["key"])
            paths |= cf.paths(r, ia)
    assert cf.all_routes() - keys == set()
    assert cf.ALL_PATHS - paths == set()


def test_walk_mirror():
    # 8 workgroups, one per XCD: each walks all of its eighth, whatever the map
    for swz in (0, 1, 2):
        assert cf.walk_counts(100, 8, swz).sum() == 100
    # every block is visited exactly once for any grid
    for swz in (0, 1, 2, 3):
        for g in (8, 16, 24, 64, 4096):
            assert cf.walk_counts(1000, g, swz).sum() == 1000
    r = cf.route(cf.KERNEL_WAVE, 0, np.arange(8_000_001, dtype=np.int64) * 8, np.ones(1), wave_walk=3, nd=1)
    assert r["walk"] == 3 and r["key"] == ("wave", 2, 1) and cf.min_walk(r) >= 2
    r = cf.route(cf.KERNEL_WAVE, 0, np.arange(8_000_001, dtype=np.int64) * 8, np.ones(1), xcd_swizzle=3, deterministic=1, nd=1)
    assert r["walk"] == 2 and r["key"] == ("wave", 2, 0)
