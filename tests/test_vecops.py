"""CPU half of the vector-kernel suite: the driver compiles and links, the helpers of tests/vecops.py agree with independent
statements of the same thing, and every comparison rule rejects a correct result with one fault injected at the largest
size the GPU tests use."""
import subprocess

import numpy as np
import pytest

import vecops as vo
from oracle import qb_oracle as qo

TILE_SHAPES = [(S, NU, 8) for S, NU in [(8, 1), (9, 1), (15, 7), (16, 8), (17, 9), (8, 64), (12, 100), (70, 70), (255, 33), (256, 8), (265, 17)]]
TILE_SHAPES += [(S, NU, B) for S, NU in [(16, 1), (17, 5), (31, 5), (33, 70), (70, 70)] for B in (16, 8)]
NMAX = 1310731            # largest streaming size
NBIG_KRYLOV = 524289      # largest size of the multi-dot / multi-axpy cases
NBIG_ROTATE = 262145      # largest size of the rotation cases


def test_driver_compiles_links_and_fails_loudly_without_gpu():
    exe = vo.driver()
    import torch
    if torch.cuda.is_available():
        return                                               # with a device only the build is checked here; the GPU tests run the program
    p = subprocess.run([exe, "none", "none", "none"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 3 and "no HIP device" in p.stdout


@pytest.mark.parametrize("S,NU,B", TILE_SHAPES)
def test_tile_map_is_krontile_and_a_bijection(S, NU, B):
    tm = vo.tile_map(S, NU, B)
    assert np.array_equal(tm, vo.tile_map_formula(S, NU, B))
    assert np.array_equal(np.sort(tm), np.arange(S * NU))


@pytest.mark.parametrize("seed", [1, 8])
def test_lehmer_stream_normalised_is_the_oracles_start_vector(seed):
    n = 4099
    v = vo.lehmer_stream(n, seed).astype(vo.LD)
    want = v / np.sqrt(np.sum(v * v))
    got = qo.vec_randomize(n, seed)
    assert np.all(got.imag == 0.0)
    # the oracle's norm is a double sum of n squares (relative error <= n u / 2 after the root), then one division and one product
    assert np.max(np.abs(got.real.astype(vo.LD) - want) / np.abs(want)) <= (n / 2 + 4) * vo.U
    assert vo.exact(vo.lehmer_stream(5, seed, offset=3), vo.lehmer_stream(8, seed)[3:])
    inv = np.array([2, 0, 1], dtype=np.int32)
    full = vo.lehmer_stream(12, seed)
    assert vo.exact(vo.lehmer_stream(12, seed, major_inv=inv, S=4), np.concatenate([full[8:12], full[0:4], full[4:8]]))


# ---- teeth: a correct result passes, the same result with one fault does not
def test_reduction_rule_rejects_one_dropped_element():
    g = vo.rng(3)
    x, y = vo.cvec(g, NMAX), vo.cvec(g, NMAX)
    nparts = vo.blas_grid(NMAX)
    (re, im), (sre, sim) = vo.ref_dotc(x, y)
    tre = x.real * y.real + x.imag * y.imag
    tim = x.real * y.imag - x.imag * y.real
    for t, ref, sa in ((tre, re, sre), (tim, im, sim), (np.abs(x) ** 2, vo.ref_nrm2sq(x), float(vo.ref_nrm2sq(x)))):
        assert vo.reduction_ratio(float(np.sum(t)), ref, NMAX, nparts, sa) <= 1.0
        for at in (0, NMAX // 2, NMAX - 1):                  # the last element is the one of the uneven third trip
            assert vo.reduction_ratio(vo.drop_one_from_sum(t, at), ref, NMAX, nparts, sa) > 1.0
    assert vo.reduction_ratio(float("nan"), re, NMAX, nparts, sre) > 1.0          # a partial sum nobody wrote


def test_elementwise_rule_rejects_one_dropped_term():
    g = vo.rng(4)
    x, y, alpha = vo.cvec(g, NMAX), vo.cvec(g, NMAX), complex(0.7109375, -0.4140625)
    ref, sa = vo.ref_axpy(alpha, x, y)
    good = y + alpha * x
    assert vo.elementwise_ratio(good, ref, 4, sa) <= 1.0
    for at in (0, NMAX - 1):
        bad = good.copy()
        bad[at] = y[at] + complex(alpha.real * x[at].real, alpha.real * x[at].imag + alpha.imag * x[at].real)     # one product of four left out
        assert vo.elementwise_ratio(bad, ref, 4, sa) > 1.0
        bad = good.copy()
        bad[at] = complex(np.nan, np.nan)                    # not written at all
        assert vo.elementwise_ratio(bad, ref, 4, sa) > 1.0


def test_krylov_rules_reject_a_basis_vector_left_out():
    g = vo.rng(5)
    n, nv = NBIG_KRYLOV, 8
    V, w, c = np.stack([vo.cvec(g, n) for _ in range(nv)]), vo.cvec(g, n), vo.cvec(g, nv)
    nparts = vo.blas_grid(n)
    dots = vo.ref_multi_dot(V, w)
    good = np.conj(V) @ w
    for i in range(nv):
        (re, im), (sre, sim) = dots[i]
        assert vo.reduction_ratio(good[i].real, re, n, nparts, sre) <= 1.0 and vo.reduction_ratio(good[i].imag, im, n, nparts, sim) <= 1.0
        # vector i dropped: its two components come back as 0
        assert max(vo.reduction_ratio(0.0, re, n, nparts, sre), vo.reduction_ratio(0.0, im, n, nparts, sim)) > 1.0
    ref, sa = vo.ref_multi_axpy(V, c, w)[nv - 1]
    good = w - c @ V
    assert vo.elementwise_ratio(good, ref, 4 * nv, sa) <= 1.0
    for i in (0, nv - 1):
        assert vo.elementwise_ratio(good + c[i] * V[i], ref, 4 * nv, sa) > 1.0
        one = good.copy()
        one[n - 1] += c[i] * V[i, n - 1]                     # left out for the single element of the second trip
        assert vo.elementwise_ratio(one, ref, 4 * nv, sa) > 1.0


@pytest.mark.parametrize("n,m,keep", [(4900, 64, 63), (NBIG_ROTATE, 2, 1)])
def test_rotation_rule_rejects_one_dropped_term_and_a_touched_column(n, m, keep):
    """the rule is per element, so the widest basis at a small size and the largest size with a basis of two show all of it:
    the fault sits in the last element, the single one of the second trip at the largest size"""
    g = vo.rng(6)
    V, S = np.stack([vo.cvec(g, n) for _ in range(m)]), vo.rvec(g, m * keep)
    ref, sa = vo.ref_rotate(V, S, keep)
    good = S.reshape(keep, m) @ V
    assert vo.elementwise_ratio(good, ref, 2 * m, sa) <= 1.0
    bad = good.copy()
    bad[keep - 1, n - 1] -= S[(keep - 1) * m + m - 1] * V[m - 1, n - 1]
    assert vo.elementwise_ratio(bad, ref, 2 * m, sa) > 1.0
    touched = V[keep:].copy()
    touched[0, n - 1] = complex(touched[0, n - 1].real, np.nextafter(touched[0, n - 1].imag, 2.0))
    assert vo.exact(V[keep:].copy(), V[keep:]) and not vo.exact(touched, V[keep:])


@pytest.mark.parametrize("S,NU,B", [(265, 17, 8), (70, 70, 16)])
def test_tiled_rule_rejects_two_exchanged_elements_of_the_last_band(S, NU, B):
    g = vo.rng(7)
    y = vo.cvec(g, S * NU)
    tm = vo.tile_map(S, NU, B)
    yt = np.empty_like(y)
    yt[tm] = y
    assert vo.tiled_exact(yt, y, tm)
    last = S * NU - 1                                        # the narrow last band ends the tiled copy
    assert tm[last] == last
    assert not vo.tiled_exact(vo.exchange_two(yt, last, last - 1), y, tm)
    assert not vo.tiled_exact(vo.exchange_two(yt, 0, 1), y, tm)
    neg0 = yt.copy()
    neg0[3] = complex(neg0[3].real, -0.0) if neg0[3].imag == 0 else -neg0[3]
    assert not vo.tiled_exact(neg0, y, tm)


def test_exact_rule_sees_one_ulp_the_sign_of_zero_and_the_sentinel():
    v = vo.lehmer_stream(4099, 8, offset=2147483645)
    assert vo.exact(v.copy(), v)
    w = v.copy()
    w[4098] = np.nextafter(w[4098], 1.0)
    assert not vo.exact(w, v)
    assert not vo.exact(np.array([0.0]), np.array([-0.0]))
    s = np.full(4, vo.SENTINEL, dtype=np.uint64).view(np.float64)
    assert vo.is_sentinel(s) and not vo.is_sentinel(np.array([np.nan]))
