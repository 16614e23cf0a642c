"""The full-space operator-times-vector kernels element by element: k_mopr_spin, k_mopr_onebody, k_mopr_terms<0> / <1>
(qbh_mopr.hip) and k_qudit_mopr (qbh_qudit.hip), through their C entry points, against tests/moprref.py (a host reference in
longdouble that scatters forward from every source state and finds targets by searchsorted; pinned by tests/test_moprref.py).

Shapes sit on every seam of the kernels: dimension-1 targets, empty and full sectors, bit 31 and the first 64-bit patterns,
site 63, 32 down spins (the last index of the part-count tables), fermion orbitals 30 and 61, every level width of the d-level
words up to bit 63, charges where the counting table is read clamped, 4096 factors in one call, and target sectors of more
than 2048 * 256 rows, where the grid-stride loop of every kernel takes a second trip.

Source vectors are random complex and not normalised.  The output buffer holds dim_new + 64 elements pre-filled with a sentinel.
Every case asserts, over every row:

  bound       |got_i - want_i| <= 4 (k_i + 4) 2^-53 scale_i,   scale_i = sum |coef_t| |amplitude_t| |x_j|,  k_i = number of terms
              that reach row i.  At most k_i terms are accumulated; each is at most two nested complex products (sqrt(5) u each,
              at most 4 roundings: coefficient x local element x source element, the amplitudes +-1, +-1/2^m being exact); every
              kernel accumulates in the order of a plain sum, whose error is at most (k_i - 1) u sum |term| to first order.  (S^z_q
              sums its k_i = n_sites coefficients first and multiplies once, which the same count covers.)  The + 4 leaves room
              for the second-order terms and for k_i = 1.
  zeros       rows with k_i = 0 are exactly 0.0 in both parts (the bound is 0 there),
  tail        the 64 elements after dim_new still hold the sentinel bit for bit,
  source      the source tensor is unchanged bit for bit,
  dimension   where the entry point returns the dimension it equals the reference's.

Each case prints the worst ratio |got - want| / bound."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import moprref
from quantum_basis_amd import _lib
from test_moprref import local_matrix

pytestmark = pytest.mark.gpu
SENTINEL = moprref.SENTINEL
TAIL = 64
ONE_TRIP = 2048 * 256                                    # rows the capped grid covers in one trip of the grid-stride loop


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=n) + 1j * rng.normal(size=n)) * 1.3).astype(np.complex128)        # not normalised


def _zs(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def _ptr(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _run(launch, x, dim_new, fill=SENTINEL):
    """launch(source address, target address) on a fresh source tensor and a target of dim_new + TAIL elements filled with
    `fill`; returns the whole target buffer, after asserting that the source came back bit for bit"""
    tx = torch.from_numpy(np.array(x)).cuda()                              # a copy: the cached host vector stays read-only
    ty = torch.full((dim_new + TAIL,), complex(fill, fill), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    launch(C.c_void_p(tx.data_ptr()), C.c_void_p(ty.data_ptr()))
    torch.cuda.synchronize()
    out = ty.cpu().numpy()
    assert tx.cpu().numpy().tobytes() == x.tobytes(), "the source vector was written"
    return out


def _check(label, launch, x, ref):
    want, scale, k = ref
    dim_new = len(want)
    out = _run(launch, x, dim_new)
    got = out[:dim_new]
    v = moprref.compare(got, want, scale, k)
    print("%-58s dim %7d  k %d..%d  worst |got - want| / bound %.3g" % (label, dim_new, k.min() if dim_new else 0, k.max() if dim_new else 0, v.worst))
    assert out[dim_new:].tobytes() == np.full(TAIL, complex(SENTINEL, SENTINEL)).tobytes(), (label, "written beyond the target sector")
    assert v.ok and v.worst <= 1.0, (label, v.worst, v.bad[:8], got[v.bad[:8]], want[v.bad[:8]])
    zero = k == 0
    assert np.all(got.real[zero] == 0.0) and np.all(got.imag[zero] == 0.0), (label, "a row that must vanish exactly does not")
    return v.worst


def _twice(label, launch, x, ref):
    """the same call into a buffer of sentinels and into a buffer of NaN: the target sectors byte-identical, no NaN"""
    dim_new = len(ref[0])
    a = _run(launch, x, dim_new, SENTINEL)[:dim_new]
    b = _run(launch, x, dim_new, float("nan"))[:dim_new]
    assert not np.isnan(b.real).any() and not np.isnan(b.imag).any(), label
    assert a.tobytes() == b.tobytes(), label
    assert moprref.compare(b, *ref).ok, label


# ================================================================================================ k_mopr_spin ==
SPIN_SHAPES = [(1, 0), (2, 1), (6, 0), (6, 6),             # dimension-1 targets, empty / full sector, a single valid kind
               (13, 6),                                    # generic
               (32, 2), (33, 2), (40, 2),                  # bit 31, then the first 64-bit patterns
               (64, 1), (64, 2),                           # site 63; S^- target C(64, 2) = 2016
               (34, 31), (34, 32)]                         # 32 down spins as target and as source (dims 5984, 561)
SPIN_LARGE = [(22, 11, 0), (22, 10, -1), (22, 12, +1),     # target C(22, 11) = 705 432: the second trip at mid filling
              (40, 5, 0), (40, 4, -1)]                     # target C(40, 5) = 658 008: the second trip on 64-bit patterns


def _spin_coef(n):
    return _zs(n, 1000 + n)


@functools.lru_cache(maxsize=None)
def _spin_case(n, n_dn, kind):
    x = _rand(math.comb(n, n_dn), 7 + 100 * n + n_dn)
    x.setflags(write=False)
    return x, moprref.spin(n, n_dn, kind, _spin_coef(n), x)


def _spin_launch(n, n_dn, kind):
    coef = _spin_coef(n)

    def launch(src, dst):
        _lib.check(_lib.lib().qbh_mopr_spin_dev(n, n_dn, kind, _ptr(coef), src, dst, None), "qbh_mopr_spin_dev")
    return launch


@pytest.mark.parametrize("shape", SPIN_SHAPES, ids=lambda s: "N%d_dn%d" % s)
def test_spin_every_valid_kind(shape):
    n, n_dn = shape
    ran = 0
    for kind in (0, -1, +1):
        n_new = n_dn - kind
        if not (0 <= n_new <= min(n, 32)):                                 # no such sector, or 33 down spins: test_mopr_cpu.py pins the refusal
            continue
        x, ref = _spin_case(n, n_dn, kind)
        assert len(ref[0]) == math.comb(n, n_new)
        _check("spin (%d, %d) kind %+d" % (n, n_dn, kind), _spin_launch(n, n_dn, kind), x, ref)
        ran += 1
    assert ran >= 1


@pytest.mark.parametrize("case", SPIN_LARGE, ids=lambda c: "N%d_dn%d_kind%d" % c)
def test_spin_second_trip_of_the_grid_stride_loop(case):
    n, n_dn, kind = case
    x, ref = _spin_case(n, n_dn, kind)
    assert len(ref[0]) > ONE_TRIP
    _check("spin (%d, %d) kind %+d" % case, _spin_launch(n, n_dn, kind), x, ref)


# ============================================================================================= k_mopr_onebody ==
def _all_pairs(n, seed):
    """all ordered pairs (a, b) x both spins, densities included, random complex weights, and one term listed twice"""
    rng = np.random.default_rng(seed)
    t = [(a, b, sp, complex(rng.normal(), rng.normal())) for a in range(n) for b in range(n) for sp in (0, 1)]
    t.append(t[len(t) // 3])
    return tuple(t)


def _six_terms(n):
    """a < b and a > b, adjacent sites, (0, n - 1) and (n - 1, 0), on both species, and one density"""
    return ((2, 9, 0, 0.7 - 0.3j), (9, 2, 1, -0.2 + 1.1j), (5, 6, 1, 0.9j), (0, n - 1, 0, 0.4 + 0.4j), (n - 1, 0, 1, 1.0 - 0.5j), (4, 4, 0, -0.8 + 0.1j))


ONEBODY_CASES = [(2, 1, 1, "pairs"), (8, 3, 4, "pairs"), (8, 0, 3, "pairs"), (8, 8, 1, "pairs"), (31, 1, 1, "pairs"), (31, 2, 1, "pairs"),
                 (12, 5, 6, "six")]


def _onebody_terms(n, which):
    return _all_pairs(n, 50 + n) if which == "pairs" else _six_terms(n)


@functools.lru_cache(maxsize=None)
def _onebody_case(n, nu, nd, which):
    x = _rand(math.comb(n, nu) * math.comb(n, nd), 11 + 1000 * n + 10 * nu + nd)
    x.setflags(write=False)
    return x, moprref.onebody(n, nu, nd, _onebody_terms(n, which), x)


def _onebody_launch(n, nu, nd, terms):
    a, b, sp = _i32([t[0] for t in terms]), _i32([t[1] for t in terms]), _i32([t[2] for t in terms])
    w = np.array([t[3] for t in terms], dtype=np.complex128)

    def launch(src, dst):
        _lib.check(_lib.lib().qbh_mopr_onebody_dev(n, nu, nd, len(terms), _ptr(a), _ptr(b), _ptr(sp), _ptr(w), src, dst, None),
                   "qbh_mopr_onebody_dev")
    return launch


@pytest.mark.parametrize("case", ONEBODY_CASES, ids=lambda c: "N%d_up%d_dn%d_%s" % c)
def test_onebody(case):
    n, nu, nd, which = case
    x, ref = _onebody_case(*case)
    assert len(ref[0]) == math.comb(n, nu) * math.comb(n, nd)
    if which == "six":
        assert len(ref[0]) == 731808 > ONE_TRIP
    _check("onebody (%d, %d, %d) %s" % case, _onebody_launch(n, nu, nd, _onebody_terms(n, which)), x, ref)


# =============================================================================================== k_mopr_terms ==
SZ, SP, SM = 0, 1, 2                                       # family 0: S^z, S^+ (down -> up), S^- (up -> down)
NN, CD, CA = 0, 1, 2                                       # family 1: n, c^dag, c
UP, DN = 0, 1


def _terms_launch(family, n, n_a, n_b, terms, dim_box):
    ptr = _i32(np.cumsum([0] + [len(fs) for _, fs in terms]))
    flat = [f for _, fs in terms for f in fs]
    kind, site, sp = _i32([f[0] for f in flat]), _i32([f[1] for f in flat]), _i32([f[2] for f in flat])
    coef = np.array([c for c, _ in terms], dtype=np.complex128)

    def launch(src, dst):
        dim = C.c_int64(-1)
        _lib.check(_lib.lib().qbh_mopr_terms_dev(family, n, n_a, n_b, len(terms), _ptr(ptr), _ptr(kind), _ptr(site), _ptr(sp) if family else None,
                                                 _ptr(coef), src, dst, C.byref(dim), None), "qbh_mopr_terms_dev")
        dim_box.append(dim.value)
    return launch


def _spin_terms(name):
    """name -> (n_sites, n_dn_old, terms)"""
    if name.startswith("mixed"):                           # the five mixed products of test_gpu_mopr.py on (9, 4)
        delta = {"mixed0": 0, "mixed+1": 1, "mixed-1": -1}[name]
        tail = {0: [], 1: [(SM, 6, 0)], -1: [(SP, 2, 0)]}[delta]
        return 9, 4, [(0.7 + 0.2j, [(SP, 2, 0), (SM, 5, 0), (SZ, 1, 0)] + tail), (-1.3j, [(SM, 0, 0), (SP, 7, 0)] + tail),
                      (0.4, [(SZ, 3, 0), (SZ, 3, 0)] + tail), (1.1, tail + [(SZ, 8, 0)]),
                      (0.25 - 0.5j, [(SP, 4, 0), (SM, 4, 0), (SM, 1, 0), (SP, 0, 0)] + tail)]
    if name == "identity":                                 # a term with no factor beside others
        return 9, 4, [(0.7 + 0.2j, [(SP, 2, 0), (SM, 5, 0), (SZ, 1, 0)]), (-0.9 + 0.3j, []), (-1.3j, [(SM, 0, 0), (SP, 7, 0)]), (0.5j, [])]
    if name == "vanishing":                                # S^+_3 S^+_3 ... vanishes on every state: rows only it could reach are exact zeros
        return 9, 4, [(2.5 - 1j, [(SP, 3, 0), (SP, 3, 0), (SM, 3, 0), (SM, 0, 0)]), (0.8 + 0.1j, [(SP, 2, 0), (SM, 5, 0)])]
    if name == "only_vanishing":
        return 9, 4, [(2.5 - 1j, [(SP, 3, 0), (SP, 3, 0), (SM, 3, 0), (SM, 0, 0)]), (1.0, [(SM, 7, 0), (SM, 7, 0), (SP, 7, 0), (SP, 1, 0)])]
    if name.startswith("wide"):                            # factors on sites 0, 31, 32 and n - 1
        n, delta = {"wide33": 33, "wide40": 40, "wide64": 64}[name[:6]], {"": 0, "+1": 1, "-1": -1}[name[6:]]
        tail = {0: [], 1: [(SM, n - 1, 0)], -1: [(SP, 32, 0)]}[delta]
        tail2 = {0: [], 1: [(SM, 0, 0)], -1: [(SP, 31, 0)]}[delta]
        return n, 2, [(0.6 - 0.2j, [(SZ, 0, 0)] + tail), (1.2j, [(SZ, 31, 0), (SZ, 32, 0)] + tail2), (-0.7, [(SP, 0, 0), (SM, n - 1, 0)] + tail2),
                      (0.3 + 0.9j, [(SM, 31, 0), (SP, 32, 0)] + tail2), (1.5, tail + [(SP, n - 1, 0), (SM, 32, 0)]), (-0.4j, tail + [(SZ, n - 1, 0)]),
                      (0.2, tail2 + [(SM, 32, 0), (SP, 31, 0), (SZ, 0, 0)])]
    if name == "to_empty":                                 # a target of dimension 1: (6, 1) -> n_dn = 0 by S^+
        return 6, 1, [(0.5 + 0.1j * s, [(SP, s, 0)]) for s in range(6)]
    if name == "to_full":                                  # (6, 5) -> 6 by S^-
        return 6, 5, [(0.5 - 0.1j * s, [(SM, s, 0)]) for s in range(6)]
    if name == "4096":                                     # exactly 4096 factors: 1024 four-factor terms with random sites on (8, 4)
        rng = np.random.default_rng(4096)
        shapes = [[SP, SM, SZ, SZ], [SM, SZ, SP, SZ], [SZ, SZ, SM, SP], [SP, SM, SP, SM], [SM, SP, SM, SP], [SZ, SZ, SZ, SZ], [SM, SP, SZ, SZ]]
        out = []
        for _ in range(1024):
            kinds = shapes[rng.integers(len(shapes))]
            out.append((complex(rng.normal(), rng.normal()), [(kd, int(rng.integers(8)), 0) for kd in kinds]))
        return 8, 4, out
    if name == "second_trip":                              # (22, 11) with four terms
        return 22, 11, [(0.7 + 0.2j, [(SP, 2, 0), (SM, 21, 0), (SZ, 1, 0)]), (-1.3j, [(SM, 0, 0), (SP, 17, 0)]), (0.4, [(SZ, 3, 0), (SZ, 20, 0)]),
                        (0.25 - 0.5j, [(SP, 4, 0), (SM, 4, 0), (SM, 11, 0), (SP, 10, 0)])]
    raise KeyError(name)


def _fermion_terms(name):
    """name -> (n_sites, n_up_old, n_dn_old, terms)"""
    n = 5
    if name == "number_conserving":
        return 5, 2, 3, [(0.8, [(CD, 1, UP), (CA, 3, UP)]), (-0.6j, [(CD, 4, DN), (CA, 0, DN)]), (1.5, [(NN, 2, UP), (NN, 2, DN)]),
                         (0.3 + 0.1j, [(CD, 0, UP), (CD, 1, DN), (CA, 3, DN), (CA, 2, UP)]), (2.0, [(CA, 1, UP), (CD, 1, UP)])]
    if name == "spin_flip":
        return 5, 2, 3, [(1.0 + 0.2j * s, [(CD, s, UP), (CA, s, DN)]) for s in range(n)] + [(0.5j, [(CD, 0, UP), (CA, 4, DN), (NN, 2, DN)])]
    if name == "remove_up":
        return 5, 2, 3, [(np.exp(2j * np.pi * s / n), [(CA, s, UP)]) for s in range(n)]
    if name == "add_pair":
        return 5, 2, 3, [(1.0 + 0.5 * s - 0.3j, [(CD, s, UP), (CD, s, DN)]) for s in range(n)]
    if name == "forbidden":                                # c^dag_a c^dag_a ...: the intermediate state does not exist, exact zeros
        return 5, 2, 3, [(1.7 - 0.4j, [(CD, 1, UP), (CD, 1, UP), (CA, 1, UP), (CA, 0, UP)]), (0.9 + 0.2j, [(CD, 1, UP), (CA, 3, UP)]),
                         (-0.5, [(CA, 2, DN), (CA, 2, DN), (CD, 2, DN), (CD, 4, DN)])]
    if name in ("site30_11", "site30_22"):                 # orbitals 30 and 61, signs counted across the species boundary
        nu = nd = 1 if name == "site30_11" else 2
        return 31, nu, nd, [(0.8 - 0.1j, [(CD, 30, UP), (CA, 0, UP)]), (-0.6j, [(CD, 0, DN), (CA, 30, DN)]), (1.5, [(NN, 30, UP), (NN, 30, DN)]),
                            (0.3 + 0.1j, [(CD, 30, UP), (CD, 0, DN), (CA, 30, DN), (CA, 0, UP)]), (2.0, [(CA, 30, DN), (CD, 30, DN)]),
                            (0.7j, [(CD, 29, DN), (CA, 30, DN)]), (-1.1, [(CD, 30, UP), (CA, 29, UP), (NN, 30, DN)])]
    if name in ("flip30_11", "flip30_22"):                 # c^dag_{30,up} c_{30,down} and its neighbours
        nu = nd = 1 if name == "flip30_11" else 2
        return 31, nu, nd, [(1.0 + 0.3j, [(CD, 30, UP), (CA, 30, DN)]), (0.4 - 0.2j, [(CD, 0, UP), (CA, 0, DN)]), (-0.9j, [(CD, 15, UP), (CA, 15, DN)]),
                            (0.6, [(CD, 30, UP), (CA, 0, DN)]), (1.3j, [(CD, 0, UP), (CA, 30, DN), (NN, 30, UP)])]
    if name == "add_up_to_none":                           # (8, 0, 3): a species with no particle gains one
        return 8, 0, 3, [(np.exp(2j * np.pi * s / 8) * (1 + 0.1 * s), [(CD, s, UP)]) for s in range(8)]
    if name == "remove_from_full":                         # (8, 8, 1): the full species loses one
        return 8, 8, 1, [(np.exp(-2j * np.pi * s / 8) * (1 + 0.1 * s), [(CA, s, UP)]) for s in range(8)]
    if name == "remove_the_last":                          # (8, 8, 1): the single down electron goes, the target has an empty species
        return 8, 8, 1, [(0.3 + 0.2j * s, [(CA, s, DN)]) for s in range(8)]
    if name == "second_trip":                              # (12, 5, 6) -> (12, 6, 5) by S^+_q: dim 731 808, nd_old != nd_new
        return 12, 5, 6, [(np.exp(2j * np.pi * 5 * s / 12) / np.sqrt(12.0), [(CD, s, UP), (CA, s, DN)]) for s in range(12)]
    raise KeyError(name)


SPIN_TERM_CASES = ["mixed0", "mixed+1", "mixed-1", "identity", "vanishing", "only_vanishing", "wide33", "wide33+1", "wide33-1", "wide40", "wide40+1",
                   "wide40-1", "wide64", "wide64+1", "wide64-1", "to_empty", "to_full", "4096", "second_trip"]
FERMION_TERM_CASES = ["number_conserving", "spin_flip", "remove_up", "add_pair", "forbidden", "site30_11", "site30_22", "flip30_11", "flip30_22",
                      "add_up_to_none", "remove_from_full", "remove_the_last", "second_trip"]


@functools.lru_cache(maxsize=None)
def _terms_case(family, name):
    if family == 0:
        n, n_a, tm = _spin_terms(name)
        n_b, dim_old = 0, math.comb(n, n_a)
    else:
        n, n_a, n_b, tm = _fermion_terms(name)
        dim_old = math.comb(n, n_a) * math.comb(n, n_b)
    x = _rand(dim_old, 13 + sum(map(ord, name)) + family)
    x.setflags(write=False)
    return n, n_a, n_b, tm, x, moprref.terms(family, n, n_a, n_b, tm, x)


def _check_terms(family, name):
    n, n_a, n_b, tm, x, ref = _terms_case(family, name)
    box = []
    worst = _check("terms<%d> %s (%d, %d, %d)" % (family, name, n, n_a, n_b), _terms_launch(family, n, n_a, n_b, tm, box), x, ref)
    assert box == [len(ref[0])], (box, len(ref[0]))
    return ref, worst


@pytest.mark.parametrize("name", SPIN_TERM_CASES)
def test_terms_on_spin_sectors(name):
    (want, scale, k), _ = _check_terms(0, name)
    n, n_a, _, tm, _, _ = _terms_case(0, name)
    if name == "identity":
        assert k.min() >= 2                                                # both empty products reach every row
    if name in ("vanishing", "only_vanishing"):
        assert (k == 0).sum() >= len(k) // 2 and ((k == 0).all() == (name == "only_vanishing"))
    if name in ("to_empty", "to_full"):
        assert len(want) == 1 and k[0] == 6                              # the one row gathers from all six sites
    if name == "4096":
        assert sum(len(fs) for _, fs in tm) == 4096 and len(tm) == 1024
    if name == "second_trip":
        assert len(want) > ONE_TRIP
    if name.startswith("wide"):
        assert {0, 31, 32, n - 1} <= {s for _, fs in tm for _, s, _ in fs}


@pytest.mark.parametrize("name", FERMION_TERM_CASES)
def test_terms_on_two_species_fermions(name):
    (want, scale, k), _ = _check_terms(1, name)
    n, nu, nd, tm, _, _ = _terms_case(1, name)
    if name == "forbidden":
        assert (k == 0).any() and k.max() == 1
    if name == "second_trip":
        assert len(want) == 731808 > ONE_TRIP and math.comb(12, 6) != math.comb(12, 5)
    if name.startswith(("site30", "flip30")):
        assert {30 + 31 * sp for _, fs in tm for _, s, sp in fs if s == 30} == {30, 61}
    if name == "remove_the_last":
        assert len(want) == 1


# =============================================================================================== k_qudit_mopr ==
QUDIT_SMALL = [(2, 6), (3, 8), (4, 6), (5, 5), (8, 4)]     # every charge, every dq of {0, +-1, +-2, +-(d - 1)} that keeps the target a sector
QUDIT_WIDE = [(2, 33), (2, 64), (3, 32), (4, 32), (8, 21)]  # words up to bit 63: the charges next to both ends
QUDIT_LARGE = [(3, 14, 14, 0), (3, 14, 13, +1), (3, 14, 15, -1)]      # target dim 616 227: the second trip


def _dqs(d):
    return sorted(q for q in {0, 1, -1, 2, -2, d - 1, 1 - d} if abs(q) < d)


# level changes by +-(d - 1) out of the charges next to the ends reach into sectors of 2 10^6 to 3 10^7 rows (long second trips
# on words that use bits 60 - 62): required like every other pair of these shapes, run one by one and not cached
QUDIT_LONG = [(4, 32, 3, +3), (4, 32, 93, -3), (8, 21, 1, +7), (8, 21, 2, +7), (8, 21, 3, +7), (8, 21, 146, -7), (8, 21, 145, -7), (8, 21, 144, -7)]
LONG_ROWS = 10 ** 6


def _qudit_required(d, n, wide):
    """(total_old, dq) a shape has to run: every dq of {0, +-1, +-2, +-(d - 1)} that keeps the target a sector, out of every
    charge (small shapes) or out of the charges within 3 (2 for d = 2) of charge 0 and of the maximal charge (wide shapes)"""
    top = n * (d - 1)
    near = 2 if d == 2 else 3
    return [(total, dq) for total in range(top + 1) for dq in _dqs(d)
            if 0 <= total + dq <= top and (not wide or total <= near or total >= top - near)]


def _qudit_extra(d, n):
    """wide shapes, beyond what is required: level changes INTO the charges next to the ends from farther inside, where both
    sectors are small (the target below 10^6 rows, the source below 8 10^6 / n_sites)"""
    top = n * (d - 1)
    near = 2 if d == 2 else 3
    return [(total, dq) for total in range(near + 1, top - near) for dq in _dqs(d)
            if (total + dq <= near or total + dq >= top - near) and 0 <= total + dq <= top
            and moprref.count(n, d, total + dq) < LONG_ROWS and moprref.count(n, d, total) * n <= 8 * 10 ** 6]


def _qudit_coef(n):
    return _zs(n, 2000 + n)


@functools.lru_cache(maxsize=None)
def _qudit_case(d, n, total, dq):
    x = _rand(moprref.count(n, d, total), 17 + 1000 * d + 10 * n + total)
    x.setflags(write=False)
    loc = local_matrix(d, dq, 300 + 10 * d + dq)
    return x, loc, moprref.qudit(n, d, total, dq, _qudit_coef(n), loc.ravel(), x)


def _qudit_launch(d, n, total, dq, loc, dim_box):
    coef, flat = _qudit_coef(n), np.ascontiguousarray(loc.ravel())

    def launch(src, dst):
        dim = C.c_int64(-1)
        _lib.check(_lib.lib().qbh_mopr_qudit_dev(n, d, total, dq, _ptr(coef), _ptr(flat), src, dst, C.byref(dim), None), "qbh_mopr_qudit_dev")
        dim_box.append(dim.value)
    return launch


def _check_qudit(d, n, total, dq, cached=True):
    x, loc, ref = (_qudit_case if cached else _qudit_case.__wrapped__)(d, n, total, dq)
    box = []
    worst = _check("qudit d %d n %d charge %d dq %+d" % (d, n, total, dq), _qudit_launch(d, n, total, dq, loc, box), x, ref)
    assert box == [len(ref[0])] and len(ref[0]) == moprref.count(n, d, total + dq)
    return worst


@pytest.mark.parametrize("shape", QUDIT_SMALL + QUDIT_WIDE, ids=lambda s: "d%d_n%d" % s)
def test_qudit_charges_and_level_changes(shape):
    d, n = shape
    top = n * (d - 1)
    wide = shape in QUDIT_WIDE
    required = _qudit_required(d, n, wide)
    # charge 0, the maximal charge and every dq occur, and the skip branch (an exact zero on the dq diagonal)
    assert {t for t, _ in required} >= {0, top} and {q for _, q in required} == set(_dqs(d))
    if not wide:
        assert {t for t, _ in required} == set(range(top + 1))
    assert (np.diag(local_matrix(d, 0, 300 + 10 * d)) == 0).sum() == 1
    # nothing required is left out: what does not run here is exactly what test_qudit_long_level_changes runs
    long = [(t, q) for t, q in required if moprref.count(n, d, t + q) >= LONG_ROWS]
    assert sorted(long) == sorted((t, q) for dd, nn, t, q in QUDIT_LONG if (dd, nn) == shape)
    for total, dq in sorted(set(required) - set(long)) + (_qudit_extra(d, n) if wide else []):
        _check_qudit(d, n, total, dq)


@pytest.mark.parametrize("case", QUDIT_LONG, ids=lambda c: "d%d_n%d_q%d_dq%d" % c)
def test_qudit_long_level_changes(case):
    d, n, total, dq = case
    assert abs(dq) == d - 1 and moprref.count(n, d, total + dq) > 4 * ONE_TRIP and (d, n) in QUDIT_WIDE
    _check_qudit(d, n, total, dq, cached=False)
    moprref.words.cache_clear()                                            # the enumerated target: up to 3 10^7 words


@pytest.mark.parametrize("case", QUDIT_LARGE, ids=lambda c: "d%d_n%d_q%d_dq%d" % c)
def test_qudit_second_trip_of_the_grid_stride_loop(case):
    d, n, total, dq = case
    assert moprref.count(n, d, total + dq) == 616227 > ONE_TRIP
    _check_qudit(d, n, total, dq)


# ============================================================================================== repeatability ==
def test_every_kernel_twice_into_sentinels_and_into_nan():
    x, ref = _spin_case(13, 6, -1)
    _twice("spin", _spin_launch(13, 6, -1), x, ref)
    x, ref = _onebody_case(8, 3, 4, "pairs")
    _twice("onebody", _onebody_launch(8, 3, 4, _onebody_terms(8, "pairs")), x, ref)
    for family, name in ((0, "mixed0"), (1, "number_conserving")):
        n, n_a, n_b, tm, x, ref = _terms_case(family, name)
        _twice("terms<%d>" % family, _terms_launch(family, n, n_a, n_b, tm, []), x, ref)
    x, loc, ref = _qudit_case(3, 8, 8, +1)
    _twice("qudit", _qudit_launch(3, 8, 8, +1, loc, []), x, ref)
