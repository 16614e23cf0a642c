"""qbh_mopr_kondo_dev and qbh_mopr_kondo_repr_dev on the device, element by element against tests/kondoops.py (numpy, written
from the operators' definitions and pinned by algebra in tests/test_kondoops.py), evaluated in longdouble.

Bound.  A target row is a sum of n_i products w_k x_k, evaluated in site order.  In any order such a sum is off by at most
n_i u sum_k |w_k| |x_k| with u = 2^-53; the factor 4 and the 4 added to n_i cover the complex products and that each w_k is
itself a product of a coefficient, a character and a square root computed in double:
    |got_i - want_i| <= 4 (n_i + 4) u sum_k |w_k| |x_k|.
n_i and the absolute sum come from the longdouble reference (kondoops.apply_full / kondoops.project).  A row without a
contribution must be exactly 0.  Every figure is printed before it is asserted.

The full-sector operator takes no bonds: an open chain and a ring of L sites are one case for it, so part 1 runs over L and
the sectors alone; the lattices enter with the translations of part 3."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp

import kondoops as ko
import quantum_basis_amd as q
from quantum_basis_amd import kondo, lattices
from oracle import qb_oracle as qo

pytestmark = pytest.mark.gpu

PLAIN = dict(value_dict=0, real_fast_path=0)
LD, CLD = np.longdouble, np.clongdouble
U53 = LD(2.0) ** -53
SENTINEL = complex(7.25e77, -3.5e77)


@lru_cache(maxsize=1)
def handle():
    """any operator handle in the generators' order: device vectors are uploaded and downloaded through one"""
    return q.csr_mat.kondo(2, 2, 0, [(0, 1)], opts=q.make_opts(**PLAIN))


@lru_cache(maxsize=64)
def sector(n, ne, sz):
    return ko.Sector(n, ne, sz)


GROUPS = {"ring": (lambda n, m: ko.chain_group(n, m), lambda n: (n,)), "torus32": (lambda n, mx, my: ko.torus_group(3, 2, mx, my), lambda n: (3, 2))}


@lru_cache(maxsize=64)
def _momentum(n, ne, sz, group, k):
    perms, turns = GROUPS[group][0](n, *k)
    return ko.Momentum(sector(n, ne, sz), perms, turns), perms, turns


def momentum(n, ne, sz, group, *k):
    """(momentum states, perms, turns) of a sector, shared between the cases and never written to"""
    return _momentum(n, ne, sz, group, tuple(a % b for a, b in zip(k, GROUPS[group][1](n))))


def rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def run_twice(call, x, dim_new):
    """the device call on x with the target pre-filled with a sentinel: no sentinel survives and two runs are bit-identical"""
    H = handle()
    vx, vy = q.DeviceVec(H, len(x)), q.DeviceVec(H, dim_new)
    vx.upload(x)
    out = []
    for _ in range(2):
        vy.upload(np.full(dim_new, SENTINEL))
        dims = call(vx.ptr, vy.ptr)
        assert dims == (len(x), dim_new), (dims, len(x), dim_new)
        out.append(vy.download())
    vx.free()
    vy.free()
    assert not np.any(out[0] == SENTINEL)
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64))
    return out[0]


def assert_rows(got, want, n_i, ab, tag):
    bound = 4 * (n_i.astype(LD) + 4) * U53 * ab
    diff = np.abs(got.astype(CLD) - want)
    live = ab > 0
    worst = float(np.max(diff[live] / bound[live])) if live.any() else 0.0
    print("%s: %d rows, %d with contributions, max n_i %d, max |dy| %.3e, worst |dy|/bound %.3f"
          % (tag, len(got), int(live.sum()), int(n_i.max()) if len(n_i) else 0, float(diff.max()) if len(diff) else 0.0, worst))
    assert np.all(diff <= bound)
    assert not got[~live].any()                            # no contribution: exactly 0


def coef_variants(op, ce, cs):
    """c / c^dag: one set; the spin flips: the electrons alone, the local spins alone, both"""
    return [(ce, None)] if op < ko.SPIN_PLUS else [(ce, None), (None, cs), (ce, cs)]


# ---- 1 ----
def check_full(n, ne, sz, seed):
    src = sector(n, ne, sz)
    x = rand(src.N, seed)
    done = 0
    for op in ko.OPS:
        te, ts = ko.target(ne, sz, op)
        if not (0 <= te <= 2 * n) or kondo.sector_dim(n, te, ts) == 0:
            continue
        dst = sector(n, te, ts)
        for ce, cs in coef_variants(op, rand(n, seed + 10 + op), rand(n, seed + 20 + op)):
            got = run_twice(lambda px, py: q.moprXvec_kondo(n, ne, sz, op, ce, cs, px, py), x, dst.N)
            want, n_i, ab = ko.apply_full(src, dst, op, ce, cs, x)
            assert_rows(got, want, n_i, ab, "L=%d (%d,%d) op %d %s%s" % (n, ne, sz, op, "e" if ce is not None else "", "s" if cs is not None else ""))
            done += 1
    return done


@pytest.mark.parametrize("n,sectors", [
    (4, [(4, 0), (3, 1), (5, 3), (2, -4), (0, 0), (8, 0), (4, 8)]),       # (0, 0), (8, 0): one s-block; (4, 8): one word
    (5, [(5, 0), (4, 1), (6, -3), (0, 5), (10, -1), (7, 2)]),             # odd L moves the particle-number blocks
])
def test_full_sector_every_op(n, sectors):
    done = 0
    for k, (ne, sz) in enumerate(sectors):
        assert kondo.sector_dim(n, ne, sz) > 0
        done += check_full(n, ne, sz, 100 * n + k)
    assert done >= 5 * len(sectors)                        # the edges of the table lack some targets
    one_block = [s for s in sectors if len(kondo.sector_blocks(n, *s)) == 1]
    assert one_block


def test_full_sector_L6_half_filling():
    assert kondo.sector_dim(6, 6, 0) == 15184
    assert check_full(6, 6, 0, 600) == 10


# ---- 2 ----
def unit(n, i, v=1.0):
    c = np.zeros(n, dtype=np.complex128)
    c[i] = v
    return c


def apply_chain(n, ne, sz, steps, x):
    """the product of device calls, applied right to left; steps = [(op, coef_elec, coef_spin), ...] left to right"""
    H = handle()
    cur = q.DeviceVec(H, len(x))
    cur.upload(x)
    for op, ce, cs in reversed(steps):
        te, ts = ko.target(ne, sz, op)
        nxt = q.DeviceVec(H, kondo.sector_dim(n, te, ts))
        q.moprXvec_kondo(n, ne, sz, op, ce, cs, cur.ptr, nxt.ptr)
        cur.free()
        cur, ne, sz = nxt, te, ts
    y = cur.download()
    cur.free()
    return y


def assert_against_operator(A, x, got, tag):
    """got against the stored operator A applied to x in longdouble, n_i = 2"""
    ia, ja, val = A.download()
    M = sp.csr_matrix((val, ja, ia), shape=(A.dim, A.dim))
    rows = np.repeat(np.arange(A.dim), np.diff(ia))
    want, ab = np.zeros(A.dim, dtype=CLD), np.zeros(A.dim, dtype=LD)
    np.add.at(want, rows, val.astype(CLD) * x.astype(CLD)[ja])
    np.add.at(ab, rows, np.abs(val).astype(LD) * np.abs(x).astype(LD)[ja])
    assert np.diff(M.indptr).max() <= 2
    assert_rows(got, want, np.full(A.dim, 2), ab, tag)
    assert np.count_nonzero(ab) > A.dim // 8               # not vacuous


@pytest.mark.parametrize("i", [0, 3])
def test_spin_flips_compose_to_the_kondo_flip_of_the_stored_operator(i):
    """S^+_i s^-_i + S^-_i s^+_i: the local spins' flip after the electrons' flip, both ways, is kxy = 2 on site i"""
    n, ne, sz = 5, 5, 0
    x = rand(kondo.sector_dim(n, ne, sz), 200 + i)
    e = unit(n, i)
    got = (apply_chain(n, ne, sz, [(ko.SPIN_PLUS, None, e), (ko.SPIN_MINUS, e, None)], x)
           + apply_chain(n, ne, sz, [(ko.SPIN_MINUS, None, e), (ko.SPIN_PLUS, e, None)], x))     # the two reach disjoint rows
    A = q.csr_mat.kondo(n, ne, sz, None, terms=kondo.Terms([], [0.0] * n, list(2 * e.real), []), opts=q.make_opts(**PLAIN))
    assert_against_operator(A, x, got, "Kondo flip on site %d" % i)


@pytest.mark.parametrize("i,j", [(0, 1), (4, 1), (2, 3)])
def test_c_dagger_c_composes_to_the_hop_of_the_stored_operator(i, j):
    """c^dag_{i,up} c_{j,up} + c^dag_{j,up} c_{i,up} from four calls against the operator with that one hop pair"""
    n, ne, sz = 5, 5, 0
    x = rand(kondo.sector_dim(n, ne, sz), 300 + i)
    ei, ej = unit(n, i), unit(n, j)
    got = (apply_chain(n, ne, sz, [(ko.CDAG_UP, ei, None), (ko.C_UP, ej, None)], x)
           + apply_chain(n, ne, sz, [(ko.CDAG_UP, ej, None), (ko.C_UP, ei, None)], x))           # disjoint rows again
    A = q.csr_mat.kondo(n, ne, sz, None, terms=kondo.Terms([(i, j, 1.0, 0.0), (j, i, 1.0, 0.0)], [0.0] * n, [0.0] * n, []),
                        opts=q.make_opts(**PLAIN))
    assert_against_operator(A, x, got, "up hop %d <-> %d" % (i, j))


# ---- 3 ----
def check_sector(n, ne, sz, group, k, qk, coef, op, seed, variants=None):
    """every coefficient variant of op from momentum k with the coefficients of momentum qk: the target is k - qk"""
    te, ts = ko.target(ne, sz, op)
    mo, perms, turns = momentum(n, ne, sz, group, *k)
    mn, _, _ = momentum(n, te, ts, group, *[a - b for a, b in zip(k, qk)])
    x = rand(mo.dim, seed)
    ce, cs = coef(*qk), coef(*qk, 0.45)
    for a, b in (variants or coef_variants(op, ce, cs)):
        got = run_twice(lambda px, py: q.moprXvec_kondo_repr(n, ne, sz, op, perms, ko.chars_of(turns), a, b, px, py), x, mn.dim)
        want, n_i, ab = ko.project(mo, mn, op, a, b, x)
        assert_rows(got, want, n_i, ab, "%s k=%s q=%s op %d %s%s" % (group, k, qk, op, "e" if a is not None else "", "s" if b is not None else ""))
        assert not got[mn.zero].any()                      # zero-norm targets receive exactly 0
    return mo, mn


@pytest.mark.parametrize("m", range(6))
def test_ring_of_6_every_momentum_every_op(m):
    n, ne, sz = 6, 6, 0
    coef = lambda qm, amp=0.7: ko.chain_coef(n, qm, amp)
    chunks = set()
    for op in ko.OPS:
        for qm in (0, 1 + m % 2, 5 - m % 3):               # three operator momenta, different from sector to sector
            mo, mn = check_sector(n, ne, sz, "ring", (m,), (qm,), coef, op, 1000 + 10 * m + qm)
            chunks.add(((mo.sec.N + 4095) // 4096, (mn.sec.N + 4095) // 4096))
    assert chunks == {(4, 4)}                              # four directory chunks: 15,184 source words, 12,432 in every target


def test_source_and_target_with_different_chunk_counts():
    """From (5, -1), 12,432 words in four chunks of the directory, to 15,184 (four), 6,735 (two) and 12,432 words"""
    n, ne, sz = 6, 5, -1
    coef = lambda qm, amp=0.7: ko.chain_coef(n, qm, amp)
    chunks = set()
    for op in ko.OPS:
        mo, mn = check_sector(n, ne, sz, "ring", (2,), (3,), coef, op, 1500 + op)
        chunks.add(((mo.sec.N + 4095) // 4096, (mn.sec.N + 4095) // 4096))
    assert {(4, 4), (4, 2)} <= chunks


@pytest.mark.parametrize("n", [4, 6])
def test_stabilised_and_zero_norm_representatives(n):
    """Words fixed by a translation, some of which vanish at the momentum, exist where all three fields can repeat: at half
    filling.  Every op out of that sector (zero-norm sources are skipped) and every op into it from the sector that leads
    there (zero-norm targets receive exactly 0: check_sector asserts it)."""
    coef = lambda qm, amp=0.7: ko.chain_coef(n, qm, amp)
    into_half = [((n + 1, 1), ko.C_UP), ((n + 1, -1), ko.C_DN), ((n - 1, -1), ko.CDAG_UP), ((n - 1, 1), ko.CDAG_DN),
                 ((n, -2), ko.SPIN_PLUS), ((n, 2), ko.SPIN_MINUS)]
    zero_src = zero_dst = stab_src = stab_dst = 0
    for m, qm in ((0, 0), (0, n // 2), (n // 2, 1), (1, n // 2 + 1), (2, 2)):
        for op in ko.OPS:
            mo, mn = check_sector(n, n, 0, "ring", (m,), (qm,), coef, op, 2000 + 10 * m + qm)
            zero_src += int(mo.zero.sum())
            stab_src += int(((mo.stab > 1) & ~mo.zero).sum())
        for (ne, sz), op in into_half:
            assert ko.target(ne, sz, op) == (n, 0)
            mo, mn = check_sector(n, ne, sz, "ring", (m,), (qm,), coef, op, 2500 + 10 * m + qm)
            zero_dst += int(mn.zero.sum())
            stab_dst += int(((mn.stab > 1) & ~mn.zero).sum())
    print("zero-norm: source %d target %d; live stabilised: source %d target %d" % (zero_src, zero_dst, stab_src, stab_dst))
    assert zero_src > 0 and zero_dst > 0 and stab_src > 0 and stab_dst > 0


@pytest.mark.parametrize("k", [(1, 1), (2, 0), (0, 0)])
def test_torus_3x2_with_two_generators(k):
    """translations that are not cyclic shifts of the site index: the fermion sign of g* != 0"""
    coef = lambda qx, qy, amp=0.7: ko.torus_coef(3, 2, qx, qy, amp)
    for op in ko.OPS:
        for qk in ((1, 1), (0, 1), (2, 0)):
            check_sector(6, 6, 0, "torus32", k, qk, coef, op, 3000 + 7 * k[0] + k[1])


# ---- 4 ----
def table_bytes(n, n_trans):
    """what the kernel stages in LDS: one 64-entry table per translation and six-bit chunk of a field, and two counting tables"""
    return (n_trans * ((n + 5) // 6) * 64 + 2 * 22 * 22) * 8


def test_wide_words_on_the_large_table_path():
    """The ring of 21 sites from (2, -19): the s field sits in bits 42 .. 62, and 21 translations of 4 chunks make 50,752 B of
    tables, so the kernel runs in its shape of 1024 lanes.  The ops whose target stays below 1e5 words."""
    n, ne, sz = 21, 2, -19
    assert kondo.sector_dim(n, ne, sz) == 53571
    assert 4 * (table_bytes(n, n) + 1024) > 160 * 1024 >= 4 * (table_bytes(13, 13) + 1024)
    coef = lambda qm, amp=0.7: ko.chain_coef(n, qm, amp)
    mo, mn = check_sector(n, ne, sz, "ring", (5,), (3,), coef, ko.C_UP, 4000)
    assert mn.sec.N == 462 and int(mo.sec.w.max()) >> 42 > 0
    mo, mn = check_sector(n, ne, sz, "ring", (5,), (3,), coef, ko.SPIN_MINUS, 4001)
    assert mn.sec.N == 4851


# ---- 5 ----
def test_more_target_rows_than_one_pass_of_the_resident_grid():
    """Ring of 9, (9, 9, 0) -> c_{q,up} -> (8, -1), k = 0 to q = 2 pi / 9: 511,174 target representatives against at most
    min(CUs x 7, 2048) workgroups of 256 lanes."""
    import torch
    n, ne, sz = 9, 9, 0
    coef = lambda qm, amp=0.7: ko.chain_coef(n, qm, amp)
    ce = coef(1)
    mo, mn = check_sector(n, ne, sz, "ring", (0,), (1,), coef, ko.C_UP, 5000, variants=[(ce, None)])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_cu = min(7, (160 * 1024) // (table_bytes(n, n) + 1024))
    lanes = min(cus * per_cu, 2048) * 256
    print("dim_old %d dim_new %d resident lanes %d" % (mo.dim, mn.dim, lanes))
    assert mn.dim == 511174 and per_cu == 7 and mn.dim > lanes
    _momentum.cache_clear()
    sector.cache_clear()


# ---- 6 ----
DEPTH = 60


def green(h, maxit, mm, z):
    g = 0.0
    for j in range(mm - 1, -1, -1):
        g = 1.0 / (z - h[maxit + j] - (h[j + 1] ** 2) * g)
    return g


def test_spectral_function_end_to_end_against_the_oracle():
    """c_{q,up} |phi0> of the Kondo chain L = 6 at half filling: ground state on the device, the operator on the device, the
    "dnmcs" Lanczos on the device; norm, the first 12 continued-fraction coefficients and the Green's function against the
    oracle's Lanczos on the downloaded target operator, started from the numpy operator-apply of the same ground state, with
    the tolerances of test_measure_full_dynamic_end_to_end_against_the_oracle.

    Which chain.  Twelve coefficients to 1e-9 ask for a well-conditioned recurrence, and on six sites it is not always one.
    Measured with the oracle alone (no device): a relative perturbation of 2e-16 of the start vector moves the first 12
    coefficients of the ring with t = 1, J_K = 1.1, U = 0 by 0.7 to 17 times that tolerance, depending on q (the state lies in
    one momentum and spin sector, a few hundred states, and the lowest Ritz value converges within the 12 steps); J_K = 3
    gives 0.3 to 0.8, the open chain at U = 0 0.09 to 0.5, the open chain with U = 2 at q = 2 pi / 6 0.012.  That last one is
    the case here.
    Depth of the Green's function.  The continued fraction is compared over its first DEPTH = 60 levels.  Past that the
    recurrence no longer remembers its start vector: under the same 2e-16 perturbation the oracle's own G(w + 0.1 i) moves by
    1e-4 of the tolerance at 60 levels, by 1e3 times the tolerance at 100 and by 1e4 times with all 198, so over all levels
    two correct runs agree only as far as their roundings happen to coincide (measured here, this kernel against the oracle
    over all 198 levels: worst ratio 1.6 in one run, 4.8e3 in the next on another machine; printed below, not asserted).
    The sum rules need no such care: sum_q |c_{q,up} phi0|^2 = <N_up> on this state through the full
    sectors, and on the ground state of the ring through its momentum sectors."""
    L, ne, sz, maxit, U = 6, 6, 0, 200, 2.0
    bonds = lattices.chain(L, pbc=False)
    A = q.csr_mat.kondo(L, ne, sz, bonds, U=U)
    assert A.info().basis_internal == 0                    # device vectors of A are in the generators' order
    res = q.locate_E0_lanczos(A, nev=1, ncv=1)
    phi = res.eigenvecs
    vphi = q.DeviceVec(A, A.dim)
    vphi.upload(phi)
    src, dst = sector(L, ne, sz), sector(L, 5, -1)
    wave = lambda qm: np.exp(2j * np.pi * qm * np.arange(L) / L) / np.sqrt(L)
    coef = wave(1)
    B = q.csr_mat.kondo(L, 5, -1, bonds, U=U)
    m, norm, hess = q.measure_full_dynamic_dev(B, lambda d: q.moprXvec_kondo(L, ne, sz, ko.C_UP, coef, None, vphi.ptr, d), maxit)
    ia, ja, val = B.download()
    O = qo.Csr(B.dim, ia, ja.astype(np.int64), val, False)
    y = ko.apply_full(src, dst, ko.C_UP, coef, None, phi)[0].astype(np.complex128)
    nrm = np.linalg.norm(y)
    print("|c_q phi0| device %.15f numpy %.15f, steps %d" % (norm, nrm, m))
    assert nrm > 0.1 and abs(norm - nrm) <= 1e-12 * nrm
    v = np.zeros(2 * B.dim, dtype=np.complex128)
    v[:B.dim] = y / nrm
    ho = np.zeros(2 * maxit)
    mo_ = qo.lanczos(0, maxit - 1, maxit, O, v, ho, "dnmcs")[0]
    assert abs(m - mo_) <= 2 and min(m, mo_) >= 100
    k = 12
    da, db = np.abs(hess[maxit:maxit + k] - ho[maxit:maxit + k]), np.abs(hess[1:k + 1] - ho[1:k + 1])
    print("a: max |delta| / (1e-11 + 1e-9 |a|) = %.3e; b: %.3e" % (np.max(da / (1e-11 + 1e-9 * np.abs(ho[maxit:maxit + k]))),
                                                                    np.max(db / (1e-11 + 1e-9 * np.abs(ho[1:k + 1])))))
    assert np.allclose(hess[maxit:maxit + k], ho[maxit:maxit + k], rtol=1e-9, atol=1e-11)
    assert np.allclose(hess[1:k + 1], ho[1:k + 1], rtol=1e-9, atol=1e-11)
    full = 0.0
    for w in np.linspace(0.0, 4.0, 9):
        z = res.E0 + w + 0.1j
        g1, g2 = norm ** 2 * green(hess, maxit, DEPTH, z), nrm ** 2 * green(ho, maxit, DEPTH, z)
        f1, f2 = norm ** 2 * green(hess, maxit, min(m, mo_) - 1, z), nrm ** 2 * green(ho, maxit, min(m, mo_) - 1, z)
        full = max(full, abs(f1 - f2) / (1e-8 * max(abs(f2), 1e-3)))
        print("w = %.1f: depth %d |dG| / tolerance %.3e; all %d levels %.3e"
              % (w, DEPTH, abs(g1 - g2) / (1e-8 * max(abs(g2), 1e-3)), min(m, mo_) - 1, abs(f1 - f2) / (1e-8 * max(abs(f2), 1e-3))))
        assert abs(g1 - g2) <= 1e-8 * max(abs(g2), 1e-3), w
    print("all levels: worst |dG| / tolerance %.3f (not asserted, see the docstring)" % full)
    B.destroy()
    # the sum rule through the full sectors
    n_up = float(np.sum(np.abs(phi) ** 2 * ko.popcount(src.u)))
    total = 0.0
    vy = q.DeviceVec(A, dst.N)
    for qm in range(L):
        assert q.moprXvec_kondo(L, ne, sz, ko.C_UP, wave(qm), None, vphi.ptr, vy.ptr) == (src.N, dst.N)
        total += A.nrm2(vy.ptr) ** 2
    print("open chain: sum_q |c_q phi0|^2 = %.12f, <N_up> = %.12f" % (total, n_up))
    assert abs(total - n_up) < 1e-10
    vy.free()
    vphi.free()
    A.destroy()


def test_sum_rule_through_the_momentum_sectors():
    """The ground state of the ring L = 6 at half filling has one momentum; in its sector, sum over q of |c_{q,up} phi0|^2
    through qbh_mopr_kondo_repr_dev equals <N_up> to 1e-10."""
    L, ne, sz = 6, 6, 0
    A = q.csr_mat.kondo(L, ne, sz, lattices.chain(L))
    phi = q.locate_E0_lanczos(A, nev=1, ncv=1).eigenvecs
    A.destroy()
    src = sector(L, ne, sz)
    weights = [float(np.linalg.norm(momentum(L, ne, sz, "ring", k0)[0].contract(phi.astype(CLD)).astype(np.complex128)) ** 2) for k0 in range(L)]
    k0 = int(np.argmax(weights))
    print("weight of phi0 by momentum:", ["%.3e" % w for w in weights])
    assert weights[k0] > 1 - 1e-10
    mk, perms, turns = momentum(L, ne, sz, "ring", k0)
    xk = mk.contract(phi.astype(CLD)).astype(np.complex128)
    H = handle()
    vx = q.DeviceVec(H, mk.dim)
    vx.upload(xk)
    total = 0.0
    for qm in range(L):
        c = ko.chain_coef(L, qm, 1.0) / np.sqrt(L)
        mn = momentum(L, 5, -1, "ring", k0 - qm)[0]
        vy = q.DeviceVec(H, mn.dim)
        assert q.moprXvec_kondo_repr(L, ne, sz, ko.C_UP, perms, ko.chars_of(turns), c, None, vx.ptr, vy.ptr) == (mk.dim, mn.dim)
        total += float(np.linalg.norm(vy.download()) ** 2)
        vy.free()
    vx.free()
    n_up = float(np.sum(np.abs(phi) ** 2 * ko.popcount(src.u)))
    print("ring: sum_q |c_q phi0|^2 = %.12f, <N_up> = %.12f" % (total, n_up))
    assert abs(total - n_up) < 1e-10
