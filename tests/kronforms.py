"""Host-only helpers for the element-wise tests of the complex Kronecker-split SpMV (qbh_split.cpp kron_build, qbh_spmv_kron.cpp
spmv_kron, k_spmv_wave2 and the kernels of qbh_kron.hip / qbh_kron_prep.hip), in the style of tests/csrforms.py.

Three parts, none of which needs a GPU:

* synthetic product-structured operators.  index = u * S + d (major u < NU, minor d < S); row (u, d) has NEAR entries at the columns
  (u, d') and FAR entries at the columns (u', d), u' != u.  Values are complex with 0.5 <= |a| <= 2, vectors have 0.5 <= |x_j| <= 1,
  so no term of a row can vanish.  The operators are not Hermitian (check_hermitian = 0).  Each profile is the smallest shape at which
  one path of the split is still reached (PROFILES);
* a mirror of the structural choices (`route`: what qbh_csr_info must report) and of the launch geometry (`paths`: which of the
  internal paths an (operator, options) pair reaches), written from the rules of kron_build, kron_short_cols, wave_geometry_for,
  k_build_wavedesc / k_build_slotdesc and the buffer logic of k_spmv_wave2;
* the error bounds (`epilogue`, `step_bound`).

Bounds.  On one GPU a row's sum is still a summation tree over its nnz_i products: the far pass sums the far products of the row
(k_spmv_wave2 OPS 0 / 3, k_kron_cross_rows for the rows of a narrow last band), the near pass sums the near products and adds the far
partial to them before the epilogue (OPS 2 / 4).  A group cut by a block boundary is two partials added (into a zeroed slot, or in
the wave-private buffer); padding slots contribute exact zeros.  So csrforms.epilogue's

    |y_i - ref_i| <= (nnz_i + 4) eps S_i,     S_i = |alpha| sum_j |a_ij||x_j| + |beta||y_i| + |gamma||x_i|

holds unchanged.  (A far term of a row with fewer than two near entries whose group is cut passes through nnz_i additions instead
of nnz_i - 1: gamma_{m+5} instead of gamma_{m+4}, and sqrt(2) * 1.01 * (m + 5) u < 0.72 (m + 5) eps <= (m + 4) eps for every m >= 0,
so the constant 4 covers it.)

Two forms differ, each by roundings counted in the kernels (u = eps / 2):

* under a communicator the near pass finishes y1 = fl(alpha * near + beta * y + gamma * x) WITHOUT the far addend (OPS 1: gamma_{nn+4}
  on the near terms, gamma_3 on the others) and k_kron_combine then stores fl(y1 + fl(alpha * far)): the far terms carry gamma_{nf+1}
  from the far pass (one more where the group is cut), one product with alpha and the final addition, gamma_{nf+4} at most; every
  term of y1 takes the final addition as well, gamma_{nn+5}.  With nn, nf <= nnz_i that is k = 5 in place of 4: COMBINE_EXTRA = 1.
* several classes with the entries across the cut in a pass of their own (kron_cross_in_near = 0): the near pass (OPS 4) finishes
  y1 from the near and far terms, the third pass (k_spmv_wave with beta = 1, gamma = 0, both exact) stores fl(fl(alpha * cross) + y1):
  gamma_{nx+3} on the cross terms, one addition more on every term of y1.  k = 5 again: CROSS_PASS_EXTRA = 1.
* the solver's step (step_bound): see there.
"""
from functools import lru_cache

import numpy as np

import csrforms as cf
from csrforms import CL, EPS, L, probe_vector, row_sums, worst      # noqa: F401  (re-exported for the tests)

CAP = 256                  # rows of k_spmv_wave2's wave-private result buffer
SLOT_BLOCK = 512           # slots of a block of the sliced far stream (= the wave tile)
MAX_GROUP = 504            # kron_build: the longest group the sliced form accepts
DYN_CHUNK = cf.K_DYN_CHUNK
COMBINE_EXTRA = 1
STEP_EXTRA = 5
CROSS_PASS_EXTRA = 1

FAR_L = (1, 2, 4, 8, 17, 63)
NEAR_M = (200, 300, 600)


# ------------------------------------------------------------------------------------------------------------ profiles --
def _near_mix(d, M):
    """near lengths of the near_M profiles by minor index: twelve short rows (7, 1, 0 in turn) -- a block then holds more rows than
    one reduction pass of 64 / TPR = 8 -- followed by twenty rows alternating M and 7 (average > 64: TPR 8)."""
    k = d % 32
    short = np.array([7, 1, 0])[k % 3]
    return np.where(k < 12, short, np.where(k % 2 == 0, M, 7))


def _spec(name):
    """-> (NU, S, near(u, d), far(u, d), diag, opts): lengths as functions of the index arrays; opts: creation options of its own."""
    if name == "tiny":
        return 2, 8, lambda u, d, rng: rng.integers(1, 4, size=u.shape), lambda u, d, rng: 1 + 0 * u, False, {}
    if name in ("uniform", "graded"):
        # 102 x 64 where 96 x 64 was planned: 96 * 64 * 5 far slots are exactly 60 blocks of 512, and the last XCD region (60 - 7 * 8 = 4
        # blocks) would hold ONE chunk of the dynamic walk; 102 * 64 * 5 slots are 64 blocks (8 per region) beside 79 near blocks (10 per
        # region, 9 in the last): two chunks or more in every region of both passes
        return 102, 64, lambda u, d, rng: 6 + 0 * u, lambda u, d, rng: 5 + 0 * u, True, {}
    if name == "edge":
        return 33, 61, lambda u, d, rng: 4 + 0 * u, lambda u, d, rng: 3 + 0 * u, False, {}
    if name == "edge_small":
        return 3, 9, lambda u, d, rng: 2 + 0 * u, lambda u, d, rng: 2 + 0 * u, False, {}
    if name == "narrow":
        # kron_band = 4: with the default band of 8 an operator with S = 5 has no full band, hence no far part, and stays unsplit
        # (kron_build: nnz_f == 0); band 4 leaves one full band and one edge row per major index, never sliced (B != 8, S < 8)
        return 50, 5, lambda u, d, rng: 2 + 0 * u, lambda u, d, rng: 2 + 0 * u, False, dict(kron_band=4)
    if name == "ragged_light":
        return 64, 64, lambda u, d, rng: 4 + 0 * u, lambda u, d, rng: np.where(d % 32 == 31, 5, 4), False, {}
    if name in ("ragged_heavy", "ragged_heavy_s2"):
        return (64, 64, lambda u, d, rng: (d + 3) % 5, lambda u, d, rng: np.where(u % 7 == 0, 0, d % 8), False,
                dict(kron_sliced=2) if name.endswith("_s2") else {})
    if name.startswith("far_") and name[4:].isdigit():
        ln = int(name[4:])
        return 80, 32, lambda u, d, rng: 3 + 0 * u, lambda u, d, rng: ln + 0 * u, False, dict(kron_sliced=2) if ln == 64 else {}
    if name.startswith("near_"):
        m = int(name[5:])
        near = (lambda u, d, rng: 40 + 0 * u) if m == 40 else (lambda u, d, rng: _near_mix(d, m))
        return 6, 640, near, lambda u, d, rng: 1 + d % 2, False, {}
    if name == "far_plain_long":
        return 600, 8, lambda u, d, rng: 2 + 0 * u, lambda u, d, rng: np.where(d == 0, 599, 1 + (u + d) % 3), False, dict(kron_sliced=0)
    if name == "wide_major":
        # kron_band = 8: by itself kron_build halves the band at NUg = 33000 (33000 * 8 * 16 > 2.5e6), the far part is then never
        # sliced and the 2 NUg <= 65536 rule of kron_short_cols is never asked; with band 8 the far part is sliced, sits inside the
        # operator's arrays and keeps int32 columns for that rule alone
        return 33000, 8, lambda u, d, rng: 2 + 0 * u, lambda u, d, rng: 2 + 0 * u, False, dict(kron_band=8)
    if name == "wide_minor":
        return 8, 33000, lambda u, d, rng: 2 + 0 * u, lambda u, d, rng: 2 + 0 * u, False, {}
    raise KeyError(name)


PROFILES = (["tiny", "uniform", "graded", "edge", "edge_small", "narrow", "ragged_light", "ragged_heavy", "ragged_heavy_s2"]
            + ["far_%d" % ln for ln in FAR_L] + ["far_64"] + ["near_%d" % m for m in NEAR_M] + ["near_40", "far_plain_long",
                                                                                                  "wide_major", "wide_minor"])


def profile_opts(name):
    """Creation options a profile needs beside the common ones (kron_band, kron_sliced)."""
    return dict(_spec(name)[5])


def _seed(name, seed):
    h = 0
    for ch in "kron/%s/%d" % (name, seed):
        h = (h * 131 + ord(ch)) % (2 ** 31)
    return h


def _targets(lens, pos, n, lo, rng, force0):
    """Per row `lens` distinct targets (pos + offset) % n with offsets in [lo, n): one sorted offset set per length."""
    rows_out, tgt_out = [], []
    for ln in np.unique(lens):
        ln = int(ln)
        if ln == 0:
            continue
        rows = np.nonzero(lens == ln)[0]
        if force0:
            offs = np.concatenate([[0], rng.choice(np.arange(1, n), size=ln - 1, replace=False)])
        else:
            offs = rng.choice(np.arange(lo, n), size=ln, replace=False)
        tgt = (pos[rows][:, None] + np.sort(offs)[None, :]) % n
        rows_out.append(np.repeat(rows, ln))
        tgt_out.append(tgt.reshape(-1))
    if not rows_out:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(rows_out), np.concatenate(tgt_out)


def row_scale(name, dim):
    """graded: row r is scaled by 2^((37 r) % 41 - 20) (exact); None otherwise."""
    if name != "graded":
        return None
    return np.ldexp(1.0, ((37 * np.arange(dim, dtype=np.int64)) % 41 - 20).astype(np.int64))


@lru_cache(maxsize=4)
def make(name, seed=0):
    """-> (dim, ia, ja, val, S, NU) with dim = NU * S: full-storage CSR, columns sorted and distinct in every row.  The arrays are
    shared between callers: leave them unchanged."""
    NU, S, near, far, diag, _ = _spec(name)
    rng = np.random.default_rng(_seed("uniform" if name == "graded" else name, seed))      # graded: the same structure and phases
    u, d = np.divmod(np.arange(NU * S, dtype=np.int64), S)
    nl = np.asarray(near(u, d, rng), dtype=np.int64)
    fl = np.asarray(far(u, d, rng), dtype=np.int64)
    assert nl.max() <= S and fl.max() <= NU - 1
    rn, tn = _targets(nl, d, S, 0, rng, diag)
    rf, tf = _targets(fl, u, NU, 1, rng, False)
    row = np.concatenate([rn, rf])
    col = np.concatenate([u[rn] * S + tn, tf * S + d[rf]])
    o = np.lexsort((col, row))
    row, col = row[o], col[o]
    dim = NU * S
    ia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=dim), out=ia[1:])
    nnz = len(col)
    val = (rng.uniform(0.5, 2.0, nnz) * np.exp(2j * np.pi * rng.random(nnz))).astype(np.complex128)
    sc = row_scale(name, dim)
    if sc is not None:
        val = val * sc[row]
    for a in (ia, col, val):
        a.setflags(write=False)
    return dim, ia, col, val, S, NU


def probe(name, dim, seed):
    """csrforms.probe_vector; graded: x_j scaled by 2^((13 j) % 23 - 11)."""
    x = probe_vector(dim, seed)
    if name == "graded":
        x = x * np.ldexp(1.0, ((13 * np.arange(dim, dtype=np.int64)) % 23 - 11).astype(np.int64))
    return x


def structure(ia, ja, S, dim):
    """The structure check: ia consistent, columns sorted and distinct and in range, every entry keeps the major or the minor index.
    -> (near lengths, far lengths) per row."""
    assert ia[0] == 0 and len(ia) == dim + 1 and np.all(np.diff(ia) >= 0) and ia[-1] == len(ja)
    assert len(ja) == 0 or (ja.min() >= 0 and ja.max() < dim)
    row = np.repeat(np.arange(dim, dtype=np.int64), np.diff(ia))
    same_row = row[1:] == row[:-1]
    assert np.all(ja[1:][same_row] > ja[:-1][same_row]), "columns are not sorted and distinct"
    near = ja // S == row // S
    farm = (ja % S == row % S) & ~near
    assert np.all(near | farm), "an entry changes both indices"
    return np.bincount(row[near], minlength=dim), np.bincount(row[farm], minlength=dim)


# -------------------------------------------------------------------------------------------------------------- mirror --
def _tile(r, S, NU, B):
    """KronTile{S, NU, B}::tile of local rows r (qbh_internal.hpp)."""
    u, d = np.divmod(r, S)
    b, j = np.divmod(d, B)
    wB = np.minimum(S - b * B, B)
    return b * B * NU + u * wB + j


def route(ia, ja, S, opts=None, rows=None):
    """What qbh_csr_info must report for an operator (or the row shard rows = (r0, r1) of whole major indices) created from these
    host arrays with kron_split = 2, kron_minor = S and `opts` (kron_band, kron_sliced, kron_cols16; defaults 0, 1, 1), and the
    geometry of its passes.  kron_far_nnz counts the far entries themselves, never the padding slots of the sliced form
    (qbh_api.cpp reports KronSplit::nnz_f, which kron_build sets to the scan of the far counts in both forms)."""
    o = dict(kron_band=0, kron_sliced=1, kron_cols16=1)
    o.update(opts or {})
    ncols = len(ia) - 1
    r0, r1 = (0, ncols) if rows is None else rows
    n = r1 - r0
    off = dict(active=False, kron_minor=0, kron_band=0, kron_sliced=0, kron_inplace=0, kron_far_nnz=0, kron_cross_nnz=0, kron_cols16=0)
    if S <= 1 or S >= ncols or ncols % S or n % S or r0 % S or ia[r1] == ia[r0]:
        return off
    NU, NUg, U0 = n // S, ncols // S, r0 // S
    lia = ia[r0:r1 + 1] - ia[r0]
    lja = ja[ia[r0]:ia[r1]]
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(lia))
    u, d = np.divmod(row, S)
    is_near = lja // S == U0 + u
    if not np.all(is_near | (lja % S == d)):
        return off                                            # one entry that changes both indices: unsplit
    B = 8
    while B > 2 and NUg * B * 16 > 2.5e6:
        B >>= 1
    if o["kron_band"] in (2, 4, 8, 16):
        B = o["kron_band"]
    edge_row = (np.arange(n) % S) >= (S // B) * B
    is_cross = ~is_near & edge_row[row]
    is_far = ~is_near & ~is_cross
    cn = np.bincount(row[is_near], minlength=n)
    cfar = np.bincount(row[is_far], minlength=n)
    cx = np.bincount(row[is_cross], minlength=n)
    nnz_n, nnz_f, nnz_x = int(cn.sum()), int(cfar.sum()), int(cx.sum())
    if nnz_f == 0:
        return off
    nnz = nnz_n + nnz_f + nnz_x
    ia_n = np.concatenate([[0], np.cumsum(cn)])
    want = o["kron_sliced"]
    sliced = False
    gia = None
    if want and B == 8 and S >= 8:
        nfr = (S // B) * B * NU
        full = np.nonzero(~edge_row)[0]
        cf_t = np.zeros(nfr, dtype=np.int64)
        cf_t[_tile(full, S, NU, B)] = cfar[full]                 # far counts in far-row (tiled) order
        gw = 8 * np.maximum(cf_t.reshape(-1, 8).max(axis=1), 1)
        slots, maxgw = int(gw.sum()), int(gw.max())
        if (want == 2 or slots - nnz_f <= nnz_f // 8) and maxgw <= MAX_GROUP and len(gw) > 0:
            sliced = True
            gia = np.concatenate([[0], np.cumsum(gw)])
    r = dict(active=True, kron_minor=S, kron_band=B, kron_sliced=int(sliced), kron_inplace=1, kron_far_nnz=nnz_f, kron_cross_nnz=nnz_x,
             S=S, NU=NU, NUg=NUg, U0=U0, B=B, nnz_n=nnz_n, nnz_x=nnz_x, cn=cn, cfar=cfar, cx=cx, ia_n=ia_n, n=n)
    if sliced:
        far_slots = int(gia[-1])
        r.update(gia=gia, far_slots=far_slots, maxgw=int(np.diff(gia).max()), nwb_f=max(1, -(-far_slots // SLOT_BLOCK)))
    else:
        cf_t = np.zeros(n, dtype=np.int64)
        cf_t[_tile(np.arange(n), S, NU, B)] = cfar              # plain far rows in tiled order; the edge rows have none
        ia_f = np.concatenate([[0], np.cumsum(cf_t)])
        far_slots = nnz_f
        g = cf.wave_geometry(ia_f)
        r.update(ia_f=ia_f, far_slots=far_slots, window_f=g["window"], nwb_f=g["n_wb"])
    g = cf.wave_geometry(ia_n)
    r.update(window_n=g["window"], nwb_n=g["n_wb"])
    # wave_geometry_for: both averages are over the rows of the operator; TPR 16 does not exist for the pipelined kernel
    r["tpr_n"] = 2 if nnz_n / n <= 32 else 4 if nnz_n / n <= 64 else 8
    r["tpr_f"] = 2 if nnz_f / n <= 32 else 4 if nnz_f / n <= 64 else 8
    # where the parts live (kron_build): the cross part keeps its scratch arrays from 32 entries on, which leaves room to align the far part
    own_x = nnz_x >= 32
    tail = nnz_n
    if own_x and -(-nnz_n // 32) * 32 + far_slots <= nnz:
        tail = -(-nnz_n // 32) * 32
    own_far = not (tail + far_slots + (0 if own_x else nnz_x) <= nnz)
    r.update(own_x=own_x and nnz_x > 0, own_far=own_far)
    # 2-byte columns (kron_short_cols): tried where 2 S (near) / 2 NUg (sliced far part inside the operator's arrays, band 8) fit 16 bits,
    # kept where every value does (near: column - first column of the major index of the block's first row; far: target major index
    # + (band - band of the block's first group) * NUg)
    c16 = 0
    if o["kron_cols16"]:
        if nnz_n > 0 and 2 * S <= 65536:
            rb = cf.block_starts(ia_n, r["window_n"], r["nwb_n"])
            cnt = ia_n[rb[1:]] - ia_n[rb[:-1]]
            base = np.repeat((rb[:-1] // S) * S, cnt)
            rel = lja[is_near] - U0 * S - base
            if len(rel) == 0 or rel.max() < 65536:
                c16 |= 1
        if sliced and not own_far and B == 8 and 2 * NUg <= 65536 and far_slots > 0:
            P = np.arange(r["nwb_f"], dtype=np.int64) * SLOT_BLOCK
            g0 = np.searchsorted(gia, P, side="right") - 1
            g1 = np.searchsorted(gia, np.minimum(P + SLOT_BLOCK, far_slots), side="left") - 1
            if ((g1 // NU - g0 // NU + 1) * NUg).max() <= 65536:
                c16 |= 2
    r["kron_cols16"] = c16
    return r


INFO_FIELDS = ("kron_minor", "kron_band", "kron_sliced", "kron_inplace", "kron_far_nnz", "kron_cross_nnz", "kron_cols16")

ALL_PATHS = {
    # structure
    "sliced", "sliced_padded", "far_plain", "far_own_arrays", "cols16_near", "cols16_far", "cols32_near_wide", "cols32_far_wide",
    "cross_rows", "cross_own_arrays", "cross_behind_far", "tile_edge", "tile8_ragged_nu", "minor_below_8", "over_group_limit",
    # rows
    "rows_no_far", "rows_no_near", "rows_empty", "groups_empty",
    # launch
    "one_block_pass", "empty_xcd_region", "two_chunks_per_region",
    # sliced far pass (OPS 3)
    "far_64_groups", "far_direct_store", "far_buffer_overflow", "far_cut_groups", "far_group_at_limit",
    # plain far pass (OPS 0)
    "far_rowpath",
    # near pass (OPS 1 / 2)
    "near_window_by_maxlen", "near_window_249", "near_rowpath", "near_rbase", "near_rbase_tpr8", "near_tpr2", "near_tpr4", "near_tpr8",
}


def _regions(n_wb):
    """Blocks in each of the 8 XCD regions of the ordered dynamic walk (DynWalk::init)."""
    per = (n_wb + 7) >> 3
    return [max(0, min((k + 1) * per, n_wb) - k * per) for k in range(8)]


def far_blocks(r):
    """Blocks of the sliced far stream (k_build_slotdesc, shift 0): first group, groups overlapped, first group continues the block
    before, last group goes on in the block after."""
    gia, slots = r["gia"], r["far_slots"]
    P0 = np.arange(r["nwb_f"], dtype=np.int64) * SLOT_BLOCK
    P1 = np.minimum(P0 + SLOT_BLOCK, slots)
    g0 = np.searchsorted(gia, P0, side="right") - 1
    g1 = np.searchsorted(gia, P1, side="left")                 # first group that starts at or behind the block's end
    return g0, g1 - g0, gia[g0] < P0, gia[g1] > P1


def paths(ia, ja, S, opts=None, rows=None):
    """The internal paths (ALL_PATHS) this operator reaches under the ordered dynamic walk (the default) and the static walks."""
    r = route(ia, ja, S, opts, rows)
    out = set()
    o = dict(kron_band=0, kron_sliced=1, kron_cols16=1)
    o.update(opts or {})
    if not r["active"]:
        return out
    NU, NUg, B = r["NU"], r["NUg"], r["B"]
    cn, cfar, cx = r["cn"], r["cfar"], r["cx"]
    if S < 8:
        out.add("minor_below_8")
    if S % B:
        out.add("tile_edge")
    if B == 8 and NUg % 32:
        out.add("tile8_ragged_nu")
    if r["nnz_x"] > 0:
        out.add("cross_rows")
        out.add("cross_own_arrays" if r["own_x"] else "cross_behind_far")
    if r["kron_cols16"] & 1:
        out.add("cols16_near")
    if r["kron_cols16"] & 2:
        out.add("cols16_far")
    if r["nnz_n"] > 0 and 2 * S > 65536:
        out.add("cols32_near_wide")
    if r["kron_sliced"] and not r["own_far"] and B == 8 and r["far_slots"] > 0 and 2 * NUg > 65536:
        out.add("cols32_far_wide")                            # every other term of kron_short_cols' rule holds: 2 NUg decides
    if np.any((cfar + cx == 0) & (cn > 0)):
        out.add("rows_no_far")
    if np.any((cn == 0) & (cfar + cx > 0)):
        out.add("rows_no_near")
    if np.any(cn + cfar + cx == 0):
        out.add("rows_empty")
    for n_wb in (r["nwb_n"], r["nwb_f"]):
        if n_wb == 1:
            out.add("one_block_pass")
        if min(_regions(n_wb)) == 0:
            out.add("empty_xcd_region")
    if all(min(_regions(n_wb)) > DYN_CHUNK for n_wb in (r["nwb_n"], r["nwb_f"])):
        out.add("two_chunks_per_region")
    # ---- far pass
    if r["kron_sliced"]:
        out.add("sliced")
        gw = np.diff(r["gia"])
        if r["far_slots"] > r["kron_far_nnz"]:
            out.add("sliced_padded")
        if r["own_far"]:
            out.add("far_own_arrays")
        nfr = len(gw) * 8
        cf_t = np.zeros(nfr, dtype=np.int64)
        full = np.nonzero((np.arange(r["n"]) % S) < (S // B) * B)[0]
        cf_t[_tile(full, S, NU, B)] = cfar[full]
        if np.any(cf_t.reshape(-1, 8).max(axis=1) == 0):
            out.add("groups_empty")
        if gw.max() > MAX_GROUP - 8:
            out.add("far_group_at_limit")
        g0, ng, c0, c1 = far_blocks(r)
        if np.any(ng == 64):
            out.add("far_64_groups")
        if np.any(c0):
            out.add("far_cut_groups")
        if np.any(8 * ng > CAP):
            out.add("far_direct_store")
        # the wave-private buffer over the blocks of one chunk (kDynChunk consecutive blocks of an XCD region: one wavefront, in order)
        per = (r["nwb_f"] + 7) >> 3
        for k in range(8):
            lo, hi = k * per, min((k + 1) * per, r["nwb_f"])
            for c in range(lo, hi, DYN_CHUNK):
                buf_r0, buf_n = 0, 0
                for b in range(c, min(c + DYN_CHUNK, hi)):
                    first, nrows = int(g0[b]) * 8, int(ng[b]) * 8
                    if buf_n > 0 and first == buf_r0 + buf_n - (8 if c0[b] else 0) and nrows <= CAP and first + nrows - buf_r0 > CAP:
                        out.add("far_buffer_overflow")
                    if buf_n > 0 and (first != buf_r0 + buf_n - (8 if c0[b] else 0) or first + nrows - buf_r0 > CAP):
                        buf_n = 0
                    if nrows > CAP:
                        buf_n = 0
                        continue
                    if buf_n == 0:
                        buf_r0 = first
                    buf_n = first + nrows - buf_r0
    else:
        out.add("far_plain")
        if o["kron_sliced"] == 2 and B == 8 and S >= 8:
            out.add("over_group_limit")
        pf = cf.paths(dict(kernel="wave", window=r["window_f"], n_wb=r["nwb_f"], tpr=r["tpr_f"]), r["ia_f"])
        if "wave_rowpath" in pf:
            out.add("far_rowpath")
    # ---- near pass
    maxlen = int(cn.max())
    out.add("near_window_by_maxlen" if maxlen <= 256 else "near_window_249")
    out.add("near_tpr%d" % r["tpr_n"])
    pn = cf.paths(dict(kernel="wave", window=r["window_n"], n_wb=r["nwb_n"], tpr=r["tpr_n"]), r["ia_n"])
    if "wave_rowpath" in pn:
        out.add("near_rowpath")
    if "wave_rbase" in pn:
        out.add("near_rbase")
        if r["tpr_n"] == 8:
            out.add("near_rbase_tpr8")
    return out


# -------------------------------------------------------------------------------------------------------------- bounds --
def epilogue(s, abs_s, nnz_row, xl, y0, alpha, beta, gamma, extra=0):
    """csrforms.epilogue with the constant 4 + extra: the per-row bound (nnz_i + 4 + extra) eps S_i and the reduction bounds built
    from it by the same formulas (see the module docstring for extra = COMBINE_EXTRA)."""
    ref = cf.epilogue(s, abs_s, nnz_row, xl, y0, alpha, beta, gamma)
    if extra:
        k = nnz_row.astype(L)
        e = ref["bound"] * (k + 4 + extra) / (k + 4)
        n = L(len(s))
        ax, ay = np.abs(xl).astype(L), np.abs(ref["y"])
        ref["bound"] = e
        ref["t_dot"] = np.sum(ax * e) + (n + 2) * L(EPS) * np.sum(ax * (ay + e))
        ref["t_nrm"] = np.sum(e * (2 * ay + e)) + (n + 2) * L(EPS) * np.sum((ay + e) ** 2)
    return ref


def step_bound(s, abs_s, nnz_row, v, a, vprev, b):
    """The solver's three-term step on v = v_j (as the caller gets it back) and v_{j-1}, with the step's own a = a_j, b = b_j:
    reference w = H v - b vprev, bound E on the reconstruction  b_{j+1} v_{j+1} + a v + b vprev  of H v, and the tolerances of a_j and
    b_{j+1}.  s, abs_s = row_sums of the host arrays with v.

    Roundings, counted in lanczos_core, k_lanczos_tail, k_axpy_norm_tile / k_axpy_norm and k_scal_to (u = eps / 2, scale
    T_i = sum_j |a_ij||v_j| + |a v_i| + |b vprev_i|; every scaling is by a REAL number, so it acts on both components alike and needs
    no sqrt 2).  The device holds u_j with v_j = fl(sc u_j), sc = fl(1 / b_j):
      * the SpMV forms fl(sc * sum a_ij u_j + beta * vprev_i) with beta = -b_j (times the scale of v_{j-1}, 1 for a vector handed in):
        (nnz_i + 4) eps on sum |a_ij||sc u_j| + |b vprev_i|; and sc u_j = v_j (1 + d), 1 u on the first sum             [2 (nnz_i + 4) + 1] u
      * the axpy subtracts c u_j with c = fl(fl(-sc * sc) * dot) while a = fl(sc * dot): c u_j = a v_i (1 + d)^4, one product and
        one addition more                                                                                                 6 u on |a v_i|
      * the result w' leaves as v_{j+1} = fl(fl(1 / b_{j+1}) * w') with b_{j+1} = fl(sqrt(sq)): b_{j+1} v_{j+1} = w' (1 + d)^3         3 u on |w'_i| <= T_i
    10 u T_i = 5 eps T_i beyond the row bound: E_i = (nnz_i + 4 + STEP_EXTRA) eps T_i with STEP_EXTRA = 5.  Second order: the ten
    roundings are gamma_10 <= 1.01 * 10 u = 5.05 eps, and the row bound spends only sqrt(2) * 1.01 * (nnz_i + 4) u < 0.72 (nnz_i + 4) eps
    of its (nnz_i + 4) eps (csrforms.epilogue), which leaves more than 1.1 eps for the 0.05.  The coefficients do not depend on lanczos_pipeline: both loops multiply in the same association.

      a_j = fl(sc * <u_j, w~>) = <v_j, w~> up to (n + 2) eps of the absolute sum:  |a - ref| <= sum |v_i| E_i + (n + 10) eps sum |v_i| (|w_i| + E_i)
      b_{j+1} = |w~ - a v| (square root of a sum of n squares):              |b' - ref| <= |E|_2 + (n + 10) eps ref
    """
    vl, pl = v.astype(CL), vprev.astype(CL)
    w = s - L(b) * pl
    T = abs_s + np.abs(L(a) * vl) + np.abs(L(b) * pl)
    E = (nnz_row.astype(L) + 4 + STEP_EXTRA) * L(EPS) * T
    n = L(len(v))
    av = np.abs(vl)
    a_ref = np.sum(np.conj(vl) * w).real
    t_a = np.sum(av * E) + (n + 10) * L(EPS) * np.sum(av * (np.abs(w) + E))
    res = w - L(a) * vl
    b_ref = np.sqrt(np.sum(res.real * res.real + res.imag * res.imag))
    t_b = np.sqrt(np.sum(E * E)) + (n + 10) * L(EPS) * b_ref
    return dict(y=s, bound=E, w=w, a=a_ref, t_a=t_a, b=b_ref, t_b=t_b)


def cut_rows(r):
    """Local rows whose far group a block boundary of the sliced far stream cuts: their far sum is two partials added, so it
    depends on where the cut falls (the same operator always cuts at the same slots; a row shard cuts elsewhere)."""
    out = np.zeros(r["n"], dtype=bool)
    if not r["kron_sliced"]:
        return out
    g0, ng, c0, c1 = far_blocks(r)
    S, NU, B = r["S"], r["NU"], r["B"]
    for g in g0[c0]:
        b, u = divmod(int(g), NU)
        out[u * S + b * B:u * S + b * B + B] = True
    return out


def worst_row(got, ref, S, near, far):
    """csrforms.worst as text: the worst row as (u, d), its near and far lengths, its error / bound."""
    i, ratio, over, err = worst(got, ref)
    return ratio, "row %d = (u, d) = (%d, %d), %d near + %d far entries: |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
        i, i // S, i % S, int(near[i]), int(far[i]), err, float(ref["bound"][i]), ratio, over)
