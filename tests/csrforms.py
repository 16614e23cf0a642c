"""Host-only helpers for the element-wise tests of the complex CSR SpMV forms (k_spmv_stream, k_spmv_vector, k_spmv_rows,
k_spmv_wave) and their fused epilogue y <- alpha*Hx + beta*y + gamma*x_local with the reductions <x_local, y> and |y|^2.

Three parts, none of which needs a GPU:

* row-length profiles -> full-storage CSR (sorted distinct columns per row) or Hermitian upper storage, with four kinds of
  values (random complex, real, <= 256 distinct, 257..65536 distinct);
* a mirror of the launch geometry (qbh_api.cpp setup_geometry / setup_wave_geometry / build_geometry, qbh_spmv_csr.hip spmv_grid
  and the walks BlockWalk / DynWalk) that names the kernel, the template instance and the coding an (operator, options) pair
  runs, which block paths it reaches, and a lower bound on the blocks each persistent workgroup walks;
* a long-double reference of the epilogue and both reductions with per-row error bounds (see `epilogue`).
"""
from fractions import Fraction

import numpy as np

EPS = np.finfo(np.float64).eps
L = np.longdouble
CL = np.clongdouble

# QBH_KERNEL_* (include/qbhip.h)
KERNEL_AUTO, KERNEL_STREAM, KERNEL_VECTOR, KERNEL_ROWS, KERNEL_MATRIX_FREE, KERNEL_WAVE = 0, 1, 2, 3, 4, 5
KERNEL_NAMES = {KERNEL_STREAM: "stream", KERNEL_VECTOR: "vector", KERNEL_ROWS: "rows", KERNEL_WAVE: "wave"}

# qbh_internal.hpp
K_BLOCK = 256
K_DICT_LDS = 1024
K_ROW_CAP = 1024
K_DYN_CHUNK = 4          # qbh_device.hpp QBH_DYN_CHUNK
WAVE_TILE = 512          # k_spmv_wave: 64 lanes x U = 8
MAX_WG_PER_CU = 8        # 32 wavefronts per CU, 4 per workgroup: no occupancy query can return more
GRID_CAP = 4096          # largest grid spmv_grid() returns (256 * 4 * 4, 256 * 8 * 2); also >= 8 workgroups x 256 CUs


# ------------------------------------------------------------------------------------------------------------ profiles --
def _lengths(spec, rng):
    """Row lengths (full storage) of a profile spec: a list of (count, length) runs, repeated `rep` times."""
    out = []
    for _ in range(spec.get("rep", 1)):
        for cnt, ln in spec["runs"]:
            out.append(np.full(cnt, ln, dtype=np.int64))
    lens = np.concatenate(out) if out else np.zeros(0, dtype=np.int64)
    if "random" in spec:
        lo, hi = spec["random"]
        lens = rng.integers(lo, hi + 1, size=spec["n"]).astype(np.int64)
    return lens


# name -> spec.  `n` rows; `runs` (count, length) pairs of the full-storage row lengths; `kinds` the value kinds it is run with.
# Buckets (avg = nnz / nrows): stream tpr 1|2|4|8|16 at avg <= 3|8|48|128|>; vector 2|4|8|16|32|64 at <= 24|96|192|512|2048|>;
# rows coded 1|2|4|8 at <= 64|128|256|>, uncoded 1|4|8 at <= 12|96|>; wave 2|4|8|16 at <= 32|64|128|>.
PROFILES = {
    "const1": dict(runs=[(1, 0), (4998, 1), (1, 0)], kinds=("complex", "few", "real")),
    "const6": dict(runs=[(3000, 6)], kinds=("complex", "few")),
    "const20": dict(runs=[(1, 0), (2999, 20)], kinds=("complex", "few", "mid", "many")),
    "const40": dict(runs=[(2000, 40)], kinds=("complex", "few")),
    "const80": dict(runs=[(1500, 80), (1, 0)], kinds=("complex", "few", "mid", "many")),
    "const112": dict(runs=[(1200, 112)], kinds=("complex", "few")),
    "const200": dict(runs=[(1200, 200)], kinds=("complex", "few", "mid", "many")),
    "const400": dict(runs=[(1, 0), (1000, 400), (1, 0)], kinds=("complex", "few", "mid", "many")),
    "const1000": dict(runs=[(1500, 1000)], kinds=("complex", "few")),
    "const2100": dict(runs=[(2200, 2100)], kinds=("complex", "few")),
    # wave blocks holding more rows than one pass of 64 / TPR lanes covers (rbase > 0), one profile per wave TPR
    "bimodal300": dict(runs=[(1, 300), (100, 1)], rep=40, kinds=("complex", "few")),
    "bimodal_t2": dict(runs=[(1, 200), (60, 1)], rep=50, kinds=("complex",)),
    "bimodal_t4": dict(runs=[(5, 200), (24, 1)], rep=50, kinds=("complex",)),
    "bimodal_t8": dict(runs=[(6, 200), (12, 1)], rep=50, kinds=("complex",)),
    "bimodal_t16": dict(runs=[(11, 200), (6, 1)], rep=50, kinds=("complex",)),
    # runs of > 2 x kRowCap empty rows and thousands of 1-entry rows: the kRowCap row groups and the oversized blocks
    "empty_runs": dict(runs=[(3, 0), (1500, 5), (2600, 0), (500, 5), (6000, 1), (3100, 0), (200, 5), (2, 0)],
                       kinds=("complex", "few", "mid")),
    # single rows longer than npb (8192) and longer than the 512-entry wave tile, first and last row empty
    "long_rows": dict(runs=[(1, 0), (6000, 5), (1, 9000), (2000, 5), (1, 600), (3000, 3), (1, 4500), (1, 0)],
                      kinds=("complex", "few")),
    "n1": dict(runs=[(1, 1)], kinds=("complex",)),
    "n2": dict(runs=[(1, 2), (1, 1)], kinds=("complex",)),
    "n63": dict(n=63, runs=[], random=(0, 63), kinds=("complex", "few")),
    "n64": dict(n=64, runs=[], random=(0, 64), kinds=("complex",)),
    "n65": dict(n=65, runs=[], random=(0, 65), kinds=("complex", "real")),
}
# Hermitian upper storage (sym=True): row lengths of the stored upper triangle; the device expands it
SYM_PROFILES = {
    "sym_rand": dict(n=3000, upper=(1, 30), kinds=("complex", "few")),
    "sym_wide": dict(n=1500, upper=(1, 400), kinds=("complex",)),
}

VALUE_COUNTS = {"few": 200, "mid": 600, "many": 5000}


def _values(kind, nnz, rng):
    if kind == "complex":
        return rng.uniform(0.5, 1.0, nnz) * np.exp(2j * np.pi * rng.random(nnz))
    if kind == "real":
        return (rng.uniform(0.5, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(np.complex128)
    m = VALUE_COUNTS[kind]
    table = rng.uniform(0.5, 1.0, m) * np.exp(2j * np.pi * rng.random(m))
    return table[rng.integers(0, m, nnz)]


def _columns(lens, n, rng):
    """Sorted distinct columns in [0, n) for rows of the given lengths: per length one random offset set, per row a random shift."""
    ja = np.empty(int(lens.sum()), dtype=np.int64)
    ia = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=ia[1:])
    for ln in np.unique(lens):
        if ln == 0:
            continue
        rows = np.nonzero(lens == ln)[0]
        offs = np.sort(rng.choice(n, size=int(ln), replace=False))
        shift = rng.integers(0, n, size=len(rows))
        cols = np.sort((offs[None, :] + shift[:, None]) % n, axis=1)
        idx = ia[rows][:, None] + np.arange(ln)[None, :]
        ja[idx] = cols
    return ia, ja


def make(name, kind, seed=0):
    """-> dict(n, ia, ja, val, sym, full=(ia, ja, val)): host arrays to hand to csr_mat and the full-storage CSR they mean."""
    rng = np.random.default_rng(_seed(name, kind, seed))
    if name in SYM_PROFILES:
        spec = SYM_PROFILES[name]
        n = spec["n"]
        lo, hi = spec["upper"]
        rows, cols = [], []
        for r in range(n):
            k = min(int(rng.integers(lo, hi + 1)), n - r)
            c = np.sort(r + rng.choice(n - r, size=k, replace=False))
            if c[0] != r:
                c = np.sort(np.concatenate([[r], c[1:]]))      # the diagonal always stored (real)
            rows.append(np.full(len(c), r))
            cols.append(c)
        r_u, c_u = np.concatenate(rows), np.concatenate(cols)
        v_u = _values(kind, len(r_u), rng)
        diag = r_u == c_u
        v_u[diag] = v_u[diag].real + 0j
        ia_u = np.zeros(n + 1, dtype=np.int64)
        np.add.at(ia_u, r_u + 1, 1)
        ia_u = np.cumsum(ia_u)
        # full storage: U + U^H - diag, rows sorted by column
        off = ~diag
        r_f = np.concatenate([r_u, c_u[off]])
        c_f = np.concatenate([c_u, r_u[off]])
        v_f = np.concatenate([v_u, np.conj(v_u[off])])
        o = np.lexsort((c_f, r_f))
        r_f, c_f, v_f = r_f[o], c_f[o], v_f[o]
        ia_f = np.zeros(n + 1, dtype=np.int64)
        np.add.at(ia_f, r_f + 1, 1)
        ia_f = np.cumsum(ia_f)
        return dict(n=n, ia=ia_u, ja=c_u.astype(np.int64), val=v_u.astype(np.complex128), sym=True,
                    full=(ia_f, c_f.astype(np.int64), v_f.astype(np.complex128)))
    spec = PROFILES[name]
    lens = _lengths(spec, rng)
    n = spec.get("n", len(lens))
    assert len(lens) == n and lens.max(initial=0) <= n
    ia, ja = _columns(lens, n, rng)
    val = _values(kind, len(ja), rng).astype(np.complex128)
    return dict(n=n, ia=ia, ja=ja, val=val, sym=False, full=(ia, ja, val))


def _seed(name, kind, seed):
    h = 0
    for ch in "%s/%s/%d" % (name, kind, seed):
        h = (h * 131 + ord(ch)) % (2 ** 31)
    return h


def all_profile_cases():
    """(profile, value kind) pairs the GPU sweep runs."""
    out = [(p, k) for p, s in PROFILES.items() for k in s["kinds"]]
    out += [(p, k) for p, s in SYM_PROFILES.items() for k in s["kinds"]]
    return out


def probe_vector(n, seed):
    """0.5 <= |x_j| <= 1, random phase: no term of a row can vanish."""
    rng = np.random.default_rng(10_000 + seed)
    return (rng.uniform(0.5, 1.0, n) * np.exp(2j * np.pi * rng.random(n))).astype(np.complex128)


# ------------------------------------------------------------------------------------------------------------ geometry --
def n_distinct(val):
    """Distinct values as the device dictionary counts them: by bit pattern (0.5 + 0i and its conjugate 0.5 - 0i differ)."""
    a = np.ascontiguousarray(val, dtype=np.complex128).view(np.uint64).reshape(-1, 2)
    s = a[np.lexsort((a[:, 1], a[:, 0]))]
    return int(len(s) > 0) + int(np.count_nonzero(np.any(s[1:] != s[:-1], axis=1)))


def coding(kernel_opt, value_dict, val, nd=None):
    """(dict_mode, n_dict) of qbh_api.cpp try_value_dict (:651-667) + the code-width choice after it (create path, :587-592)."""
    if not value_dict or len(val) == 0:
        return 0, 0
    rows_family = kernel_opt not in (KERNEL_STREAM, KERNEL_VECTOR)        # A->kernel == QBH_KERNEL_ROWS (WAVE / AUTO included)
    cap = 65536 if (rows_family and value_dict != 2) else 256
    nd = n_distinct(val) if nd is None else nd
    if nd > cap:
        return 0, 0
    return (1 if nd <= 256 else 2 if nd <= K_DICT_LDS else 3), nd


def rows_geometry(kernel, ia, dict_mode, npb_opt):
    """Mirror of qbh_api.cpp setup_geometry (lines 230-269): npb, tpr, unroll, window, n_blocks.  None if npb is rejected."""
    nrows = len(ia) - 1
    nnz = int(ia[-1])
    lens = np.diff(ia)
    maxlen = int(lens.max()) if nrows > 0 else 0
    avg = nnz / nrows if nrows > 0 else 0.0
    coded = dict_mode != 0
    unroll = 4
    if kernel == KERNEL_ROWS:
        npb = 8192 if dict_mode == 1 else 4096 if dict_mode >= 2 else 2048
        cap_rows = 0.75 * K_ROW_CAP * (avg if avg > 1.0 else 1.0)
        while npb > 1024 and npb > cap_rows:
            npb >>= 1
        if npb_opt > 0:
            npb = npb_opt
        tpr = 1 if avg <= 64 else 2 if avg <= 128 else 4 if avg <= 256 else 8
        if not coded and avg > 12:
            tpr = 4 if avg <= 96 else 8
        unroll = 8 if tpr == 1 else 4
    else:
        npb = npb_opt if npb_opt > 0 else 2048
        if kernel == KERNEL_VECTOR:
            tpr = 2 if avg <= 24 else 4 if avg <= 96 else 8 if avg <= 192 else 16 if avg <= 512 else 32 if avg <= 2048 else 64
        else:
            tpr = 1 if avg <= 3 else 2 if avg <= 8 else 4 if avg <= 48 else 8 if avg <= 128 else 16
    if npb not in (1024, 2048, 4096) and not (npb == 8192 and kernel == KERNEL_ROWS and dict_mode == 1):
        return None
    window = npb - (maxlen - 1 if maxlen > 0 else 0) if maxlen <= npb // 2 else npb // 2
    n_blocks = max(1, -(-nnz // window))
    return dict(npb=npb, tpr=tpr, unroll=unroll, window=window, n_blocks=n_blocks)


def wave_geometry(ia):
    """Mirror of qbh_api.cpp setup_wave_geometry (lines 416-444): tpr, window, n_wb."""
    nrows = len(ia) - 1
    nnz = int(ia[-1])
    maxlen = int(np.diff(ia).max()) if nrows > 0 else 0
    window = 505 - (maxlen - 1 if maxlen > 0 else 0) if maxlen <= 256 else 249
    n_wb = max(1, -(-nnz // window))
    avg = nnz / nrows if nrows > 0 else 0.0
    tpr = 2 if avg <= 32 else 4 if avg <= 64 else 8 if avg <= 128 else 16
    return dict(tpr=tpr, window=window, n_wb=n_wb)


def block_starts(ia, window, n_blocks):
    """k_build_rowblocks / k_build_wavedesc: first row r with ia[r] >= w * window (r in [0, nrows]), sentinel nrows."""
    nrows = len(ia) - 1
    w = np.arange(n_blocks, dtype=np.int64)
    rb = np.searchsorted(ia[:nrows], w * window, side="left")
    return np.concatenate([rb, [nrows]]).astype(np.int64)


def walk_counts(n_units, grid, swz, chunk_mult=1):
    """Units (row blocks; groups of 4 wave blocks) each workgroup of a `grid` launch takes under BlockWalk (qbh_device.hpp)."""
    per_xcd = (n_units + 7) >> 3
    nslot = grid >> 3
    chunk = nslot * max(chunk_mult, 1)
    if swz == 2:
        per_xcd = -(-per_xcd // chunk) * chunk
    wg = np.arange(grid)
    xcd, slot = wg & 7, wg >> 3
    ntrip = np.maximum(0, -(-(per_xcd - slot) // nslot))
    counts = np.zeros(grid, dtype=np.int64)
    for t in range(int(ntrip.max(initial=0))):
        lb = slot + t * nslot
        ok = lb < per_xcd
        if swz == 1:
            b = xcd * per_xcd + lb
        elif swz == 2:
            b = ((lb // chunk) * 8 + xcd) * chunk + (lb % chunk)
        else:
            b = lb * 8 + xcd
        counts += (ok & (b < n_units)).astype(np.int64)
    return counts


def route(kernel_opt, value_dict, ia, val, npb_opt=0, xcd_swizzle=2, wave_walk=-1, deterministic=0, ncu=256, nd=None):
    """What an unsplit, unsharded-or-sharded CSR operator created with these options runs under qbh_spmv_dev (complex x, y):
    dict(kernel, info_kernel, dict_mode, n_dict, tpr, npb, unroll, n_blocks (info.n_blocks), walk, grid_max, key) or None when
    creation rejects the options.  key is the template instance: ("stream", NPB, TPR, DICT), ("vector", G, DICT),
    ("rows", NPB, P, DICT), ("wave", TPR, DYN).  Mirrors qbh_api.cpp:566-568 (kernel), 453 (use_wave), qbh_spmv.cpp local_part (walk)."""
    dict_mode, nd = coding(kernel_opt, value_dict, val, nd)
    k = KERNEL_VECTOR if kernel_opt == KERNEL_VECTOR else KERNEL_STREAM if kernel_opt == KERNEL_STREAM else KERNEL_ROWS
    g = rows_geometry(k, ia, dict_mode, npb_opt)
    if g is None:
        return None
    use_wave = k == KERNEL_ROWS and dict_mode == 0 and kernel_opt != KERNEL_ROWS
    r = dict(dict_mode=dict_mode, n_dict=nd, n_blocks=g["n_blocks"], npb=g["npb"], unroll=g["unroll"])
    if use_wave:
        w = wave_geometry(ia)
        swz = wave_walk if wave_walk >= 0 else xcd_swizzle
        if swz == 3 and deterministic:
            swz = 2
        units = (w["n_wb"] + 3) >> 2
        r.update(kernel="wave", info_kernel=KERNEL_WAVE, tpr=w["tpr"], walk=swz, n_wb=w["n_wb"], window=w["window"],
                 grid_max=max(8, min(MAX_WG_PER_CU * ncu, -(-units // 8) * 8) // 8 * 8),
                 key=("wave", w["tpr"], int(swz == 3)))
        return r
    name = KERNEL_NAMES[k]
    units = g["n_blocks"]
    if k == KERNEL_VECTOR:
        units = -(-(len(ia) - 1) // (K_BLOCK // g["tpr"]))
    r.update(kernel=name, info_kernel=k, tpr=g["tpr"], walk=xcd_swizzle, window=g["window"], units=units,
             grid_max=max(8, -(-min(units, GRID_CAP) // 8) * 8))
    if k == KERNEL_STREAM:
        r["key"] = ("stream", g["npb"], g["tpr"], int(dict_mode != 0))
    elif k == KERNEL_VECTOR:
        r["key"] = ("vector", g["tpr"], int(dict_mode != 0))
    else:
        r["key"] = ("rows", g["npb"], g["tpr"], dict_mode)
    return r


def all_routes():
    """Every template instance qbh_spmv_dev can launch on a complex CSR operator (qbh_spmv_csr.hip launch_spmv, qbh_spmv_wave.hip launch_spmv_wave)."""
    keys = set()
    for npb in (1024, 2048, 4096):
        for t in (1, 2, 4, 8, 16):
            for d in (0, 1):
                keys.add(("stream", npb, t, d))
    for t in (2, 4, 8, 16, 32, 64):
        for d in (0, 1):
            keys.add(("vector", t, d))
    for npb in (1024, 2048, 4096, 8192):
        for d in (0, 1, 2, 3):
            if npb == 8192 and d != 1:
                continue
            for t in ((1, 4, 8) if d == 0 else (1, 2, 4, 8)):
                keys.add(("rows", npb, t, d))
    for t in (2, 4, 8, 16):
        for dyn in (0, 1):
            keys.add(("wave", t, dyn))
    return keys


ALL_PATHS = {"stream_oversized", "stream_tile", "rows_groups", "rows_oversized", "rows_tile", "wave_rbase", "wave_rowpath",
             "wave_tile", "vector"}


def paths(r, ia):
    """Block paths the route reaches: stream_oversized (k_spmv_stream :315), rows_groups (rg > 0, :475), rows_oversized,
    wave_rbase (a pass with rbase > 0), wave_rowpath (block longer than the tile), and the ordinary tile paths."""
    out = set()
    if r["kernel"] == "vector":
        return {"vector"}
    if r["kernel"] == "wave":
        rb = block_starts(ia, r["window"], r["n_wb"])
        p0, p1 = ia[rb[:-1]], ia[rb[1:]]
        nr = rb[1:] - rb[:-1]
        nlong = p1 - (p0 - (p0 & 7))
        live = nr > 0
        if np.any(live & (nlong > WAVE_TILE)):
            out.add("wave_rowpath")
        if np.any(live & (nlong <= WAVE_TILE)):
            out.add("wave_tile")
        if np.any(live & (nlong <= WAVE_TILE) & (nr > 64 // r["tpr"])):
            out.add("wave_rbase")
        return out
    rb = block_starts(ia, r["window"], r["n_blocks"])
    nr = rb[1:] - rb[:-1]
    nlong = ia[rb[1:]] - ia[rb[:-1]]
    live = nr > 0
    if r["kernel"] == "stream":
        big = live & ((nlong > r["npb"]) | (nr > K_ROW_CAP))
        if np.any(big):
            out.add("stream_oversized")
        if np.any(live & ~big):
            out.add("stream_tile")
    else:
        if np.any(live & (nlong > r["npb"])):
            out.add("rows_oversized")
        if np.any(live & (nlong <= r["npb"])):
            out.add("rows_tile")
        if np.any(live & (nlong <= r["npb"]) & (nr > K_ROW_CAP)):
            out.add("rows_groups")
    return out


def min_walk(r, grid_max=None):
    """Lower bound, over every grid the launch can take (8 .. grid_max in steps of 8), on the blocks one persistent workgroup (wave:
    one wavefront) walks; for the dynamic walk the chunks of kDynChunk blocks in the smallest XCD region per wavefront that can
    draw from it.  Static walks only ever skip the padding, so the count is exact per grid."""
    gmax = r["grid_max"] if grid_max is None else grid_max
    if r["kernel"] == "wave":
        n_wb = r["n_wb"]
        if r["walk"] == 3:
            per = (n_wb + 7) >> 3
            last = n_wb - 7 * per
            chunks = -(-min(per, last) // K_DYN_CHUNK) if last > 0 else 0
            return chunks / (gmax // 8 * 4)
        units = (n_wb + 3) >> 2
        # a unit is 4 wave blocks, one per wavefront; only the last unit can be partly past the end
        return min(int(walk_counts(units, g, r["walk"]).min()) for g in range(8, gmax + 1, 8)) - 1
    return min(int(walk_counts(r["units"], g, r["walk"]).min()) for g in range(8, gmax + 1, 8))


# ----------------------------------------------------------------------------------------------------------- reference --
def row_sums(ia, ja, val, x, chunk=1 << 23):
    """(sum_j a_ij x_j, sum_j |a_ij| |x_j|) per row in long double, chunked so that ~1e8 nonzeros fit in host memory."""
    n = len(ia) - 1
    s = np.zeros(n, dtype=CL)
    a = np.zeros(n, dtype=L)
    ax = np.abs(x).astype(L)
    r0 = 0
    while r0 < n:
        r1 = int(np.searchsorted(ia, ia[r0] + chunk, side="right")) - 1
        r1 = min(max(r1, r0 + 1), n)
        p0, p1 = int(ia[r0]), int(ia[r1])
        if p1 > p0:
            c = ja[p0:p1]
            prod = val[p0:p1].astype(CL) * x[c].astype(CL)
            mag = np.abs(val[p0:p1]).astype(L) * ax[c]
            # segments of the nonempty rows only: each then runs exactly to the next nonempty row's start (or the chunk's end)
            ne = np.nonzero(ia[r0 + 1:r1 + 1] > ia[r0:r1])[0]
            idx = ia[r0 + ne] - p0
            s[r0 + ne] = np.add.reduceat(prod, idx)
            a[r0 + ne] = np.add.reduceat(mag, idx)
        r0 = r1
    return s, a


def epilogue(s, abs_s, nnz_row, xl, y0, alpha, beta, gamma, weights=None):
    """Reference y = alpha s + beta y0 + gamma xl, its reductions and their error bounds.

    Per row (u = eps / 2, gamma_k = k u / (1 - k u) <= 1.01 k u while k u <= 0.01):
      * each product a_ij x_j is formed componentwise, re = ar xr - ai xi (two products, one add; FMA only removes roundings),
        so each component carries <= gamma_2 (|ar xr| + |ai xi|) <= gamma_2 |a_ij| |x_j|  (Cauchy-Schwarz);
      * the m = nnz_i products are summed in SOME order (lane strides, shuffle trees, LDS): every term passes through at most m - 1
        additions, so each component of the row sum errs by <= gamma_{m+1} sum_j |a_ij| |x_j|;
      * alpha * sum + beta * y + gamma * x: one product and at most two additions more for each term: gamma_{m+4} on the alpha term,
        gamma_3 on the others.
    Each component of y_i then errs by <= gamma_{m+4} S_i with S_i = |alpha| sum_j |a_ij||x_j| + |beta||y_i| + |gamma||x_i|, the
    modulus by sqrt(2) times that, and sqrt(2) * 1.01 * (m + 4) u < (m + 4) eps, so

        |y_i - ref_i| <= e_i = c (nnz_i + k) eps S_i   with c = 1, k = 4.

    Reductions over the n rows (the kernels reduce the rows' own computed y, in any order):
      <x, y>: |dot - ref| <= sum_i |x_i| e_i + (n + 2) eps sum_i |x_i| (|ref_i| + e_i)   (products gamma_2, n - 1 additions, sqrt 2)
      |y|^2:  |nrm - ref| <= sum_i e_i (2 |ref_i| + e_i) + (n + 2) eps sum_i (|ref_i| + e_i)^2
    """
    al, be, ga = L(alpha), L(beta), L(gamma)
    xl_l = xl.astype(CL)
    y = al * s
    if beta != 0.0:
        y = y + be * y0.astype(CL)
    if gamma != 0.0:
        y = y + ga * xl_l
    scale = abs(al) * abs_s + abs(ga) * np.abs(xl).astype(L)
    if beta != 0.0:
        scale = scale + abs(be) * np.abs(y0).astype(L)
    e = (nnz_row.astype(L) + 4) * L(EPS) * scale
    # weights: how often each row occurs in the full vector (periodic operators reduce over one period)
    w = np.ones(len(s), dtype=L) if weights is None else weights.astype(L)
    n = float(w.sum())
    ax = np.abs(xl).astype(L)
    ay = np.abs(y)
    dot = np.sum(w * (np.conj(xl_l) * y))
    nrm = np.sum(w * (y.real * y.real + y.imag * y.imag))
    t_dot = np.sum(w * ax * e) + (L(n) + 2) * L(EPS) * np.sum(w * ax * (ay + e))
    t_nrm = np.sum(w * e * (2 * ay + e)) + (L(n) + 2) * L(EPS) * np.sum(w * (ay + e) ** 2)
    return dict(y=y, bound=e, dot=dot, nrm=nrm, t_dot=t_dot, t_nrm=t_nrm)


def exact_row_sums(ia, ja, val, x):
    """Fraction reference of sum_j a_ij x_j (real and imaginary parts) for small cases."""
    out = []
    for r in range(len(ia) - 1):
        re = im = Fraction(0)
        for p in range(int(ia[r]), int(ia[r + 1])):
            a, b = val[p], x[ja[p]]
            ar, ai, br, bi = (Fraction(float(a.real)), Fraction(float(a.imag)), Fraction(float(b.real)), Fraction(float(b.imag)))
            re += ar * br - ai * bi
            im += ar * bi + ai * br
        out.append((re, im))
    return out


def worst(got, ref):
    """(row, error / bound, number of rows over) of a computed y against epilogue() output."""
    err = np.abs(got.astype(CL) - ref["y"])
    bnd = np.maximum(ref["bound"], L(np.finfo(np.float64).tiny))
    ratio = err / bnd
    ratio = np.where(np.isfinite(ratio), ratio, L(np.inf))
    i = int(np.argmax(ratio)) if len(ratio) else 0
    return i, (float(ratio[i]) if len(ratio) else 0.0), int((ratio > 1).sum()), (float(err[i]) if len(err) else 0.0)


# ------------------------------------------------------------------------------------------------- formula operators --
# Large operators built on the device in chunks.  Columns and values are closed formulas of (row, entry, nonzero offset); all
# components are small integers, so every product and row sum is exact in float64 and the host reference is exact too.
def formula_cols(r, k, n, salt):
    """Distinct columns for entry k < L of row r (int64 arrays; works on numpy and torch): an odd stride per row keeps them distinct."""
    return (r * 7919 + salt + k * (2 * (r % 97) + 1013)) % n


def formula_vals(p):
    """Value of nonzero offset p: <= 251 distinct, never zero; depends on p mod 251 (2^31 and 2^32 are not multiples of 251)."""
    t = (p * 37) % 251
    return t % 15 + 1, t // 15 - 8           # (re, im)


def formula_x(j):
    """Probe vector entries: re in 1..8, im in +-1..+-4 (never zero)."""
    h = (j * 40503 + 17) % 65521
    im = h % 8 - 4
    return h // 8 % 8 + 1, im + (im >= 0)


def periodic_x(j):
    """Probe vector for the periodic operator: a function of j mod 7."""
    t = j % 7
    return t + 1, t - 3 + (t >= 3)


# ------------------------------------------------------------------------------------------------------------ the sweep --
def forms():
    """Options of every form the sweep creates per profile (make_opts keywords).  Duplicates of an already-run route are skipped."""
    out = [dict(spmv_kernel=KERNEL_WAVE, value_dict=0), dict(spmv_kernel=KERNEL_WAVE, value_dict=0, wave_walk=3),
           dict(spmv_kernel=KERNEL_WAVE, value_dict=0, wave_walk=0), dict(spmv_kernel=KERNEL_WAVE, value_dict=0, wave_walk=1),
           dict(spmv_kernel=KERNEL_WAVE, value_dict=0, xcd_swizzle=3, deterministic=1), dict(spmv_kernel=KERNEL_WAVE, value_dict=1)]
    for vd in (0, 1, 2):
        for npb in (0, 1024, 2048, 4096, 8192):
            out.append(dict(spmv_kernel=KERNEL_ROWS, value_dict=vd, nnz_per_block=npb))
    for vd in (0, 1):
        for npb in (0, 1024, 4096):
            out.append(dict(spmv_kernel=KERNEL_STREAM, value_dict=vd, nnz_per_block=npb))
        out.append(dict(spmv_kernel=KERNEL_VECTOR, value_dict=vd))
    for k in (KERNEL_ROWS, KERNEL_STREAM, KERNEL_VECTOR):
        for s in (0, 1, 3):
            out.append(dict(spmv_kernel=k, value_dict=0, xcd_swizzle=s))
    return out


def sweep(ia, val):
    """[(options, route)] of the forms() that creation accepts, one per distinct (route, walk, deterministic)."""
    nd = n_distinct(val) if len(val) else 0
    seen, out = set(), []
    for f in forms():
        r = route(f["spmv_kernel"], f["value_dict"], ia, val, npb_opt=f.get("nnz_per_block", 0), xcd_swizzle=f.get("xcd_swizzle", 2),
                  wave_walk=f.get("wave_walk", -1), deterministic=f.get("deterministic", 0), nd=nd)
        if r is None:
            continue
        sig = (r["key"], r["walk"], f.get("deterministic", 0))
        if sig in seen:
            continue
        seen.add(sig)
        out.append((f, r))
    return out
