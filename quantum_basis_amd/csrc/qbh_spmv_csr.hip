// qbh_spmv_csr.hip -- hand-written gfx950 (CDNA4) kernels of the CSR x vector hot path.
//
// Everything here is HBM-bound complex128 / int32 work: no MFMA.  What matters is
// (1) the val/col streams are read once, fully coalesced, non-temporal (so that the
// gathered x keeps the L2 / Infinity Cache), (2) many independent loads in flight per lane,
// (3) workgroup -> row-block mapping that lets each XCD's private L2 see a contiguous range
// of rows (x-gather locality), (4) BLAS-1 work fused into the SpMV epilogue so vectors are
// not re-read.
//
// Replaces mkl_sparse_z_mv (src/sparse.cc:287) and the cblas_z* level-1 calls of the
// Lanczos / CG loops (src/lanczos.cc:195-214, 296-337).
//
// This file: the workgroup-granular CSR kernels.  The wave-granular kernels are in qbh_spmv_wave.hip, the level-1 kernels in
// qbh_blas1.hip, the device helpers all of them share in qbh_device.hpp.
#include "qbh_internal.hpp"
#include "qbh_device.hpp"
#include "qbh_dict.hpp"

namespace qbh {

// ------------------------------------------------- streaming SpMV (default) ----
// One workgroup per row block of <= NPB nonzeros.  Phase 1: all 256 lanes stream the
// block's col/val ranges (perfectly coalesced, NPB/256 independent 4 B + 16 B + gathered
// 16 B loads in flight per lane) and park val*x products in LDS.  Phase 2: TPR lanes per
// row sum the row's LDS segment, shuffle-reduce, run the fused epilogue.
// The block descriptors (first row rb[], first nonzero bp[]) of the NEXT block are fetched
// while the current one is processed, and the epilogue operands (old y, local x) are
// requested before the stream loads, so a block's critical path is col -> x -> LDS only.
template <int NPB, int TPR, bool DICT>
__global__ __launch_bounds__(kBlock) void k_spmv_stream(SpmvArgs a)
{
    spmv_args_resolve(a);
    __shared__ d2 prod[NPB];
    __shared__ int rowoff[kRowCap + 1];
    __shared__ double red[12];
    __shared__ d2 dict_s[DICT ? 256 : 1];

    constexpr int U = NPB / kBlock;          // independent load chains per lane
    constexpr int G = kBlock / TPR;          // rows reduced per pass
    const int tid = threadIdx.x;
    const int g = tid / TPR, sub = tid % TPR;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool need_y = a.beta != 0.0;
    const bool need_x = a.gamma != 0.0 || a.partials != nullptr;

    if (DICT) {
        dict_s[tid] = a.dict[tid];
        __syncthreads();
    }

    BlockWalk walk(a.n_blocks, a.swizzle);
    int64_t lb = walk.slot;
    int64_t b = walk.block(lb);
    bool live = lb < walk.per_xcd && b < a.n_blocks;
    int r0 = 0, r1 = 0;
    int64_t p0 = 0, p1 = 0;
    if (live) {
        r0 = a.rb[b]; r1 = a.rb[b + 1];
        p0 = a.bp[b]; p1 = a.bp[b + 1];
    }
    while (lb < walk.per_xcd) {
        // descriptors of the next block this workgroup will take (uniform -> scalar loads)
        const int64_t lb_n = lb + walk.nslot;
        const int64_t b_n = walk.block(lb_n);
        const bool live_n = lb_n < walk.per_xcd && b_n < a.n_blocks;
        int r0_n = 0, r1_n = 0;
        int64_t p0_n = 0, p1_n = 0;
        if (live_n) {
            r0_n = a.rb[b_n]; r1_n = a.rb[b_n + 1];
            p0_n = a.bp[b_n]; p1_n = a.bp[b_n + 1];
        }
        const int nr = r1 - r0;
        const int64_t nlong = p1 - p0;
        if (live && nr > 0) {
            if (nlong <= NPB && nr <= kRowCap) {
                const int n = (int)nlong;
                // row offsets and epilogue operands: requested first, consumed last
                const int ro = (int)(a.ia[r0 + (tid <= nr ? tid : 0)] - p0);
                d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
                const bool mine = sub == 0 && g < nr;
                if (mine && need_y) yo = load_y_old(a, r0 + g);
                if (mine && need_x) xi = load_x_local(a, r0 + g);
                if (n > 0) {
                    // All U loads of each stream are issued back to back with a clamped index
                    // (no per-element branch): U col + U val + U gathered-x loads in flight
                    // per lane -- the memory-level parallelism a branchy loop does not have.
                    const int32_t *jp = a.ja + p0;
                    const int nm1 = n - 1;
                    int c[U];
                    d2 v[U], xv[U];
                    uint8_t cb[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int i = tid + u * kBlock;
                        c[u] = ntload(jp + (i < n ? i : nm1)) & a.colmask;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int i = tid + u * kBlock;
                        const int ii = i < n ? i : nm1;
                        if (DICT) cb[u] = ntload(a.code + p0 + ii);
                        else      v[u] = ntload(a.val + p0 + ii);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) xv[u] = a.xg[c[u]];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int i = tid + u * kBlock;
                        if (DICT) v[u] = dict_s[cb[u]];
                        if (i < n) prod[i] = cmul(v[u], xv[u]);
                    }
                }
                if (tid <= nr) rowoff[tid] = ro;
                for (int i = tid + kBlock; i <= nr; i += kBlock) rowoff[i] = (int)(a.ia[r0 + i] - p0);
                __syncthreads();
                for (int r = g; r < nr; r += G) {
                    const int e = rowoff[r + 1];
                    d2 sum = {0.0, 0.0};
                    for (int q = rowoff[r] + sub; q < e; q += TPR) sum += prod[q];
#pragma unroll
                    for (int off = TPR / 2; off > 0; off >>= 1) {
                        sum.x += __shfl_xor(sum.x, off, 64);
                        sum.y += __shfl_xor(sum.y, off, 64);
                    }
                    if (sub == 0) {
                        if (r == g) row_epilogue2(a, (int64_t)r0 + r, sum, yo, xi, acc);
                        else        row_epilogue(a, (int64_t)r0 + r, sum, acc);
                    }
                }
                __syncthreads();
            } else {
                // oversized block (a row longer than the LDS tile, or > kRowCap very short
                // rows): row by row, whole workgroup per row.  Correctness path, not tuned.
                for (int r = 0; r < nr; ++r) {
                    const int64_t s = a.ia[r0 + r], e = a.ia[r0 + r + 1];
                    double part[2] = {0.0, 0.0};
                    for (int64_t q = s + tid; q < e; q += kBlock) {
                        d2 v;
                        if (DICT) v = dict_s[a.code[q]];
                        else      v = a.val[q];
                        const d2 t = cmul(v, a.xg[a.ja[q] & a.colmask]);
                        part[0] += t.x;
                        part[1] += t.y;
                    }
                    block_sum<2>(part, red);
                    if (tid == 0) {
                        d2 sum = {part[0], part[1]};
                        row_epilogue(a, (int64_t)r0 + r, sum, acc);
                    }
                    __syncthreads();
                }
            }
        }
        lb = lb_n; b = b_n; live = live_n;
        r0 = r0_n; r1 = r1_n; p0 = p0_n; p1 = p1_n;
    }
    if (a.partials != nullptr) {
        block_sum<3>(acc, red);
        if (tid == 0) {
            a.partials[(size_t)blockIdx.x * 3 + 0] = acc[0];
            a.partials[(size_t)blockIdx.x * 3 + 1] = acc[1];
            a.partials[(size_t)blockIdx.x * 3 + 2] = acc[2];
        }
    }
}

// ------------------------------------------------ row-aligned SpMV -------------
// Same row blocks as k_spmv_stream, different use of LDS.  Phase 1 stages only the block's
// (col, value-or-code) ranges into LDS with coalesced non-temporal loads.  Phase 2 maps LANES
// TO ROWS: sub-slice s of P handles steps k = s, s+P, ... of each of R = 256/P consecutive
// rows, so at every step the lanes of a wavefront gather the k-th entries of consecutive rows.
// For Kronecker-structured Hamiltonians (H = T_up (x) 1 + 1 (x) T_dn + D) the leading and the
// trailing entries of consecutive rows point at CONSECUTIVE x elements, so stepping alternately
// from the front and from the back of the row turns those gathers into full-line coalesced
// loads.  Row sums stay in registers (no 16-byte products through LDS, no shuffle tree);
// with the value dictionary the LDS footprint is 5 B/nnz and 8 workgroups fit a CU.
// DICT: 0 complex128 values | 1 one-byte codes, dictionary (<= 256) in LDS | 2 two-byte codes, dictionary
// (<= kDictLds) in LDS | 3 two-byte codes, dictionary (<= 65536) read through the caches
template <int NPB, int P, int UN, int DICT, bool REALX>
__global__ __launch_bounds__(kBlock) void k_spmv_rows(SpmvArgs a)
{
    spmv_args_resolve(a);
    constexpr int R = kBlock / P;            // rows per pass
    constexpr int U = NPB / kBlock;          // staged cols per lane
    constexpr int CPW = DICT >= 2 ? 4 : 8;   // codes per 8-byte word
    constexpr int UC = (NPB / CPW + kBlock - 1) / kBlock;   // 8-byte code words per lane
    __shared__ int scol[NPB];
    __shared__ d2 sval[DICT ? 1 : NPB];
    __shared__ unsigned long long scode8[DICT ? NPB / CPW : 1];
    __shared__ d2 dict_s[DICT == 1 ? 256 : DICT == 2 ? kDictLds : 1];
    __shared__ int rowoff[kRowCap + 1];
    __shared__ d2 part[P > 1 ? kBlock : 1];
    __shared__ double red[12];

    const int tid = threadIdx.x;
    const int sub = tid / R, rloc = tid % R;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool need_y = a.beta != 0.0;
    const bool need_x = a.gamma != 0.0 || a.partials != nullptr;
    const uint8_t *scode = reinterpret_cast<const uint8_t *>(scode8);
    const uint16_t *scode16 = reinterpret_cast<const uint16_t *>(scode8);
    const uint16_t *gcode16 = reinterpret_cast<const uint16_t *>(a.code);
    auto coded_value = [&](int i) -> d2 {          // value of staged element i
        if (DICT == 1) return dict_s[scode[i]];
        if (DICT == 2) return dict_s[scode16[i]];
        return a.dict[scode16[i]];
    };

    if (DICT == 1) {
        dict_s[tid] = a.dict[tid];
        __syncthreads();
    }
    if (DICT == 2) {
        for (int i = tid; i < kDictLds; i += kBlock) dict_s[i] = a.dict[i];
        __syncthreads();
    }

    BlockWalk walk(a.n_blocks, a.swizzle, a.chunk_mult);
    int64_t lb = walk.slot;
    int64_t b = walk.block(lb);
    bool live = lb < walk.per_xcd && b < a.n_blocks;
    int r0 = 0, r1 = 0;
    int64_t p0 = 0, p1 = 0;
    if (live) {
        r0 = a.rb[b]; r1 = a.rb[b + 1];
        p0 = a.bp[b]; p1 = a.bp[b + 1];
    }
    while (lb < walk.per_xcd) {
        const int64_t lb_n = lb + walk.nslot;
        const int64_t b_n = walk.block(lb_n);
        const bool live_n = lb_n < walk.per_xcd && b_n < a.n_blocks;
        int r0_n = 0, r1_n = 0;
        int64_t p0_n = 0, p1_n = 0;
        if (live_n) {
            r0_n = a.rb[b_n]; r1_n = a.rb[b_n + 1];
            p0_n = a.bp[b_n]; p1_n = a.bp[b_n + 1];
        }
        const int nr = r1 - r0;
        const int64_t nlong = p1 - p0;
        if (live && nr > 0) {
            if (nlong <= NPB) {
                const int n = (int)nlong;
                // ---- phase 1: stage the block's index / value streams ----
                // (a block of very short rows can hold more than kRowCap of them: their offsets are staged and their sums
                // formed kRowCap rows at a time, nrg = rows of the current group)
                const int nrg0 = nr < kRowCap ? nr : kRowCap;
                const int ro = (int)(a.ia[r0 + (tid <= nrg0 ? tid : 0)] - p0);
                d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
                const bool mine = sub == 0 && rloc < nr;
                if (mine && need_y) yo = load_y_old(a, r0 + rloc);
                if (mine && need_x) xi = load_x_local(a, r0 + rloc);
                if (n > 0) {
                    const int32_t *jp = a.ja + p0;
                    const int nm1 = n - 1;
                    int c[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int i = tid + u * kBlock;
                        c[u] = ntload(jp + (i < n ? i : nm1)) & a.colmask;
                    }
                    if (DICT) {
                        unsigned long long w[UC];
                        const int nw = (n + CPW - 1) / CPW;          // 8-byte words covering the codes
#pragma unroll
                        for (int u = 0; u < UC; ++u) {
                            const int i = tid + u * kBlock;
                            // unaligned 8-byte global load; the last word may read up to 7 bytes past the
                            // block's range but never past the code array (padded by 16 bytes at build)
                            w[u] = ntload(reinterpret_cast<const unsigned long long *>(a.code + p0 * (8 / CPW)) + (i < nw ? i : 0));
                        }
#pragma unroll
                        for (int u = 0; u < UC; ++u) {
                            const int i = tid + u * kBlock;
                            if (i < NPB / CPW) scode8[i] = w[u];
                        }
                    } else {
                        d2 v[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int i = tid + u * kBlock;
                            v[u] = ntload(a.val + p0 + (i < n ? i : nm1));
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) sval[tid + u * kBlock] = v[u];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) scol[tid + u * kBlock] = c[u];
                }
                if (tid <= nrg0) rowoff[tid] = ro;
                for (int i = tid + kBlock; i <= nrg0; i += kBlock) rowoff[i] = (int)(a.ia[r0 + i] - p0);
                __syncthreads();
                for (int rg = 0; rg < nr; rg += kRowCap) {
                const int nrg = nr - rg < kRowCap ? nr - rg : kRowCap;
                if (rg > 0) {                                          // next group of rows of the same staged block
                    __syncthreads();
                    for (int i = tid; i <= nrg; i += kBlock) rowoff[i] = (int)(a.ia[r0 + rg + i] - p0);
                    __syncthreads();
                }
                // ---- phase 2: lanes <-> rows ----
                for (int rbase = 0; rbase < nrg; rbase += R) {
                    const int row = rbase + rloc;
                    const bool rowok = row < nrg;
                    const int base = rowok ? rowoff[row] : 0;
                    const int len = rowok ? rowoff[row + 1] - base : 0;
                    int wmax = len;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        const int o = __shfl_xor(wmax, off, 64);
                        wmax = o > wmax ? o : wmax;
                    }
                    d2 sum = {0.0, 0.0};
                    for (int k0 = sub; k0 < wmax; k0 += UN * P) {
                        int cc[UN];
                        int ix[UN];
                        bool ok[UN];
#pragma unroll
                        for (int j = 0; j < UN; ++j) {
                            const int k = k0 + j * P;
                            ok[j] = k < len;
                            const int f = (k & 1) ? len - 1 - (k >> 1) : (k >> 1);   // front / back alternation
                            ix[j] = base + (ok[j] ? f : 0);
                            cc[j] = scol[ix[j]];
                        }
                        if (REALX) {
                            // real operator applied to a real vector: gather 8-byte real parts from the packed
                            // copy of x; (a+0i)(b+0i) = ab+0i exactly, so the result is bit-identical
                            double xr[UN], vr[UN];
#pragma unroll
                            for (int j = 0; j < UN; ++j) xr[j] = a.xr[cc[j]];
#pragma unroll
                            for (int j = 0; j < UN; ++j) {
                                if (DICT) vr[j] = coded_value(ix[j]).x;
                                else      vr[j] = sval[ix[j]].x;
                            }
#pragma unroll
                            for (int j = 0; j < UN; ++j)
                                if (ok[j]) sum.x += vr[j] * xr[j];
                        } else {
                            d2 xv[UN], vv[UN];
#pragma unroll
                            for (int j = 0; j < UN; ++j) xv[j] = a.xg[cc[j]];
#pragma unroll
                            for (int j = 0; j < UN; ++j) {
                                if (DICT) vv[j] = coded_value(ix[j]);
                                else      vv[j] = sval[ix[j]];
                            }
#pragma unroll
                            for (int j = 0; j < UN; ++j)
                                if (ok[j]) sum += cmul(vv[j], xv[j]);
                        }
                    }
                    if (P > 1) {
                        part[tid] = sum;
                        __syncthreads();
                        if (sub == 0) {
#pragma unroll
                            for (int s2 = 1; s2 < P; ++s2) sum += part[s2 * R + rloc];
                        }
                    }
                    if (sub == 0 && rowok) {
                        if (rbase == 0 && rg == 0) row_epilogue2(a, (int64_t)r0 + row, sum, yo, xi, acc);
                        else                       row_epilogue(a, (int64_t)r0 + rg + row, sum, acc);
                    }
                    if (P > 1 && rbase + R < nrg) __syncthreads();     // part[] is reused by the next pass
                }
                }
                if (P == 1) __syncthreads();                           // scol is rewritten by the next block
            } else {
                for (int r = 0; r < nr; ++r) {
                    const int64_t s = a.ia[r0 + r], e = a.ia[r0 + r + 1];
                    double pr[2] = {0.0, 0.0};
                    for (int64_t q = s + tid; q < e; q += kBlock) {
                        d2 v;
                        if (DICT == 1)      v = dict_s[a.code[q]];
                        else if (DICT == 2) v = dict_s[gcode16[q]];
                        else if (DICT == 3) v = a.dict[gcode16[q]];
                        else                v = a.val[q];
                        const int cq = a.ja[q] & a.colmask;
                        const d2 xq = REALX ? d2{a.xr[cq], 0.0} : a.xg[cq];
                        const d2 t = cmul(v, xq);
                        pr[0] += t.x;
                        pr[1] += t.y;
                    }
                    block_sum<2>(pr, red);
                    if (tid == 0) {
                        d2 sum = {pr[0], pr[1]};
                        row_epilogue(a, (int64_t)r0 + r, sum, acc);
                    }
                    __syncthreads();
                }
            }
        }
        lb = lb_n; b = b_n; live = live_n;
        r0 = r0_n; r1 = r1_n; p0 = p0_n; p1 = p1_n;
    }
    if (a.partials != nullptr) {
        block_sum<3>(acc, red);
        if (tid == 0) {
            a.partials[(size_t)blockIdx.x * 3 + 0] = acc[0];
            a.partials[(size_t)blockIdx.x * 3 + 1] = acc[1];
            a.partials[(size_t)blockIdx.x * 3 + 2] = acc[2];
        }
    }
}

// ------------------------------------------- sub-wavefront-per-row SpMV --------
// G lanes per row, NO LDS staging and no workgroup barrier: a wavefront owns 64/G consecutive rows and every lane walks
// its row in strides of G, UN entries at a time -- UN column loads, UN value loads and then UN x gathers in flight per
// lane.  Nothing limits occupancy but registers (the row kernel's 20 B/nnz of LDS hold it at 3 workgroups per CU), so
// the chain row pointer -> (column, value) -> x -> FMA of one wavefront hides behind up to 8 wavefronts per SIMD.
// The matrix stream is read straight from global memory: the G lanes of a row take G consecutive entries (64 B of
// values at G = 4), consecutive steps touch the same 128-byte lines again while they are still in L1, so HBM sees each
// line once.  Entries are taken alternately from the front and the back of the row, as in k_spmv_rows: for the
// Kronecker-structured Hamiltonians the k-th entries of consecutive rows then point at consecutive x elements.
template <int G, int UN, bool DICT>
__global__ __launch_bounds__(kBlock) void k_spmv_vector(SpmvArgs a)
{
    spmv_args_resolve(a);
    __shared__ double red[12];
    __shared__ d2 dict_s[DICT ? 256 : 1];
    const int tid = threadIdx.x;
    constexpr int RPB = kBlock / G;            // rows per workgroup pass
    const int g = tid / G, sub = tid % G;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool need_y = a.beta != 0.0;
    const bool need_x = a.gamma != 0.0 || a.partials != nullptr;
    if (DICT) {
        dict_s[tid] = a.dict[tid];
        __syncthreads();
    }
    const int64_t n_chunks = (a.nrows + RPB - 1) / RPB;
    const int64_t last = a.ia[a.nrows] - 1;    // clamp for the masked lanes (nnz > 0)
    BlockWalk walk(n_chunks, a.swizzle, a.chunk_mult);
    for (int64_t lb = walk.slot; lb < walk.per_xcd; lb += walk.nslot) {
        const int64_t b = walk.block(lb);
        if (b >= n_chunks) continue;
        const int64_t row = b * RPB + g;
        const bool rowok = row < a.nrows;
        const int64_t s = rowok ? a.ia[row] : 0;
        const int len = rowok ? (int)(a.ia[row + 1] - s) : 0;
        d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
        const bool mine = sub == 0 && rowok;
        if (mine && need_y) yo = load_y_old(a, row);
        if (mine && need_x) xi = load_x_local(a, row);
        int wmax = len;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(wmax, off, 64);
            wmax = o > wmax ? o : wmax;
        }
        d2 sum = {0.0, 0.0};
        for (int k0 = sub; k0 < wmax; k0 += G * UN) {
            int c[UN];
            bool ok[UN];
            int64_t q[UN];
            d2 v[UN], xv[UN];
            uint8_t cb[UN];
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                const int k = k0 + j * G;
                ok[j] = k < len;
                const int f = (k & 1) ? len - 1 - (k >> 1) : (k >> 1);     // front / back alternation
                q[j] = ok[j] ? s + f : last;
                c[j] = ntload(a.ja + q[j]) & a.colmask;
            }
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                if (DICT) cb[j] = ntload(a.code + q[j]);
                else      v[j] = ntload(a.val + q[j]);
            }
#pragma unroll
            for (int j = 0; j < UN; ++j) xv[j] = a.xg[c[j]];
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                if (DICT) v[j] = dict_s[cb[j]];
                if (ok[j]) sum += cmul(v[j], xv[j]);
            }
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            sum.x += __shfl_xor(sum.x, off, 64);
            sum.y += __shfl_xor(sum.y, off, 64);
        }
        if (mine) row_epilogue2(a, row, sum, yo, xi, acc);
    }
    if (a.partials != nullptr) {
        block_sum<3>(acc, red);
        if (tid == 0) {
            a.partials[(size_t)blockIdx.x * 3 + 0] = acc[0];
            a.partials[(size_t)blockIdx.x * 3 + 1] = acc[1];
            a.partials[(size_t)blockIdx.x * 3 + 2] = acc[2];
        }
    }
}

// ---- instance tables ----
// One function per kernel family maps the run-time parameters to the address of the instance, nullptr where there is none.
// The launcher and the occupancy query of a family read the same table, so an instance is listed once.
template <int G, bool DICT>
static SpmvKernel vector_kernel_un(int un)
{
    return un == 8 ? k_spmv_vector<G, 8, DICT> : un == 2 ? k_spmv_vector<G, 2, DICT> : k_spmv_vector<G, 4, DICT>;
}

static SpmvKernel vector_kernel(int tpr, int un, bool dict)
{
    switch (tpr) {
    case 2:  return dict ? vector_kernel_un<2, true>(un)  : vector_kernel_un<2, false>(un);
    case 4:  return dict ? vector_kernel_un<4, true>(un)  : vector_kernel_un<4, false>(un);
    case 8:  return dict ? vector_kernel_un<8, true>(un)  : vector_kernel_un<8, false>(un);
    case 16: return dict ? vector_kernel_un<16, true>(un) : vector_kernel_un<16, false>(un);
    case 32: return dict ? vector_kernel_un<32, true>(un) : vector_kernel_un<32, false>(un);
    case 64: return dict ? vector_kernel_un<64, true>(un) : vector_kernel_un<64, false>(un);
    default: return nullptr;
    }
}

template <int NPB, bool DICT>
static SpmvKernel stream_kernel_tpr(int tpr)
{
    switch (tpr) {
    case 1:  return k_spmv_stream<NPB, 1, DICT>;
    case 2:  return k_spmv_stream<NPB, 2, DICT>;
    case 4:  return k_spmv_stream<NPB, 4, DICT>;
    case 8:  return k_spmv_stream<NPB, 8, DICT>;
    case 16: return k_spmv_stream<NPB, 16, DICT>;
    default: return nullptr;
    }
}

static SpmvKernel stream_kernel(int npb, int tpr, bool dict)
{
    switch (npb) {
    case 1024: return dict ? stream_kernel_tpr<1024, true>(tpr) : stream_kernel_tpr<1024, false>(tpr);
    case 2048: return dict ? stream_kernel_tpr<2048, true>(tpr) : stream_kernel_tpr<2048, false>(tpr);
    case 4096: return dict ? stream_kernel_tpr<4096, true>(tpr) : stream_kernel_tpr<4096, false>(tpr);
    default: return nullptr;
    }
}

template <int NPB, int PP, int DICT>
static SpmvKernel rows_kernel_un(int un, bool realx)
{
    if (un == 8) return realx ? k_spmv_rows<NPB, PP, 8, DICT, true> : k_spmv_rows<NPB, PP, 8, DICT, false>;
    return realx ? k_spmv_rows<NPB, PP, 4, DICT, true> : k_spmv_rows<NPB, PP, 4, DICT, false>;
}

template <int NPB, int DICT>
static SpmvKernel rows_kernel_p(int tpr, int un, bool realx)
{
    switch (tpr) {
    case 1: return rows_kernel_un<NPB, 1, DICT>(un, realx);
    case 2: return rows_kernel_un<NPB, 2, DICT>(un, realx);
    case 4: return rows_kernel_un<NPB, 4, DICT>(un, realx);
    case 8: return rows_kernel_un<NPB, 8, DICT>(un, realx);
    default: return nullptr;
    }
}

template <int DICT>
static SpmvKernel rows_kernel_npb(int npb, int tpr, int un, bool realx)
{
    switch (npb) {
    case 1024: return rows_kernel_p<1024, DICT>(tpr, un, realx);
    case 2048: return rows_kernel_p<2048, DICT>(tpr, un, realx);
    case 4096: return rows_kernel_p<4096, DICT>(tpr, un, realx);
    case 8192:
        if constexpr (DICT == 1) return rows_kernel_p<8192, DICT>(tpr, un, realx);
        return nullptr;
    default: return nullptr;
    }
}

// dict_mode as k_spmv_rows' DICT
static SpmvKernel rows_kernel(int dict_mode, int npb, int tpr, int un, bool realx)
{
    switch (dict_mode) {
    case 0: return rows_kernel_npb<0>(npb, tpr, un, realx);
    case 1: return rows_kernel_npb<1>(npb, tpr, un, realx);
    case 2: return rows_kernel_npb<2>(npb, tpr, un, realx);
    default: return rows_kernel_npb<3>(npb, tpr, un, realx);
    }
}

// The occupancy queries take an unroll other than 8 (vector kernel: 8 or 2) as 4, as the launch does, and the row kernel's asks
// about the complex-gather form (REALX = false) whatever the launch will gather: kept as found.  A failed query returns 0 and
// leaves the runtime's error state as it is.
static int kernel_occupancy(SpmvKernel k)
{
    int n = 0;
    if (k == nullptr) return 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, kBlock, 0) == hipSuccess ? n : 0;
}

// workgroups of the lanes-per-row kernel resident per CU (0 if unknown)
int vector_kernel_occupancy(int tpr, int un, bool dict)
{
    return kernel_occupancy(vector_kernel(tpr, un, dict));
}

// workgroups of the row kernel that are resident per CU (0 if unknown); dict_mode as k_spmv_rows' DICT
int rows_kernel_occupancy(int npb, int tpr, int un, int dict_mode)
{
    return kernel_occupancy(rows_kernel(dict_mode, npb, tpr, un, false));
}

int spmv_grid(int kernel, int64_t n_blocks, int64_t nrows, int tpr)
{
    // 256 CUs; the streaming kernel fits 4 workgroups per CU (LDS), the vector kernel 8.
    int64_t units = n_blocks;
    int64_t cap = 256 * 4 * 4;
    if (kernel == QBH_KERNEL_ROWS) cap = 256 * 8 * 2;
    if (kernel == QBH_KERNEL_VECTOR) {
        const int rpb = kBlock / tpr;
        units = (nrows + rpb - 1) / rpb;
        cap = 256 * 8 * 2;
    }
    int64_t g = units < cap ? units : cap;
    g = ((g + 7) / 8) * 8;
    if (g < 8) g = 8;
    return (int)g;
}

int launch_spmv(const SpmvArgs &a_in, int kernel, int npb, int tpr, int grid, hipStream_t s)
{
    SpmvArgs a = a_in;
    if (a.yin == nullptr) a.yin = a.y;           // the beta term reads y itself unless a driver names another vector
    SpmvKernel k;
    // an unsupported combination: the table says which parameter has no instance (1 lane per row exists for every block size)
    if (kernel == QBH_KERNEL_ROWS) {
        const int dict_mode = a.code == nullptr ? 0 : a.dict_mode;
        k = rows_kernel(dict_mode, npb, tpr, a.unroll, a.xr != nullptr);
        if (k == nullptr) {
            if (rows_kernel(dict_mode, npb, 1, a.unroll, false) != nullptr) set_error("k_spmv_rows: unsupported lanes-per-row %d (1, 2, 4, 8)", tpr);
            else if (npb == 8192) set_error("nnz_per_block 8192 needs the one-byte value dictionary");
            else set_error("k_spmv_rows: unsupported nnz_per_block %d", npb);
            return QBH_EINVAL;
        }
    } else if (a.code != nullptr && a.dict_mode != 1) {
        set_error("two-byte value codes need the row kernel");
        return QBH_EUNSUPP;
    } else if (kernel == QBH_KERNEL_VECTOR) {
        k = vector_kernel(tpr, a.unroll, a.code != nullptr);
        if (k == nullptr) {
            set_error("unsupported lanes-per-row %d", tpr);
            return QBH_EINVAL;
        }
    } else {
        k = stream_kernel(npb, tpr, a.code != nullptr);
        if (k == nullptr) {
            if (stream_kernel(npb, 1, false) != nullptr) set_error("unsupported threads-per-row %d", tpr);
            else set_error("unsupported nnz_per_block %d (1024, 2048 or 4096)", npb);
            return QBH_EINVAL;
        }
    }
    return launch_kernel(k, grid, kBlock, s, a);
}

}  // namespace qbh
