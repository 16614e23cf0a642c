// qbh_spmv_wave.hip -- the wave-granular SpMV kernels (k_spmv_wave, k_spmv_wave2), their block descriptors, the
// ordered reduction of the chunk partials, launchers and occupancy.
#include "qbh_internal.hpp"
#include "qbh_device.hpp"

namespace qbh {

// ------------------------------------------------ wave-granular SpMV (uncoded) ---
// One WAVEFRONT per block of whole rows holding <= 512 nonzeros; no workgroup barrier anywhere.  Lane l takes the
// entries l, l+64, ... of the block: 8 column + 8 value loads (coalesced, non-temporal), then the 8 gathers, all in
// flight together; the products go to a wave-private 8 KB LDS tile and TPR lanes per row sum them, shuffle-reduce
// and run the fused epilogue.  Against the workgroup-granular kernels above this keeps 16 independent load / gather
// / reduce pipelines per CU instead of 3 lock-stepped ones, which is what the cache-friendly operators were limited
// by (DESIGN-history 5.0 item 4): chain L = 26 goes from 1.06 to 0.72 ms.  Descriptors (first row / first nonzero of the
// block and of the next one) are fetched one block ahead.
// Complex128 values, complex vectors only: the coded / real-gather formats stay on k_spmv_rows.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int TPR, bool DYN>
__global__ __launch_bounds__(kBlock) void k_spmv_wave(SpmvArgs a)
{
    spmv_args_resolve(a);
    constexpr int U = 8, NW = 64 * U, RP = 64 / TPR;
    __shared__ d2 prod_s[4 * NW];
    __shared__ double red[12];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    d2 *prod = prod_s + wv * NW;
    const int sub = lane % TPR, rloc = lane / TPR;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool need_y = a.beta != 0.0;
    const bool need_x = a.gamma != 0.0 || a.partials != nullptr;

    // unit = 4 consecutive wave blocks (one per wavefront of the workgroup), walked XCD-aware like the row blocks
    BlockWalk walk((a.n_wb + 3) >> 2, a.swizzle, a.chunk_mult);
    // The descriptor pair (this block, next block) is read one trip ahead as ONE 32-byte vector load -- lane j holds
    // dword j -- and broadcast with readlane when the trip starts: the compiler tracks it like any other load (an
    // explicit s_load would be faster still, but nothing stops the register allocator from copying its destination
    // SGPRs while the load is in flight).  A block past the end reads the sentinel pair (n_wb, n_wb + 1): zero rows.
    constexpr bool dyn = DYN;            // compile-time: the atomic of the dynamic walk must not leak into the static kernel's waits
    DynWalk dw;
    if constexpr (dyn) dw.init(a.n_wb, a.wctr, lane);
    auto load_desc = [&](int64_t lb) -> int {
        int64_t w = a.n_wb;
        if (dyn) {
            w = dw.block(lb);
        } else if (lb < walk.per_xcd) {
            w = walk.block(lb) * 4 + wv;
            if (w > a.n_wb) w = a.n_wb;
        }
        return reinterpret_cast<const int *>(a.wd + w)[lane & 7];
    };
    const int64_t step = dyn ? 1 : walk.nslot;
    int64_t lb = dyn ? 0 : walk.slot;
    int dq = load_desc(lb);
    while (dyn ? dw.live(lb) : (lb < walk.per_xcd)) {
        const uint32_t q0 = (uint32_t)__builtin_amdgcn_readlane(dq, 0), q1 = (uint32_t)__builtin_amdgcn_readlane(dq, 1);
        const uint32_t q4 = (uint32_t)__builtin_amdgcn_readlane(dq, 4), q5 = (uint32_t)__builtin_amdgcn_readlane(dq, 5);
        const int r0 = __builtin_amdgcn_readlane(dq, 2), nr = __builtin_amdgcn_readlane(dq, 6) - r0;
        const int64_t p0 = (int64_t)(((uint64_t)q1 << 32) | q0);
        const int64_t p1 = (int64_t)(((uint64_t)q5 << 32) | q4);
        if constexpr (dyn) {
            if (dw.asks(lb)) dw.nxt = dw.take(dw.ask(lane));
        }
        lb += step;
        if constexpr (dyn) dw.advance(lb);
        dq = load_desc(lb);                                                 // next block's descriptors, used one trip later
        if (nr <= 0) continue;
        // the stream is read from the 128-byte boundary below the block's first value (8 entries): every 1 KB value load then
        // covers exactly 8 lines instead of 9, the tile holds sh + n <= 512 entries (the builder leaves the room)
        const int sh = (int)(p0 & 7);
        const int64_t base = p0 - sh;
        const int64_t nlong = p1 - base;
        if (nlong <= NW) {
            const int n = (int)nlong;
            // first pass row offsets + epilogue operands: requested before the streams, consumed last
            int s0 = 0, e0 = 0;
            d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
            if (rloc < nr) {
                s0 = (int)(a.ia[r0 + rloc] - base);
                e0 = (int)(a.ia[r0 + rloc + 1] - base);
                if (sub == 0) {
                    if (need_y) yo = a.yin[r0 + rloc];
                    if (need_x) xi = a.xl[r0 + rloc];
                }
            }
            if (n > 0) {
                const int nm1 = n - 1;
                int c[U];
                d2 v[U], xv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = lane + u * 64;
                    c[u] = ntload(a.ja + base + (i < n ? i : nm1)) & a.colmask;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = lane + u * 64;
                    v[u] = ntload(a.val + base + (i < n ? i : nm1));
                }
#pragma unroll
                for (int u = 0; u < U; ++u) xv[u] = a.xg[c[u]];
#pragma unroll
                for (int u = 0; u < U; ++u) prod[lane + u * 64] = cmul(v[u], xv[u]);
            }
            wave_lds_fence();
            for (int rbase = 0; rbase < nr; rbase += RP) {
                const int row = rbase + rloc;
                int s = s0, e = e0;
                if (rbase > 0) {
                    s = e = 0;
                    if (row < nr) {
                        s = (int)(a.ia[r0 + row] - base);
                        e = (int)(a.ia[r0 + row + 1] - base);
                    }
                }
                d2 sum = {0.0, 0.0};
                for (int k = s + sub; k < e; k += TPR) sum += prod[k];
#pragma unroll
                for (int off = TPR / 2; off > 0; off >>= 1) {
                    sum.x += __shfl_xor(sum.x, off, 64);
                    sum.y += __shfl_xor(sum.y, off, 64);
                }
                if (sub == 0 && row < nr) {
                    if (rbase == 0) row_epilogue2(a, (int64_t)r0 + row, sum, yo, xi, acc);
                    else            row_epilogue(a, (int64_t)r0 + row, sum, acc);
                }
            }
            wave_lds_fence();                      // the tile is rewritten by the next block
        } else {
            // a row longer than the wave tile: the wavefront walks the block's rows one at a time (correctness path)
            for (int r = 0; r < nr; ++r) {
                const int64_t s = a.ia[r0 + r], e = a.ia[r0 + r + 1];
                d2 sum = {0.0, 0.0};
                for (int64_t k = s + lane; k < e; k += 64) sum += cmul(a.val[k], a.xg[a.ja[k] & a.colmask]);
                sum.x = wave_sum(sum.x);
                sum.y = wave_sum(sum.y);
                if (lane == 0) row_epilogue(a, (int64_t)r0 + r, sum, acc);
            }
        }
    }
    if (a.partials != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c * 4 + wv] = acc[c];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                a.partials[(size_t)blockIdx.x * 3 + c] = (red[c * 4 + 0] + red[c * 4 + 1]) + (red[c * 4 + 2] + red[c * 4 + 3]);
        }
    }
}

// instance table of k_spmv_wave: every tpr other than 2, 4 and 8 takes the 16 form.  The launcher and the occupancy query both
// read it, so an instance is listed once.
template <bool DYN>
static SpmvKernel wave_kernel_tpr(int tpr)
{
    switch (tpr) {
    case 2:  return k_spmv_wave<2, DYN>;
    case 4:  return k_spmv_wave<4, DYN>;
    case 8:  return k_spmv_wave<8, DYN>;
    default: return k_spmv_wave<16, DYN>;
    }
}

static SpmvKernel wave_kernel(int tpr, bool dyn)
{
    return dyn ? wave_kernel_tpr<true>(tpr) : wave_kernel_tpr<false>(tpr);
}

// workgroups of kernel k resident per CU; a failed query returns 0 and does not stay behind as the runtime's last error
static int kernel_occupancy(SpmvKernel k)
{
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, kBlock, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return occ;
}

int launch_spmv_wave(const SpmvArgs &a_in, int tpr, int grid, hipStream_t s)
{
    SpmvArgs a = a_in;
    if (a.yin == nullptr) a.yin = a.y;           // the beta term reads y itself unless a driver names another vector
    return launch_kernel(wave_kernel(tpr, a.swizzle == 3), grid, kBlock, s, a);
}

// asks about the static walk (DYN = false) whatever walk the launch will use: kept as found
int wave_kernel_occupancy(int tpr)
{
    return kernel_occupancy(wave_kernel(tpr, false));
}

// wave block w = the rows whose first nonzero lies in [w*window, (w+1)*window); entry n_wb and n_wb + 1 = sentinels
__global__ void k_build_wavedesc(const int64_t *ia, int64_t nrows, int64_t window, WaveDesc *wd, int64_t n_wb)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > n_wb + 1) return;
    WaveDesc d;
    d.pad = 0;
    if (w >= n_wb) {
        d.p0 = ia[nrows];
        d.r0 = (int32_t)nrows;
    } else {
        const int64_t target = w * window;
        int64_t lo = 0, hi = nrows;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ia[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        d.p0 = ia[lo];
        d.r0 = (int32_t)lo;
    }
    wd[w] = d;
}

int launch_build_wavedesc(const int64_t *d_ia, int64_t nrows, int64_t window, WaveDesc *d_wd, int64_t n_wb, hipStream_t s)
{
    const int64_t n = n_wb + 2;
    return launch_kernel(k_build_wavedesc, (unsigned)((n + 255) / 256), 256, s, d_ia, nrows, window, d_wd, n_wb);
}


// ------------------------------------ pipelined wave kernel (Kronecker split) ----
// The same decomposition as k_spmv_wave, software-pipelined per wavefront for the two passes of a split operator, whose
// gathers hit the L2: the gathers of block i are issued, THEN the 16 stream loads of block i+1, and only the gathers are
// waited for (vector-memory results return in order, so the order of issue is what keeps a block's stream in flight
// while the previous block is reduced).  Every load of the steady state is unconditional (clamped addresses): the
// compiler's s_waitcnt counts are then exact.  Descriptors are fetched two blocks ahead.
// OPS 0: plain store of the row sums (far pass; y is the far buffer, rows are far rows)
// OPS 3: the same for the far part stored SLICED: inside every group of 8 consecutive far rows the entries are interleaved
//        (entry k of rows 8g..8g+7 contiguous, the group padded to its longest row -- no padding where the 8 rows are the
//        8 minor indices of one major index), so the coalesced stream ALREADY has consecutive lanes on consecutive rows with
//        the same entry number: every gather instruction reads full 128-byte lines of the tiled x.  ia holds the group
//        pointers, the descriptor's row fields count groups.
// OPS 2: fused epilogue, the far result of the row added first (read at the row's tiled index)
// wavefronts per SIMD of the near pass: 2 = 204 VGPRs, no spill; 3 = 168 VGPRs with 17 spilled (measured: see DESIGN-history 4.1c)
#ifndef QBH_NEAR_WAVES
#define QBH_NEAR_WAVES 2
#endif
#ifndef QBH_FAR_WAVES
#define QBH_FAR_WAVES 3
#endif
#ifdef QBH_NT_ROW_STORE
#define QBH_ROW_STORE(p, v) __builtin_nontemporal_store((v), (p))
#else
#define QBH_ROW_STORE(p, v) (*(p) = (v))
#endif
// C16: the part's columns are 2 bytes each (a.ja16), relative to a base named by the block's descriptor (SpmvArgs::ja16): 8 lines
// of column stream per block instead of 16 -- the passes are bound by line requests, not bytes (DESIGN-history 5.0b)
// G8 (sliced far pass with 2-byte columns only): the 8 slots of every line of the stream name the same major index (T (x) 1, verified
// at conversion) and a.ja8 holds that value once per line -- ONE column load per lane and block (1 line of the 512-slot block's ~140
// instead of 8), and one register instead of eight carried across the pipeline stage; the per-slot values are formed by cross-lane
// moves where the gathers are issued.  Gather addresses, and everything behind them, are those of the per-slot stream.
// V8 (only with G8): the 8 values of every line are the same bits as well (verified at conversion) and a.val8 holds that value once per
// line -- the eight value loads of a block stay, but the 8 lanes of a line share one address: each load is ONE 128-byte line instead
// of eight (8 lines of the block's stream instead of 64).  Every lane holds the value of its own slot as before, so nothing behind
// the loads changes: the operands of every product are those of the per-slot stream.  (The other form -- one load per lane and
// block, the slot's value taken from the line's lane by cross-lane moves: 96 VGPRs instead of 154 -- measured 0.28 ms slower on the
// headline's far pass, profiles/far_vals8_time.txt; LDS, not registers, caps this pass's occupancy.)
// NL (the one-class near passes only): a.len8 holds the rows' lengths, one byte each.  ONE clamped 1-byte load per lane and block, issued
// with the block's stream (lane l: row l of the block), replaces the two 8-byte row-pointer loads -- a block's ~28 rows are a
// quarter of a line instead of 2-3 lines -- and one register instead of two is carried across the pipeline stage.  The rows' offsets
// are the exclusive prefix sums from the descriptor's lead on, formed across the lanes when the block is reduced; every pass of the
// row loop takes its row's (offset, length) from the owning lane, so a block with more rows than one pass takes (6 % of the
// headline's) loads no pointers behind the next block's stream.  A block with more than 64 rows takes a further round of 64 lengths
// inside the loop.  The epilogue operands of the later passes are still loaded there, as before.
// VP (the one-class near passes, only beside C16; with NL or without): the off-diagonal values of a near row are the same bits in every major index
// (1 (x) T' + D, verified at creation) and a.valp holds those of the first major index, a.kK entries that stay cached: the eight value
// loads of a block read the pattern at (entry - major index of the block's first row * kK), wrapped once where the block reaches into
// the next major index (or its lead into the one before) -- plain loads, not non-temporal ones: the lines are meant to stay.  The one
// entry per row that differs, the diagonal, enters the row sum at its own slot: its position inside the row comes with the row's
// length (a.dpos8; NL: bits 24-31 of the packed word, else loaded beside the row's pointers), its value (a.diag) with the row's other epilogue operands, and the product the
// row loop takes there is cmul({diag, +0.0}, x[row]) -- x[row] is what the slot gathered (2-byte columns: xg == xl).  The operands of every
// product and the order of every sum are those of the per-entry stream.  (The other form -- a sentinel in the pattern and a
// predicated load of diag[column] beside the gathers -- was not needed: this one keeps 2 wavefronts per SIMD without a spill.)
template <int TPR, int OPS, bool DYN, bool C16 = false, bool G8 = false, bool NL = false, bool V8 = false, bool VP = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((OPS == 0 || OPS == 3) ? QBH_FAR_WAVES : QBH_NEAR_WAVES, (OPS == 0 || OPS == 3) ? QBH_FAR_WAVES : QBH_NEAR_WAVES))) void k_spmv_wave2(SpmvArgs a)
{
    spmv_args_resolve(a);
    static_assert(!C16 || OPS == 1 || OPS == 2 || OPS == 3, "2-byte columns: the one-class near passes and the sliced far pass");
    static_assert(!G8 || (C16 && OPS == 3), "grouped columns: the sliced far pass with 2-byte columns");
    static_assert(!NL || OPS == 1 || OPS == 2, "row lengths: the one-class near passes");
    static_assert(!V8 || G8, "grouped values: only beside the grouped columns");
    static_assert(!VP || (C16 && (OPS == 1 || OPS == 2)), "shared value pattern: the one-class near passes with 2-byte columns");
    constexpr int NW = 512, RP = 64 / TPR;
    constexpr bool EPI = OPS == 1 || OPS == 2 || OPS == 4, FAR = OPS == 2 || OPS == 4;      // OPS 1: the fused epilogue WITHOUT a far addend
    // The fused reductions under the ordered dynamic walk: which wavefront takes which chunk depends on the run, so per-wavefront
    // partial sums would make <x, y> and |y|^2 differ in the last bits from run to run.  Every CHUNK (kDynChunk consecutive blocks,
    // always taken whole by one wavefront, rows in order) has a slot of its own instead: its three sums are stored when the
    // wavefront moves on and k_reduce_chunks adds the slots in a fixed order -- bit-reproducible a_j / b_j at the dynamic walk's speed.
    constexpr bool CHUNKRED = DYN && (OPS == 1 || OPS == 2 || OPS == 4);
    constexpr bool MULTI = OPS == 4;             // OPS 4 = OPS 2 for an operator with several classes (KronMap): the far result of a row sits at its
                                                 // compact far row id, looked up through the class table a.kcls; the block's descriptor names its class
    __shared__ d2 prod_s[4 * NW];
    __shared__ double red[12];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    d2 *prod = prod_s + wv * NW;
    const int sub = lane % TPR, rloc = lane / TPR;
    double acc[3] = {0.0, 0.0, 0.0};
    const bool need_y = a.beta != 0.0;

    BlockWalk walk((a.n_wb + 3) >> 2, a.swizzle, a.chunk_mult);
    constexpr bool dyn = DYN;
    DynWalk dw;
    auto load_desc = [&](int64_t lb) -> int {
        int64_t w = a.n_wb;
        if (dyn) {
            w = dw.block(lb);
        } else if (lb < walk.per_xcd) {
            w = walk.block(lb) * 4 + wv;
            if (w > a.n_wb) w = a.n_wb;
        }
        return reinterpret_cast<const int *>(a.wd + w)[lane & 7];
    };
    const int64_t step = dyn ? 1 : walk.nslot;
    struct Blk {
        int64_t p0;              // the 128-byte boundary below the block's first value (the stream is read from there: 8 lines per
                                 // 1 KB value load instead of 9); row offsets are taken relative to it
        int r0, nr, n;           // n = entries from p0 to the block's end; -1: a row longer than the tile (row-at-a-time path)
        bool cont0, cont1;       // OPS 3: the first group began in the block before / the last group goes on in the block after
        int cls;                 // OPS 4: class of the block's first row
        int64_t xb;              // C16: element of the gather source that column value 0 of this block names
        int lead;                // entries between p0 and the block's first entry (they belong to the block before: loaded, never used)
        int ve;                  // VP: entry of the value pattern that p0 names (negative: a lead that begins in the major index before)
    };
    // far result of one row (OPS 2 / 4)
    // (rows and minor sizes are below 2^31 -- int32 columns -- so the index arithmetic of a row's far slot is 32-bit: a 64-bit
    // division by a run-time divisor is ~100 instructions on the critical path of every block's epilogue operands)
    const uint32_t kS32 = (uint32_t)a.kS, kB32 = (uint32_t)a.kB;
    const int kLB = 31 - __builtin_clz(kB32 | 1u);                   // band widths are powers of two
    auto far_at = [&](int64_t row, int c0) -> d2 {
        if constexpr (MULTI) {
            int c = c0;
            while (row >= a.kcls[c + 1].rbase) ++c;                 // a block rarely straddles two classes
            const KronCls k = a.kcls[c];
            const uint32_t local = (uint32_t)(row - k.rbase), S32 = (uint32_t)k.S, u = local / S32, d = local - u * S32;
            if (d >= ((S32 >> 3) << 3)) return d2{0.0, 0.0};         // a row of the class's narrow last band: no far part
            return a.far[k.fbase + (int64_t)(d >> 3) * 8 * k.NU + (int64_t)u * 8 + (d & 7)];
        } else {
            const uint32_t r = (uint32_t)row, u = r / kS32, d = r - u * kS32;
            const uint32_t b = d >> kLB, j = d & (kB32 - 1u), rem = kS32 - (b << kLB), wB = rem < kB32 ? rem : kB32;
            return a.far[(int64_t)b * (a.kNU << kLB) + (int64_t)u * wB + j];
        }
    };
    // OPS 3: a block is 512 consecutive SLOTS of the sliced stream whatever the groups are (descriptor: first slot, first
    // group that overlaps, pad = 1 when that group began in the previous block); a group cut by a block boundary gets its
    // row sums from both blocks by atomic add into rows zeroed before the pass (two addends: the result does not depend
    // on their order), every other row a plain store
    auto decode = [&](int dq) -> Blk {
        const uint32_t q0 = (uint32_t)__builtin_amdgcn_readlane(dq, 0), q1 = (uint32_t)__builtin_amdgcn_readlane(dq, 1);
        const uint32_t q4 = (uint32_t)__builtin_amdgcn_readlane(dq, 4), q5 = (uint32_t)__builtin_amdgcn_readlane(dq, 5);
        Blk b;
        const int64_t pfirst = (int64_t)(((uint64_t)q1 << 32) | q0);
        // OPS 3: blocks are exact runs of slots, cut so that they start on 128-byte boundaries of the arrays (k_build_slotdesc's shift)
        b.p0 = OPS == 3 ? pfirst : pfirst - (pfirst & 7);
        b.lead = OPS == 3 ? 0 : (int)(pfirst & 7);
        const int64_t p1 = (int64_t)(((uint64_t)q5 << 32) | q4);
        b.r0 = __builtin_amdgcn_readlane(dq, 2);
        b.nr = __builtin_amdgcn_readlane(dq, 6) - b.r0;
        b.cls = MULTI ? __builtin_amdgcn_readlane(dq, 3) : 0;
        b.xb = 0;
        b.ve = 0;
        if constexpr (C16) {
            const int64_t pad = (uint32_t)__builtin_amdgcn_readlane(dq, 3);
            b.xb = OPS == 3 ? (pad >> 1) * 8 * a.kNU : pad * a.kS;
            if constexpr (VP) {
                // a sentinel descriptor names major index 0 beside the END of the part: whatever is not an entry of the block's own
                // major index (or a lead in front of it) reads the pattern from its start
                const int64_t ve = b.p0 - pad * a.kK;
                b.ve = (ve >= -8 && ve < a.kK) ? (int)ve : 0;
            }
        }
        b.cont0 = OPS == 3 && (__builtin_amdgcn_readlane(dq, 3) & 1);
        b.cont1 = OPS == 3 && (__builtin_amdgcn_readlane(dq, 7) & 1);
        if (b.cont1) b.nr += 1;
        b.n = (p1 - b.p0) <= NW ? (int)(p1 - b.p0) : -1;
        return b;
    };
    struct Ops {
        int s, e;                // OPS 3: s = the group pointer of group `lane` of the block, relative to the block's first slot
        d2 yo, xi, fr;
        int dp;                  // VP: position of the diagonal entry inside row `lane` of the block
        double dg;               // VP: the row's diagonal value (real: its imaginary part is +0.0, checked at creation)
    };
    // OPS 3: a block overlaps at most 64 groups (a group holds 8 slots or more), so ONE load per lane, issued with the block's
    // stream, brings every group pointer the block needs; the reduction passes read them by cross-lane moves.  (A load
    // issued later would have to be waited for with the whole next stream in front of it: results return in order.)
    auto group_range = [&](const Blk &b, int gp, int row, int &s_, int &e_, bool &clip) {     // row = 8 * group + j inside the block
        const int gi = row >> 3;
        const int gs = __shfl(gp, gi & 63, 64);
        int ge = __shfl(gp, (gi + 1) & 63, 64);
        if (gi + 1 >= 64) ge = b.n;
        clip = gs < 0 || ge > b.n;
        s_ = (gs < 0 ? 0 : gs) + (row & 7);
        e_ = ge > b.n ? b.n : ge;
    };
    // stream + first-pass operands of a block; an empty / oversized block reads entry 0 of its range (clamped)
    auto issue = [&](const Blk &b, int (&c)[8], d2 (&v)[8], Ops &o) {
        const int nn = b.n > 0 ? b.n : 1;
        const int nm1 = nn - 1;
        // p0 of the sentinel is nnz: clamp the base so that even an empty block loads inside the arrays
        const int64_t base = b.n > 0 ? b.p0 : 0;
        if constexpr (G8) {
            // line l of the block = slots 8 l .. 8 l + 7 (blocks start at multiples of 512 slots and hold a multiple of 8); lane l keeps
            // line l's value, a line past the block's end reads the last one (what the clamped per-slot loads name there)
            const int lm = nm1 >> 3;
            c[0] = ntload(a.ja8 + (base >> 3) + (lane < lm ? lane : lm));
#pragma unroll
            for (int u = 1; u < 8; ++u) c[u] = 0;
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = lane + u * 64;
                if constexpr (C16) c[u] = ntload(a.ja16 + base + (i < nn ? i : nm1));
                else               c[u] = ntload(a.ja + base + (i < nn ? i : nm1)) & a.colmask;
            }
        }
        // The up to 7 entries in front of the block's first one are the tail of the block BEFORE: their 2-byte columns are relative
        // to THAT block's base, and decoded with this block's they can point up to two major indices ahead -- past the end of x
        // for the last blocks of an operator or shard (found by the 4-rank C3 rehearsal, round 5: a memory access fault on the ranks
        // whose vectors ended at an allocation boundary).  Their products are never used: gather element 0 of the block's base.
        if constexpr (C16 && OPS != 3) {
            if (b.n > 0 && lane < b.lead) c[0] = 0;
        }
        if constexpr (V8) {
            // slot lane + 64 u sits in line lane / 8 + 8 u: the 8 lanes of a line read the line's value themselves (one 128-byte line
            // per load); a line past the block's end reads the last one, which is what the clamped per-slot loads name there
            const int lm = nm1 >> 3;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int l = (lane >> 3) + 8 * u;
                v[u] = ntload(a.val8 + (base >> 3) + (l < lm ? l : lm));
            }
        } else if constexpr (VP) {
            // slot i of the block is entry ve + i of the pattern: past the end of the major index of the block's first row it is the
            // next one's (- kK), a lead in front of its start the one before's (+ kK); kK >= 1024 > 7 + 512, so once is enough
            const int kk = (int)a.kK, e0 = b.n > 0 ? b.ve : 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = lane + u * 64;
                int e = e0 + (i < nn ? i : nm1);
                e = e >= kk ? e - kk : e;
                e = e < 0 ? e + kk : e;
                v[u] = a.valp[e];
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = lane + u * 64;
                v[u] = ntload(a.val + base + (i < nn ? i : nm1));
            }
        }
        if (OPS == 3) {
            const int64_t ng = (a.nrows + 7) >> 3;
            int64_t g = (int64_t)b.r0 + lane;
            g = g < ng ? g : ng;
            int64_t rel = a.ia[g] - base;
            rel = rel < -4096 ? -4096 : rel > 4096 ? 4096 : rel;
            o.s = (int)rel;
            o.e = 0;
        } else if constexpr (NL) {
            // the length of row `lane` of the block, as loaded (the lanes at or beyond b.nr re-read the last row's and are masked where
            // the prefix sums are formed: nothing here waits for the load)
            const int last = b.nr > 0 ? b.nr - 1 : 0;
            o.s = a.len8[(int64_t)b.r0 + (lane < last ? lane : last)];
            o.e = 0;
            if constexpr (VP) o.dp = a.dpos8[(int64_t)b.r0 + (lane < last ? lane : last)];
        } else {
            const bool mine = rloc < b.nr;
            const int64_t row = mine ? (int64_t)b.r0 + rloc : 0;
            o.s = (int)(a.ia[row] - base);
            o.e = (int)(a.ia[row + 1] - base);
            if (!mine) o.s = o.e = 0;
            if constexpr (VP) o.dp = a.dpos8[row];
        }
    };
    // epilogue operands of the CURRENT block's first pass: issued after its gathers and before the next block's stream (they
    // are not carried across a block as a second register set; the wait for the gathers still leaves them in flight)
    auto issue_ops = [&](const Blk &b, Ops &o) {
        if (EPI) {
            int64_t row = rloc < b.nr ? (int64_t)b.r0 + rloc : 0;
            if (MULTI && rloc >= b.nr) row = b.r0 < a.nrows ? b.r0 : a.nrows - 1;      // idle lanes: a row of the block's own class (the class search starts there)
            o.yo = a.yin[row];
            o.xi = a.xl[row];
            o.fr = FAR ? far_at(row, b.cls) : d2{0.0, 0.0};
            if constexpr (VP) o.dg = a.diag[row];
            if (!need_y) o.yo = d2{0.0, 0.0};
        }
    };
    // Finished rows of the ordered walk are not stored row by row: a wavefront's consecutive blocks hold consecutive rows, so
    // the results wait in a wave-private LDS buffer and leave as full 1 KB stores when the run of rows ends (chunk change) or
    // the buffer is full.  (tools/lab/region_probe: one 512-byte store per 8 KB block costs a stream 17 %, the same bytes in
    // 1 KB stores every fourth block 4 %.)  OPS 3: a group cut between two blocks of the SAME run is summed in the buffer;
    // only the groups cut at the ends of a run are added atomically.
#ifndef QBH_BUF_MODE
#define QBH_BUF_MODE 1                           // 0 never | 1 the sliced far pass | 2 every pass of the ordered walk
#endif
    constexpr bool BUF = DYN && (QBH_BUF_MODE == 2 || (QBH_BUF_MODE == 1 && OPS == 3));
    constexpr int CAP = 256;
    __shared__ d2 rbuf_s[BUF ? 4 * CAP : 1];
    d2 *rbuf = rbuf_s + (BUF ? wv * CAP : 0);
    int64_t buf_r0 = 0;
    int buf_n = 0, buf_nb = 0;                   // rows buffered; rows buffered before the current block
    bool at_first = false, at_last = false, merge_first = false, direct = !BUF;
    auto emit = [&](int64_t row, d2 v, bool atomic) {
        if (OPS == 3) {
            if (row < a.nrows) {
                if (atomic) {
                    double *yp = reinterpret_cast<double *>(a.y + row);
                    unsafeAtomicAdd(yp, v.x);
                    unsafeAtomicAdd(yp + 1, v.y);
                } else {
                    QBH_ROW_STORE(a.y + row, v);
                }
            }
        } else {
            QBH_ROW_STORE(a.y + row, v);
        }
    };
    auto flush = [&]() {
        if (BUF && buf_n > 0) {
            wave_lds_fence();
            for (int i = lane; i < buf_n; i += 64) emit(buf_r0 + i, rbuf[i], OPS == 3 && ((i < 8 && at_first) || (i >= buf_n - 8 && at_last)));
            wave_lds_fence();
            buf_n = 0;
        }
    };
    // before the rows of a block: first row, row count, "first group continues the buffered one"
    auto open_block = [&](int64_t first, int nrows_blk, bool c0, bool fits) {
        if (BUF) {
            if (buf_n > 0 && (!fits || first != buf_r0 + buf_n - (c0 ? 8 : 0) || first + nrows_blk - buf_r0 > CAP)) flush();
            direct = !fits || nrows_blk > CAP;
            if (!direct) {
                if (buf_n == 0) {
                    buf_r0 = first;
                    at_first = c0;
                    merge_first = false;
                } else {
                    merge_first = c0;
                }
                buf_nb = buf_n;
            }
        }
    };
    auto close_block = [&](int64_t first, int nrows_blk, bool c1) {
        if (BUF && !direct) {
            buf_n = (int)(first + nrows_blk - buf_r0);
            at_last = c1;
        }
    };
    auto finish_row = [&](int64_t row, d2 sum, d2 yo, d2 xi, d2 fr, bool clip) {
        d2 v = sum;
        if (EPI) {
            if (FAR) sum += fr;
            v = a.alpha * sum + a.beta * yo + a.gamma * xi;
            acc[0] += xi.x * v.x + xi.y * v.y;
            acc[1] += xi.x * v.y - xi.y * v.x;
            acc[2] += v.x * v.x + v.y * v.y;
        }
        if (BUF && !direct) {
            const int idx = (int)(row - buf_r0);
            if (OPS == 3 && merge_first && idx < buf_nb) v += rbuf[idx];
            rbuf[idx] = v;
        } else {
            emit(row, v, clip);
        }
    };

    // Ordered dynamic walk: the XCDs do not run at the same speed (measured with QBH_XCD_TIMING on C3: three of the eight finish
    // their eighth of the near pass 1.5-1.9 ms before the pass ends, one its eighth of the far pass 1.3 ms early), so a wavefront
    // whose own XCD's region is exhausted joins the queue of the next XCD's region, and so on round the ring.  The hop is OUTSIDE
    // the pipelined loop (a pipeline drain and refill per hop, at most 7 per wavefront): the loop itself has no new branch.
    constexpr int NHOP =
#ifdef QBH_NO_XCD_STEAL
        1;
#else
        dyn ? 8 : 1;
#endif
#ifdef QBH_WAVE_TIMING
    unsigned long long tm[4] = {0, 0, 0, 0}, nblk = 0;
#endif
    int64_t red_slot = -1;                       // CHUNKRED: slot of the chunk whose rows acc[] is collecting
    auto red_flush = [&]() {
        if constexpr (CHUNKRED) {
            if (red_slot >= 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
                if (lane == 0) {
                    double *slot = a.chunk_red + red_slot * 3;
                    slot[0] = acc[0];
                    slot[1] = acc[1];
                    slot[2] = acc[2];
                }
                acc[0] = acc[1] = acc[2] = 0.0;
            }
        }
    };
    for (int hop = 0; hop < NHOP; ++hop) {
    if constexpr (dyn) dw.init(a.n_wb, a.wctr, lane, (int)((blockIdx.x + hop) & 7));
    int64_t lb = dyn ? 0 : walk.slot;
    int dq0 = load_desc(lb), dq1 = load_desc(lb + step);
    Blk b0 = decode(dq0), b1 = decode(dq1);
    int cA[8];
    d2 vA[8];
    Ops oA;
    issue(b0, cA, vA, oA);
#ifdef QBH_WAVE_TIMING
#define QBH_TICK(i, t_from) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tm[i] += t_ - (t_from); t_from = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
    unsigned long long t_mark = __builtin_amdgcn_s_memtime();
#else
#define QBH_TICK(i, t_from) do { } while (0)
#endif
    while (dyn ? dw.live(lb) : (lb < walk.per_xcd)) {
        const int dq2 = load_desc(lb + 2 * step);
        unsigned int reply = 0;
        bool asking = false;
        if constexpr (dyn) {
            asking = dw.asks(lb);
            if (asking) {
                if constexpr (CHUNKRED) {            // first turn of a chunk: the sums of the chunk before go to its slot
                    red_flush();
                    red_slot = dw.chunk_slot();
                }
                reply = dw.ask(lane);                // in front of the gathers: answered by the time they are
            }
        }
        d2 xv[8];
        if constexpr (C16) {
            // sliced far part: slot i of a block belongs to far row 8 g + i % 8 (groups and blocks start at multiples of 8 slots)
            const d2 *xq = a.xg + b0.xb + (OPS == 3 ? (lane & 7) : 0);
            if constexpr (G8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) xv[u] = xq[__shfl(cA[0], (lane >> 3) + 8 * u, 64) << 3];      // slot lane + 64 u sits in line lane / 8 + 8 u
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) xv[u] = xq[OPS == 3 ? (cA[u] << 3) : cA[u]];
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) xv[u] = a.xg[cA[u]];
        }
        issue_ops(b0, oA);
        __builtin_amdgcn_sched_barrier(0);      // the gathers go out BEFORE the next block's stream (in-order return)
        int cB[8];
        d2 vB[8];
        Ops oB;
        issue(b1, cB, vB, oB);
        __builtin_amdgcn_sched_barrier(0);
        QBH_TICK(0, t_mark);                   // top of the turn .. gathers and next stream issued (waits for this block's columns)
        if (b0.n >= 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) prod[lane + u * 64] = cmul(vA[u], xv[u]);
            wave_lds_fence();
            QBH_TICK(1, t_mark);               // .. gathers arrived, products in LDS
            constexpr int RSTRIDE = OPS == 3 ? 8 : 1;                  // distance of a row's consecutive entries in the tile
            const int nrows_blk = OPS == 3 ? 8 * b0.nr : b0.nr;
            const int64_t first_row = OPS == 3 ? (int64_t)b0.r0 * 8 : (int64_t)b0.r0;
            open_block(first_row, nrows_blk, b0.cont0, true);
            // NL: lane l keeps (offset from p0 | length << 16) of row l of the current round of 64 rows; the offsets are the exclusive
            // prefix sums of the lengths from the end of the round before on (first round: the descriptor's lead).  An offset is at
            // most the tile's 512, a length at most 255.  VP: the position of the row's diagonal entry rides in bits 24-31.
            int pk = 0, round_end = b0.lead;
            auto lens_round = [&](int len_raw, int dp_raw, int rb) {
                const int len = rb + lane < b0.nr ? len_raw : 0;
                // inclusive prefix sum over the wavefront by data-parallel moves (no LDS traffic): shifts inside the rows of 16 lanes,
                // then lane 15 of a row into the next row, lane 31 into the upper half; a lane without a source adds 0
                int inc = len;
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, false);       // row_shr:1
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, false);       // row_shr:2
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, false);       // row_shr:4
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xf, 0xf, false);       // row_shr:8
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xa, 0xf, false);       // row_bcast:15 into rows 1 and 3
                inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xc, 0xf, false);       // row_bcast:31 into rows 2 and 3
                pk = (round_end + inc - len) | (len << 16);
                if constexpr (VP) pk |= dp_raw << 24;
                round_end += __builtin_amdgcn_readlane(inc, 63);
            };
            if constexpr (NL) lens_round(oA.s, VP ? oA.dp : 0, 0);
            for (int rbase = 0; rbase < nrows_blk; rbase += RP) {
                const int row = rbase + rloc;
                int s_ = oA.s, e_ = oA.e;
                bool clip = false;
                d2 yo = oA.yo, xi = oA.xi, fr = oA.fr;
                double dg = 0.0;
                int dk = -1;                                         // VP: the tile slot of the row's diagonal entry
                if constexpr (VP) dg = oA.dg;
                if (OPS == 3) {
                    group_range(b0, oA.s, row, s_, e_, clip);        // every lane takes part in the cross-lane moves
                    if (row >= nrows_blk) s_ = e_ = 0;
                } else if constexpr (NL) {
                    if (rbase > 0 && (rbase & 63) == 0) {            // more than 64 rows: the next 64 lengths, loaded here (correctness path)
                        const int last = b0.nr - rbase - 1;
                        const int64_t at = (int64_t)b0.r0 + rbase + (lane < last ? lane : last);
                        lens_round(a.len8[at], VP ? a.dpos8[at] : 0, rbase);
                    }
                    const int q = __shfl(pk, row & 63, 64);           // every lane takes part in the cross-lane moves
                    s_ = q & 0xffff;
                    if constexpr (VP) {
                        e_ = s_ + ((q >> 16) & 0xff);
                        dk = s_ + (int)((uint32_t)q >> 24);
                    } else {
                        e_ = s_ + (q >> 16);
                    }
                    if (row >= nrows_blk) s_ = e_ = 0;
                    // VP: every lane of a row needs x[row] and the diagonal value -- whichever of them sums the diagonal's slot
                    if (EPI && rbase > 0 && (VP || sub == 0) && row < nrows_blk) {
                        if (sub == 0) {
                            yo = need_y ? a.yin[b0.r0 + row] : d2{0.0, 0.0};
                            if (FAR) fr = far_at((int64_t)b0.r0 + row, b0.cls);
                        }
                        xi = a.xl[b0.r0 + row];
                        if constexpr (VP) dg = a.diag[b0.r0 + row];
                    }
                } else {
                    int dp = 0;
                    if constexpr (VP) dp = oA.dp;
                    if (rbase > 0) {
                        s_ = e_ = 0;
                        if (row < nrows_blk) {
                            s_ = (int)(a.ia[b0.r0 + row] - b0.p0);
                            e_ = (int)(a.ia[b0.r0 + row + 1] - b0.p0);
                            if constexpr (VP) dp = a.dpos8[b0.r0 + row];
                            if (EPI && (VP || sub == 0)) {
                                if (sub == 0) {
                                    yo = need_y ? a.yin[b0.r0 + row] : d2{0.0, 0.0};
                                    if (FAR) fr = far_at((int64_t)b0.r0 + row, b0.cls);
                                }
                                xi = a.xl[b0.r0 + row];
                                if constexpr (VP) dg = a.diag[b0.r0 + row];
                            }
                        }
                    }
                    if constexpr (VP) dk = s_ + dp;
                }
                d2 sum = {0.0, 0.0};
                if constexpr (VP) {
                    const d2 dprod = cmul(d2{dg, 0.0}, xi);                   // the product of the per-entry stream at that slot, operand for operand
                    for (int k = s_ + sub; k < e_; k += TPR) sum += k == dk ? dprod : prod[k];
                } else {
                    for (int k = s_ + sub * RSTRIDE; k < e_; k += TPR * RSTRIDE) sum += prod[k];
                }
#pragma unroll
                for (int off = TPR / 2; off > 0; off >>= 1) {
                    sum.x += __shfl_xor(sum.x, off, 64);
                    sum.y += __shfl_xor(sum.y, off, 64);
                }
                if (sub == 0 && row < nrows_blk) finish_row(first_row + row, sum, yo, xi, fr, clip);
            }
            close_block(first_row, nrows_blk, b0.cont1);
            QBH_TICK(2, t_mark);               // .. rows reduced and finished
            wave_lds_fence();
        } else {
            open_block(0, 0, false, false);
            for (int r = 0; r < (OPS == 3 ? 0 : b0.nr); ++r) {     // a row longer than the tile: row at a time (correctness path; sliced blocks never exceed the tile)
                const int64_t row = (int64_t)b0.r0 + r;
                const int64_t s_ = a.ia[row], e_ = a.ia[row + 1];
                d2 sum = {0.0, 0.0};
                for (int64_t k = s_ + lane; k < e_; k += 64) sum += cmul(a.val[k], C16 ? a.xg[b0.xb + a.ja16[k]] : a.xg[a.ja[k] & a.colmask]);
                sum.x = wave_sum(sum.x);
                sum.y = wave_sum(sum.y);
                if (lane == 0) {
                    d2 yo = {0.0, 0.0}, xi = {0.0, 0.0}, fr = {0.0, 0.0};
                    if (EPI) {
                        if (need_y) yo = a.yin[row];
                        xi = a.xl[row];
                        if (FAR) fr = far_at(row, b0.cls);
                    }
                    finish_row(row, sum, yo, xi, fr, false);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            cA[u] = cB[u];
            vA[u] = vB[u];
        }
        oA.s = oB.s;
        oA.e = oB.e;
        if constexpr (VP) oA.dp = oB.dp;
        b0 = b1;
        b1 = decode(dq2);
        if constexpr (dyn) {
            if (asking) dw.nxt = dw.take(reply);
        }
        lb += step;
        if constexpr (dyn) dw.advance(lb);
#ifdef QBH_WAVE_TIMING
        // the copy of the next block's registers needs its VALUES: the wait for the rest of the stream lands here
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        QBH_TICK(3, t_mark);
        ++nblk;
#endif
    }
    flush();
    red_flush();
    red_slot = -1;
    }       // hop
#ifdef QBH_XCD_TIMING            // debug build: when does each XCD run out of blocks?  (s_memtime ticks; slots 1 / 2 behind every XCD's counter)
    if (dyn && lane == 0) {
        const unsigned long long t_end = wall_clock64();       // the device-wide constant-rate counter (s_memtime is per XCD)
        atomicMax(a.wctr + (blockIdx.x & 7) * 16 + 1, t_end);
        atomicMin(a.wctr + (blockIdx.x & 7) * 16 + 2, t_end);
    }
#endif
#ifdef QBH_WAVE_TIMING
    if (lane == 0) {
        unsigned long long *dbg = a.wctr + 128 - 8;             // last 8 words of this pass's counter block
        for (int i = 0; i < 4; ++i) atomicAdd(dbg + i, tm[i]);
        atomicAdd(dbg + 4, nblk);
    }
#endif
    if (!CHUNKRED && a.partials != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c * 4 + wv] = acc[c];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                a.partials[(size_t)blockIdx.x * 3 + c] = (red[c * 4 + 0] + red[c * 4 + 1]) + (red[c * 4 + 2] + red[c * 4 + 3]);
        }
    }
}

// slots of the chunk partials -> 256 x 3 partial sums in a fixed order (block b: slots [b * per, (b + 1) * per), lanes striding,
// fixed tree): what finish_reduction / k_reduce_partials then add up.  34 MB at C3, once per SpMV: ~10 us.
__global__ __launch_bounds__(256) void k_reduce_chunks(const double *slots, int64_t n_slots, double *partials)
{
    __shared__ double sm[12];
    const int64_t per = (n_slots + gridDim.x - 1) / gridDim.x, s0 = (int64_t)blockIdx.x * per, s1 = s0 + per < n_slots ? s0 + per : n_slots;
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = s0 + threadIdx.x; i < s1; i += 256) {
        v[0] += slots[i * 3 + 0];
        v[1] += slots[i * 3 + 1];
        v[2] += slots[i * 3 + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 3; ++c) sm[c * 4 + (threadIdx.x >> 6)] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) partials[(size_t)blockIdx.x * 3 + c] = (sm[c * 4 + 0] + sm[c * 4 + 1]) + (sm[c * 4 + 2] + sm[c * 4 + 3]);
}
int launch_reduce_chunks(const double *slots, int64_t n_slots, double *partials, int *nparts_out, hipStream_t s)
{
    const int g = 256;
    hipLaunchKernelGGL(k_reduce_chunks, dim3(g), dim3(256), 0, s, slots, n_slots, partials);
    QBH_HIP(hipGetLastError());
    if (nparts_out) *nparts_out = g;
    return QBH_OK;
}
int64_t wave2_chunk_slots(int64_t n_wb)
{
    const int64_t per = (n_wb + 7) >> 3;
    return 8 * ((per + kDynChunk - 1) / kDynChunk);
}

// instance table of k_spmv_wave2: every tpr other than 2 and 4 takes the 8 form, every pass form other than 0, 1, 3 and 4 is 2;
// 2-byte columns (c16) exist for the one-class near passes and the sliced far pass only, grouped ones (g8) for the latter only,
// row lengths (nl) for the one-class near passes only; grouped values (v8) only beside grouped columns; the shared value pattern
// (vp) for the one-class near passes beside 2-byte columns only, with or without the row lengths
template <int OPS, bool C16, bool G8 = false, bool NL = false, bool V8 = false, bool VP = false>
static SpmvKernel wave2_kernel_tpr(int tpr, bool dyn)
{
    switch (tpr) {
    case 2:  return dyn ? k_spmv_wave2<2, OPS, true, C16, G8, NL, V8, VP> : k_spmv_wave2<2, OPS, false, C16, G8, NL, V8, VP>;
    case 4:  return dyn ? k_spmv_wave2<4, OPS, true, C16, G8, NL, V8, VP> : k_spmv_wave2<4, OPS, false, C16, G8, NL, V8, VP>;
    default: return dyn ? k_spmv_wave2<8, OPS, true, C16, G8, NL, V8, VP> : k_spmv_wave2<8, OPS, false, C16, G8, NL, V8, VP>;
    }
}

template <int OPS, bool C16>
static SpmvKernel wave2_kernel_nl(int tpr, bool dyn, bool nl, bool vp = false)
{
    if constexpr (C16) {
        if (vp) return nl ? wave2_kernel_tpr<OPS, true, false, true, false, true>(tpr, dyn) : wave2_kernel_tpr<OPS, true, false, false, false, true>(tpr, dyn);
    } else {
        if (vp) return nullptr;
    }
    return nl ? wave2_kernel_tpr<OPS, C16, false, true>(tpr, dyn) : wave2_kernel_tpr<OPS, C16>(tpr, dyn);
}

static SpmvKernel wave2_kernel(int tpr, int ops, bool dyn, bool c16, bool g8, bool nl, bool v8, bool vp)
{
    if (nl && ops != 1 && ops != 2) return nullptr;
    if (v8 && !g8) return nullptr;
    if (vp && !c16) return nullptr;
    if (g8) {
        if (!c16 || ops != 3) return nullptr;
        return v8 ? wave2_kernel_tpr<3, true, true, false, true>(tpr, dyn) : wave2_kernel_tpr<3, true, true>(tpr, dyn);
    }
    if (c16) {
        switch (ops) {
        case 1:  return wave2_kernel_nl<1, true>(tpr, dyn, nl, vp);
        case 2:  return wave2_kernel_nl<2, true>(tpr, dyn, nl, vp);
        case 3:  return wave2_kernel_tpr<3, true>(tpr, dyn);
        default: return nullptr;
        }
    }
    switch (ops) {
    case 0:  return wave2_kernel_tpr<0, false>(tpr, dyn);
    case 1:  return wave2_kernel_nl<1, false>(tpr, dyn, nl);
    case 3:  return wave2_kernel_tpr<3, false>(tpr, dyn);
    case 4:  return wave2_kernel_tpr<4, false>(tpr, dyn);
    default: return wave2_kernel_nl<2, false>(tpr, dyn, nl);
    }
}

int launch_spmv_wave2(const SpmvArgs &a_in, int tpr, int ops, int grid, hipStream_t s)
{
    SpmvArgs a = a_in;
    if (a.yin == nullptr) a.yin = a.y;           // the beta term reads y itself unless a driver names another vector
    if (a.swizzle == 3 && (ops == 1 || ops == 2 || ops == 4) && a.chunk_red == nullptr) {
        set_error("launch_spmv_wave2: the dynamic walk of an epilogue pass needs its chunk-partial slots");
        return QBH_EINVAL;
    }
    const SpmvKernel k = wave2_kernel(tpr, ops, a.swizzle == 3, a.ja16 != nullptr, a.ja8 != nullptr, a.len8 != nullptr, a.val8 != nullptr, a.valp != nullptr);
    if (k == nullptr) {
        set_error("launch_spmv_wave2: %s%s columns%s%s%s with pass form %d", a.ja16 ? "2-byte" : "int32", a.ja8 ? " grouped" : "", a.len8 ? " / row lengths" : "",
                  a.val8 ? " / grouped values" : "", a.valp ? " / shared value pattern" : "", ops);
        return QBH_EINVAL;
    }
    return launch_kernel(k, grid, kBlock, s, a);
}

// asks about the ordered dynamic walk with int32 columns (DYN = true, C16 = false) whatever the launch will use: kept as found
int wave2_kernel_occupancy(int tpr, int ops)
{
    return kernel_occupancy(wave2_kernel(tpr, ops, true, false, false, false, false, false));
}

}  // namespace qbh
