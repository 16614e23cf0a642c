// qbh_device.hpp -- device helpers shared by the SpMV, BLAS-1 and matrix-free kernels: complex product, non-temporal load,
// wavefront / workgroup sums, the XCD-aware walks over blocks and the fused row epilogue.
#pragma once

#include "qbh_internal.hpp"

namespace qbh {

// ------------------------------------------------------------------ helpers ----
__device__ __forceinline__ d2 cmul(d2 a, d2 b)
{
    d2 r;
    r.x = a.x * b.x - a.y * b.y;
    r.y = a.x * b.y + a.y * b.x;
    return r;
}

template <typename T>
__device__ __forceinline__ T ntload(const T *p)
{
    return __builtin_nontemporal_load(p);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum NC doubles per thread over the workgroup; result valid in thread 0.
// `scratch` must hold NC*4 doubles of LDS.  Deterministic (fixed tree).
template <int NC>
__device__ __forceinline__ void block_sum(double (&v)[NC], double *scratch)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = wave_sum(v[c]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) scratch[c * 4 + wave] = v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
            v[c] = (scratch[c * 4 + 0] + scratch[c * 4 + 1]) + (scratch[c * 4 + 2] + scratch[c * 4 + 3]);
    }
}

// XCD-aware walk over row blocks: workgroup w runs on XCD w % 8 (observed dispatch
// order, used for speed only).  With swizzle each XCD walks one contiguous eighth of the
// row blocks so the x windows it gathers stay in its own 4 MiB L2.
struct BlockWalk {
    int64_t per_xcd, xcd, slot, nslot, nb, chunk;
    int swz;
    __device__ BlockWalk(int64_t n_blocks, int swizzle, int chunk_mult = 1)
    {
        nb = n_blocks;
        per_xcd = (n_blocks + 7) >> 3;
        xcd = blockIdx.x & 7;
        slot = blockIdx.x >> 3;
        nslot = gridDim.x >> 3;
        swz = swizzle;
        // mode 2 walks chunk-wise (a chunk = chunk_mult rounds of the XCD's resident workgroups); round the per-XCD
        // count up to whole chunks so every block is visited
        chunk = nslot * (chunk_mult > 0 ? chunk_mult : 1);
        if (swz == 2) per_xcd = ((per_xcd + chunk - 1) / chunk) * chunk;
    }
    // lb = this XCD's local sequence number (slot, slot + nslot, ...).
    //  0: interleaved           block = lb*8 + xcd        (all XCDs sweep the same region)
    //  1: contiguous eighths    block = xcd*per_xcd + lb  (each XCD owns one eighth of the rows)
    //  2: chunked               the concurrently resident workgroups of an XCD (nslot of them) take
    //                           one contiguous chunk (chunk_mult rounds long); the 8 XCDs take 8 neighbouring chunks
    __device__ int64_t block(int64_t lb) const
    {
        if (swz == 1) return xcd * per_xcd + lb;
        if (swz == 2) return ((lb / chunk) * 8 + xcd) * chunk + (lb % chunk);
        return lb * 8 + xcd;
    }
};

// Dynamic ORDERED walk of the wave kernels (xcd_swizzle 3).  A persistent static walk lets the workgroups of an XCD drift apart
// (nothing synchronises them over thousands of blocks): on C3 their union of x windows then no longer fits the L2 -- 45 % of
// the gathers of the band-major far part missed a 1.65 MB window that the L2 holds perfectly in isolation, and the count did
// not depend on the band width (narrower bands, proportionally more of them in flight).  Here every XCD owns one contiguous
// eighth of the wave blocks and ALL its wavefronts draw chunks of kDynChunk consecutive blocks from one counter, so the eighth
// is consumed in order and the blocks in flight on an XCD are always neighbours.  blockIdx % 8 names the counter (the observed
// dispatch order puts those workgroups on one XCD; if it did not, only the locality would suffer).
#ifndef QBH_DYN_CHUNK
#define QBH_DYN_CHUNK 4
#endif
constexpr int kDynChunk = QBH_DYN_CHUNK;
static_assert(kDynChunk >= 3, "the walk looks two turns ahead and learns the next chunk in the first turn of the current one");
struct DynWalk {
    // cur: first block of the chunk the wavefront is in (turns n0 .. n0 + kDynChunk - 1); nxt: of the chunk after it.  The
    // counter is asked (ask) in the first turn of a chunk BEFORE that turn's gathers and read (take) after they have been
    // waited for: results return in order, so the reply costs no wait of its own and never drains the stream loads issued
    // behind it.  (An atomic add would be rewritten by the compiler into a wave reduction that reads the reply at once;
    // the wrapping increment is left alone, and the counter counts chunks.)
    int64_t xbase, xend, n_wb, cur, nxt, n0;
    int region;
    unsigned int *ctr;
    __device__ unsigned int ask(int lane) const
    {
        unsigned int c = 0;
        if (lane == 0) c = atomicInc(ctr, 0xFFFFFFFFu);
        return c;
    }
    __device__ int64_t take(unsigned int c) const { return xbase + (int64_t)__builtin_amdgcn_readfirstlane(c) * kDynChunk; }
    // region: whose eighth of the blocks (0..7); a wavefront starts on its own XCD's and, when that is exhausted, joins the
    // queues of the others one after the other (k_spmv_wave2's hop loop): the XCDs do not run at the same speed
    __device__ void init(int64_t n_blocks, unsigned long long *counters, int lane, int region = -1)
    {
        n_wb = n_blocks;
        const int xcd = region < 0 ? (int)(blockIdx.x & 7) : region;
        this->region = xcd;
        const int64_t per = (n_blocks + 7) >> 3;
        xbase = xcd * per;
        xend = xbase + per < n_blocks ? xbase + per : n_blocks;
        ctr = reinterpret_cast<unsigned int *>(counters + xcd * 16);
        cur = take(ask(lane));
        nxt = xend;
        n0 = 0;
    }
    __device__ bool asks(int64_t n) const { return n == n0; }        // the turn that draws the next chunk
    // number of the CURRENT chunk among all chunks of the launch (8 regions x chunks per region): where its reduction partials go
    __device__ int64_t chunk_slot() const
    {
        const int64_t per = (n_wb + 7) >> 3, cpx = (per + kDynChunk - 1) / kDynChunk;
        return (int64_t)region * cpx + (cur - xbase) / kDynChunk;
    }
    __device__ int64_t at(int64_t n) const { return (n < n0 + kDynChunk ? cur : nxt) + n % kDynChunk; }
    // wave block of this wavefront's n-th turn (n = the current turn .. two turns ahead); n_wb = the sentinel (past the end)
    __device__ int64_t block(int64_t n) const
    {
        const int64_t w = at(n);
        return w < xend ? w : n_wb;
    }
    __device__ bool live(int64_t n) const { return at(n) < xend; }
    // after moving on to turn n
    __device__ void advance(int64_t n)
    {
        if (n % kDynChunk == 0) {
            cur = nxt;
            n0 = n;
        }
    }
};

// fused epilogue of one row: y <- alpha*(Hx) + beta*y + gamma*x_local, and the running
// partial sums of <x,y> and |y|^2 (K3, K4 and the CG shift folded into K1).
// yo / xi are the old y[row] and x_local[row], loaded by the caller (so that the loads can
// be issued long before the row sum is ready).
// rowmap (far part of a coded Kronecker split): the kernel's rows are in tiled order, the vectors are not
__device__ __forceinline__ int64_t out_row(const SpmvArgs &a, int64_t row)
{
    return a.rowmap ? KronTile{a.kS, a.kNU, a.kB}.orig(row) : row;
}
__device__ __forceinline__ d2 load_y_old(const SpmvArgs &a, int64_t row)
{
    row = out_row(a, row);
    return a.y_re != nullptr ? d2{a.y_re[row], 0.0} : a.yin[row];
}
__device__ __forceinline__ d2 load_x_local(const SpmvArgs &a, int64_t row)
{
    row = out_row(a, row);
    return a.y_re != nullptr ? d2{a.xl_re[row], 0.0} : a.xl[row];
}

__device__ __forceinline__ void row_epilogue2(const SpmvArgs &a, int64_t row, d2 sum, d2 yo, d2 xi,
                                              double (&acc)[3])
{
    d2 yn = a.alpha * sum + a.beta * yo + a.gamma * xi;
    row = out_row(a, row);
    if (a.y_re != nullptr) a.y_re[row] = yn.x;
    else                   a.y[row] = yn;
    acc[0] += xi.x * yn.x + xi.y * yn.y;
    acc[1] += xi.x * yn.y - xi.y * yn.x;
    acc[2] += yn.x * yn.x + yn.y * yn.y;
}

__device__ __forceinline__ void row_epilogue(const SpmvArgs &a, int64_t row, d2 sum, double (&acc)[3])
{
    d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
    if (a.beta != 0.0) yo = load_y_old(a, row);
    if (a.gamma != 0.0 || a.partials != nullptr) xi = load_x_local(a, row);
    row_epilogue2(a, row, sum, yo, xi, acc);
}

}  // namespace qbh
