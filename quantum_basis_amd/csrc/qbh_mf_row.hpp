// qbh_mf_row.hpp -- what the lane-per-row matrix-free kernels share once a row's off-diagonal sum is known: the operands of
// the fused epilogue, the epilogue itself, the workgroup's three partial sums, and the gather-accumulate of one entry.
// The expressions and their order ARE the definition of y <- alpha*(Hx) + beta*y + gamma*x for these kernels: a reordering
// changes the FMA contraction and with it the last bit of every result.
#pragma once

#include "qbh_device.hpp"

namespace qbh {

// old y and the row's own x of local row lrow = global row grow (the gather source holds the row's own element)
template <bool REALX>
__device__ __forceinline__ void mf_row_load(const MfVec &v, int64_t lrow, int64_t grow, d2 &yo, d2 &xi)
{
    yo = d2{0.0, 0.0};
    xi = d2{0.0, 0.0};
    if (v.y_re != nullptr) {                   // all-real operation (REALX): y and x as doubles
        if (v.beta != 0.0) yo.x = v.y_re[lrow];
        xi.x = v.xr[grow];
    } else {
        if (v.beta != 0.0) yo = v.y[lrow];
        if (REALX) xi.x = v.xr[grow];
        else       xi = v.xg[grow];
    }
}

// the row's real diagonal dg joins its sum; y <- alpha*sum + beta*yo + gamma*xi; <x, y> and |y|^2 run on in acc
__device__ __forceinline__ void mf_row_finish(const MfVec &v, int64_t lrow, d2 sum, double dg, d2 xi, d2 yo, double (&acc)[3])
{
    sum += dg * xi;
    const d2 yn = v.alpha * sum + v.beta * yo + v.gamma * xi;
    if (v.y_re != nullptr) v.y_re[lrow] = yn.x;
    else                   v.y[lrow] = yn;
    // acc[0] += xi.x * yn.x + xi.y * yn.y and acc[2] += yn.x * yn.x + yn.y * yn.y with the contraction written out: which of
    // the two products of a sum the compiler fuses is its own tie-break (it moved when this code became a function), and the
    // choice is the last bit of the reduced scalars.  A difference has one reading (the first product is the fused one).
    acc[0] += fma(xi.x, yn.x, xi.y * yn.y);
    acc[1] += xi.x * yn.y - xi.y * yn.x;
    acc[2] += fma(yn.x, yn.x, yn.y * yn.y);
}

// acc summed over a workgroup of BLOCK lanes into partials[blockIdx.x * 3 ..]: every wavefront, then lane 0 adds the
// wavefronts in order.  red holds 3 * (BLOCK / 64) doubles of LDS; every lane of the workgroup calls (partials is uniform).
template <int BLOCK>
__device__ __forceinline__ void mf_block_partials(double (&acc)[3], double *red, double *partials)
{
    if (partials == nullptr) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) red[c * (BLOCK / 64) + wave] = acc[c];
    }
    __syncthreads();
    if (tid == 0) {
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int w2 = 0; w2 < BLOCK / 64; ++w2) s += red[c * (BLOCK / 64) + w2];
            partials[(size_t)blockIdx.x * 3 + c] = s;
        }
    }
}

// sum += val * x[col]: the packed real parts (REALX; the entry's value is real then) or the complex gather source
template <bool REALX>
__device__ __forceinline__ void mf_gather_add(const MfVec &v, d2 &sum, d2 val, int64_t col)
{
    if (REALX) {
        sum.x += val.x * v.xr[col];
    } else {
        const d2 x = v.xg[col];
        sum.x += val.x * x.x - val.y * x.y;
        sum.y += val.x * x.y + val.y * x.x;
    }
}

// one sum per workgroup of BLOCK lanes for the kernels that count what an apply kernel would add: part[blockIdx.x]
template <int BLOCK>
__device__ __forceinline__ void mf_block_count(unsigned long long c, unsigned long long *red, unsigned long long *part)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < BLOCK / 64; ++w) s += red[w];
        part[blockIdx.x] = s;
    }
}

}  // namespace qbh
