// qbh_corr.hpp -- what the all-pair correlation kernels share (qbh_corr.hip: spin-1/2 and two-species fermions; qbh_corr_qudit.hip:
// d-level sites): the block size and LDS budget, the block reduction into partials[blockIdx.x][pass][accumulator], and the host
// side of a launch (grid rule, second stage k_corr_reduce + download; defined in qbh_corr.hip).
#pragma once
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_device.hpp"

namespace qbh {

constexpr int kCorrBlock = 256;                              // 155 VGPRs (real spin form): three workgroups of four wavefronts per CU
constexpr size_t kCorrLdsCap = (size_t)150 * 1024;           // the budget of launch_mf_heis

// acc summed over the workgroup into partials[(blockIdx.x * gridDim.y + blockIdx.y) * NA ..]: every wavefront, then lane c adds
// the wavefronts of accumulator c in order (the pattern of mf_block_partials for NA accumulators).  red: NA * (kCorrBlock / 64).
template <int NA>
__device__ __forceinline__ void corr_block_partials(double (&acc)[NA], double *red, double *partials)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NA; ++c) red[c * (kCorrBlock / 64) + wave] = acc[c];
    }
    __syncthreads();
    if (tid < NA) {
        double s = 0.0;
        for (int w = 0; w < kCorrBlock / 64; ++w) s += red[tid * (kCorrBlock / 64) + w];
        partials[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * NA + tid] = s;
    }
}

// v is the same in every lane: keep it in scalar registers
__device__ __forceinline__ uint32_t corr_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t corr_uniform(uint64_t v)
{
    return ((uint64_t)corr_uniform((uint32_t)(v >> 32)) << 32) | corr_uniform((uint32_t)v);
}

// workgroups along x: what the LDS lets a CU hold (four at most), each walking its share of the `rows_per_block`-row pieces
int corr_grid(int64_t dim, size_t lds, int rows_per_block);
// second stage + download: out[ncomp] = sum over the n_parts workgroups, in the order of k_corr_reduce; the sums are written
// behind the partials, which therefore hold (n_parts + 1) * ncomp doubles
int corr_finish(double *d_partials, int n_parts, int ncomp, std::vector<double> &out, hipStream_t s);

}  // namespace qbh
