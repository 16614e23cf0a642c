// qbh_corr.hpp -- what the seven all-pair correlation calls share (full sectors: qbh_corr.hip, qbh_corr_qudit.hip,
// qbh_corr_kondo.hip; momentum sectors, with qbh_corr_repr.hpp on top: qbh_corr_repr.hip, qbh_corr_hubrepr.hip,
// qbh_corr_quditrepr.hip, qbh_corr_kondorepr.hip).  Device: the block reduction into partials[blockIdx.x][pass][accumulator],
// a row's amplitude and uniform loads.  Host: the argument checks, the two grid rules, the one launch path with its two-stage
// reduction (defined in qbh_corr.hip), the layout of the passes in the reduced sums and the fills of the output arrays that
// several families share.
#pragma once
#include <algorithm>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_device.hpp"

namespace qbh {

constexpr int kCorrBlock = 256;                              // 155 VGPRs (real spin form): three workgroups of four wavefronts per CU
constexpr size_t kCorrLdsCap = (size_t)150 * 1024;           // the budget of launch_mf_heis

// acc summed over the workgroup of BLOCK lanes into partials[(blockIdx.x * gridDim.y + blockIdx.y) * NA ..]: every wavefront, then
// lane c adds the wavefronts of accumulator c in order (the pattern of mf_block_partials for NA accumulators).  red: NA * (BLOCK / 64).
template <int NA, int BLOCK = kCorrBlock>
__device__ __forceinline__ void corr_block_partials(double (&acc)[NA], double *red, double *partials)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NA; ++c) red[c * (BLOCK / 64) + wave] = acc[c];
    }
    __syncthreads();
    if (tid < NA) {
        double s = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) s += red[tid * (BLOCK / 64) + w];
        partials[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * NA + tid] = s;
    }
}

// v is the same in every lane: keep it in scalar registers
__device__ __forceinline__ uint32_t corr_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t corr_uniform(uint64_t v)
{
    return ((uint64_t)corr_uniform((uint32_t)(v >> 32)) << 32) | corr_uniform((uint32_t)v);
}

// the amplitude of `row`: exactly one of xg (complex) / xr (packed real, no imaginary part) is given
template <bool REALX>
__device__ __forceinline__ d2 corr_load_x(const d2 *xg, const double *xr, int64_t row)
{
    d2 x = {0.0, 0.0};
    if (REALX) x.x = xr[row];
    else       x = xg[row];
    return x;
}

// the bounds of a pass's G groups in a padded start array: group g owns [k0[g], k0[g + 1])
template <int G>
__device__ __forceinline__ void corr_group_bounds(const int32_t *start, int first, int (&k0)[G + 1])
{
#pragma unroll
    for (int g = 0; g <= G; ++g) k0[g] = (int)corr_uniform((uint32_t)start[first + g]);
}

// The row loop of the three full-sector kernels (k_corr_spin, k_corr_qudit, k_corr_kondo) is written out in each of them.  A pass
// has to know every row's word again, and unranking it (a dependent LDS walk per site) would cost a large part of a pass.  So a
// workgroup takes tiles of kCorrBlock * R CONSECUTIVE rows: every lane unranks one row and steps to the next R - 1 words in order,
// the tile's words go through LDS, and the lanes then take them row-interleaved, so that consecutive lanes still hold consecutive
// rows for the gathers.  A lane's R words are R + 1 words apart from the next lane's (an odd stride: neither the stores nor the
// loads meet in a bank).  A shared template with the two steps as callables was tried and dropped: the compiler then contracts
// two multiply-adds of the packed-real Kondo LL instance differently (one result moves by an ulp) and takes 6 more VGPRs in one
// spin instance.

// ---------------------------------------------------------------------------------------------------------- host --
// the refusals every call shares (QBH_EINVAL, QBH_EINVAL, QBH_ENODEVICE); each call keeps them at its own place in its order
int corr_check_vectors(const char *who, const void *d_vec, const void *d_vec_re);
int corr_check_norm2(const char *who, const double *norm2);
int corr_check_device();

// Workgroups along x, two rules.  corr_grid, full sectors: 256 lanes walk tiles of `rows_per_block` rows; a CU holds what its LDS
// lets it (158 KB over the tables + 2 KB of reduction scratch and granules), four workgroups at most, one at least.
// repr_launch_shape, momentum sectors: one lane per representative; 160 KB over the tables + 4 KB, and when fewer than four
// workgroups of 256 lanes fit, ONE of 1024 lanes (a large table is then staged once per CU, and its kernels keep the four
// wavefronts per SIMD that needs).  The rules belong to different kernels and their numbers are not merged: the grid fixes the
// order of summation and with it the bits of every result, and the tests mirror corr_grid.
int corr_grid(int64_t dim, size_t lds, int rows_per_block);

constexpr int kReprBlockS = 256, kReprBlockL = 1024;
constexpr int kReprPerCuS = 4;                               // workgroups of 256 lanes per CU at most
constexpr size_t kReprLdsCu = (size_t)160 * 1024;
constexpr size_t kReprLdsStatic = 4096;                      // the reduction scratch of a workgroup and allocation granules

struct ReprShape {
    bool large;
    int block, gx;
};

inline ReprShape repr_launch_shape(size_t lds, int64_t dim)
{
    const int fit = (int)(kReprLdsCu / (lds + kReprLdsStatic));
    ReprShape s;
    s.large = fit < 4;
    s.block = s.large ? kReprBlockL : kReprBlockS;
    const int per_cu = s.large ? 1 : std::min(kReprPerCuS, fit);
    const int64_t nblk = (dim + s.block - 1) / s.block;
    s.gx = (int)std::max<int64_t>(1, std::min<int64_t>(nblk, (int64_t)device_cu_count() * per_cu));
    return s;
}

// the untyped core of every launch: set the dynamic LDS of `kernel` (one argument, *arg), launch it on (gx, n_pass) workgroups
// of `block` lanes, return the last error
hipError_t corr_launch(const void *kernel, int gx, int n_pass, int block, size_t lds, hipStream_t s, const void *arg);
// A reduced launch owns partials [gx][n_pass * na] and, behind them, their sums [n_pass * na]: corr_reduce_doubles of them.
// corr_reduce_launch points arg.partials at `slice`, the caller's piece of a larger allocation, or with slice = NULL at a fresh
// allocation given to the pool, launches kernel(arg), adds the workgroups in the order of k_corr_reduce and downloads the sums
// into out.  `who` names the public entry point in the message of a HIP failure.
size_t corr_reduce_doubles(int gx, int n_pass, int na);
int corr_reduce_launch_any(const char *who, const void *kernel, int gx, int n_pass, int na, int block, size_t lds, hipStream_t s,
                           const void *arg, double **partials, std::vector<void *> &pool, std::vector<double> &out);
template <typename Args>
int corr_reduce_launch(const char *who, void (*kernel)(Args), int gx, int n_pass, int na, int block, size_t lds, hipStream_t s, Args &arg,
                       double *slice, std::vector<void *> &pool, std::vector<double> &out)
{
    arg.partials = slice;
    return corr_reduce_launch_any(who, reinterpret_cast<const void *>(kernel), gx, n_pass, na, block, lds, s, &arg, &arg.partials, pool, out);
}

// Where the passes of every kind lie in the reduced sums comp[pass][NA]; kinds (at most 5) are added in pass order.
struct CorrPasses {
    int n_pass = 0, first[5] = {}, count[5] = {};
    void add(int kind, int n_items, int per_pass)
    {
        first[kind] = n_pass;
        n_pass += count[kind] = (n_items + per_pass - 1) / per_pass;
    }
    // accumulator `slot` of `item`: slot-major [slot][item % per_pass] ...
    double at(const std::vector<double> &comp, int kind, int item, int per_pass, int slot, int NA) const
    {
        return comp[(size_t)(first[kind] + item / per_pass) * NA + (size_t)slot * per_pass + item % per_pass];
    }
    // ... or item-major [item % per_pass][slot] with per_item accumulators an item
    double at_item(const std::vector<double> &comp, int kind, int item, int per_pass, int per_item, int slot, int NA) const
    {
        return comp[(size_t)(first[kind] + item / per_pass) * NA + (size_t)per_item * (item % per_pass) + slot];
    }
};

// out[i][j] = v, out[j][i] = conj v
inline void corr_put_herm(qbh_z *out, int N, int i, int j, double re, double im)
{
    out[(size_t)i * N + j] = qbh_z{re, im};
    out[(size_t)j * N + i] = qbh_z{re, -im};
}

// nn[2A + B][i][i] = <n_A n_B> of one site: n^2 = n
inline void corr_put_nn_diag(double *nn, int N, int i, double nu, double docc, double nd)
{
    const size_t NN = (size_t)N * N, ii = (size_t)i * N + i;
    nn[0 * NN + ii] = nu;
    nn[1 * NN + ii] = docc;
    nn[2 * NN + ii] = docc;
    nn[3 * NN + ii] = nd;
}

// nn[..][i][j] and nn[..][j][i] from the four sums of the pair i < j: <n_{i,up} n_{j,dn}> is the du entry of (j, i)
inline void corr_put_nn_pair(double *nn, int N, int i, int j, double uu, double ud, double du, double dd)
{
    const size_t NN = (size_t)N * N, ij = (size_t)i * N + j, ji = (size_t)j * N + i;
    nn[0 * NN + ij] = nn[0 * NN + ji] = uu;
    nn[1 * NN + ij] = nn[2 * NN + ji] = ud;
    nn[2 * NN + ij] = nn[1 * NN + ji] = du;
    nn[3 * NN + ij] = nn[3 * NN + ji] = dd;
}

// nn[..][i][j] from the sums UU, DD, F, B of the class of (i, j) with n_u unordered pairs: <n_{i,up} n_{j,dn}> from the forward
// orientations and, from the mirror orientation, <n_{i,dn} n_{j,up}> = <n_{j,up} n_{i,dn}>; a class that is its own mirror has
// only forward pairs
inline void corr_put_nn_class(double *nn, int N, int i, int j, double uu, double dd, double f, double b, double n_u, bool self,
                              bool forward)
{
    const size_t NN = (size_t)N * N, ij = (size_t)i * N + j;
    nn[ij] = uu / n_u;
    nn[NN + ij] = self ? f / (2.0 * n_u) : (forward ? f : b) / n_u;
    nn[2 * NN + ij] = self ? f / (2.0 * n_u) : (forward ? b : f) / n_u;
    nn[3 * NN + ij] = dd / n_u;
}

// the diagonals that follow from a site's sums (a NULL array is skipped): hop[s][i][i] = n_s, flip or ee [i][i] = n_up - docc
inline void corr_put_onsite_diag(qbh_z *hop, qbh_z *flip, int N, int i, double nu, double nd, double docc)
{
    const size_t NN = (size_t)N * N, ii = (size_t)i * N + i;
    if (hop) {
        hop[0 * NN + ii] = qbh_z{nu, 0.0};
        hop[1 * NN + ii] = qbh_z{nd, 0.0};
    }
    if (flip) flip[ii] = qbh_z{nu - docc, 0.0};
}

// <S^z_i S^z_j> from D = sum |psi|^2 [the two spins differ]
inline double corr_zz_pair(double n2, double D) { return 0.25 * (n2 - 2.0 * D); }

}  // namespace qbh
