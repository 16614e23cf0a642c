// qbh_kondo_lds.hpp -- what the kernels of the Kondo momentum sectors share: the tables they stage in LDS, the choice between
// the two workgroup shapes and the launch.  Used by qbh_sector_mf_kondo.hip (qbh_mf_kondo_repr) and qbh_kondo_mopr.hip
// (qbh_mopr_kondo_repr_dev).
//
// The translation tables and the two counting tables A and binom of a KondoDev are always staged in LDS: with at most 21 sites
// (4 six-bit chunks per field) and 64 translations they take at most 138,816 B.
#pragma once
#include "qbh_sector.hpp"

namespace qbh {
namespace {

constexpr int kKondoTabEntries = kKondoTab * kKondoTab;
constexpr size_t kMfKreprLdsCap = (size_t)150 * 1024;         // the budget of launch_mf_heis
constexpr size_t kMfKreprLdsMax =
    ((size_t)kReprMaxTrans * ((kKondoMaxSites + 5) / 6) * 64 + 2 * (size_t)kKondoTabEntries) * sizeof(uint64_t);
static_assert(kMfKreprLdsMax == 138816 && kMfKreprLdsMax <= kMfKreprLdsCap,
              "the translation tables, A and binom of every admissible sector fit LDS: there is no global-memory path");

// Two workgroup shapes for one kernel body.  A CU holds per_cu workgroups of 256 lanes (what the registers of the kernel
// admit) or one of 1024, and the LDS the tables take (160 KB per CU) decides between them:
//   four or more workgroups of 256 lanes fit:  256 lanes, min(per_cu, 160 KB / footprint) per CU
//   fewer fit (footprint above 40 KB):         1024 lanes, one workgroup per CU: 16 waves per CU instead of 4 to 12
constexpr int kMfKreprBlockS = 256, kMfKreprBlockL = 1024;
constexpr size_t kMfKreprLdsCu = (size_t)160 * 1024;
constexpr size_t kMfKreprLdsStatic = 1024;                    // the reduction scratch of a workgroup and allocation granules

inline size_t krepr_lds_bytes(int n_tab) { return ((size_t)n_tab + 2 * (size_t)kKondoTabEntries) * sizeof(uint64_t); }
inline int krepr_fit(int n_tab) { return (int)(kMfKreprLdsCu / (krepr_lds_bytes(n_tab) + kMfKreprLdsStatic)); }
inline bool krepr_large(int n_tab) { return krepr_fit(n_tab) < 4; }

// the resident grid for nrows rows; per_cu: the register-limited workgroups of 256 lanes per CU of the kernel
inline int krepr_grid(int n_tab, int64_t nrows, int per_cu_small)
{
    const bool large = krepr_large(n_tab);
    const int block = large ? kMfKreprBlockL : kMfKreprBlockS;
    const int per_cu = large ? 1 : std::min(per_cu_small, krepr_fit(n_tab));
    const int64_t nblk = (nrows + block - 1) / block;
    return (int)std::min<int64_t>(nblk, std::min<int64_t>((int64_t)device_cu_count() * per_cu, kMaxRedBlocks));
}

// tab | A | binom into LDS and the pointers the row walk reads them through (K: the sector whose words are ranked)
__device__ __forceinline__ void krepr_stage(const uint64_t *g_tab, int n_tab, const KondoDev &K, uint64_t *lds, int nthreads,
                                            const uint64_t *&tab, const uint64_t *&A, const uint64_t *&binom)
{
    for (int k = threadIdx.x; k < n_tab; k += nthreads) lds[k] = g_tab[k];
    for (int k = threadIdx.x; k < kKondoTabEntries; k += nthreads) {
        lds[n_tab + k] = K.A[k];
        lds[n_tab + kKondoTabEntries + k] = K.binom[k];
    }
    __syncthreads();
    tab = lds;
    A = lds + n_tab;
    binom = A + kKondoTabEntries;
}

template <class Kernel, class... Args>
hipError_t krepr_launch(Kernel k, int grid, int block, size_t lds, hipStream_t s, Args... args)
{
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(block), lds, s, args...);
    return hipGetLastError();
}

}  // namespace
}  // namespace qbh
