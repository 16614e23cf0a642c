// qbh_kondo.hip -- device assembly of the Kondo lattice model (conduction electrons plus a localized spin-1/2 on every
// site; the reference's add_orbital("electron") + add_orbital("spin-1/2") examples): qbh_gen_kondo, the same operator applied
// without a stored matrix (qbh_mf_kondo, k_mf_kondo), and the term checks the momentum-sector generator in qbh_sector.hip
// shares.  Basis, ranking and the row terms: qbh_kondo.hpp.
//
// Count -> scan -> fill.  The fill kernel follows k_qudit_fill: one row per lane, its entries insertion-sorted by column in
// the lane's own LDS column as (column, entry code), the values decoded from the codes on the way out.  No private array,
// so nothing spills to scratch; the two counting tables (2 x 22 x 22 x 8 B) sit in LDS in both kernels.
#include <algorithm>
#include <array>
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_kondo.hpp"
#include "qbh_mf_row.hpp"

namespace qbh {
namespace {

constexpr int kKondoFillBlock = 64;      // one wave per workgroup in the fill kernel: lane = row, LDS column = lane
constexpr int kKondoTabWords = 2 * kKondoTab * kKondoTab;

// A and binom into LDS: lds[0, 484) = A, lds[484, 968) = binom
__device__ __forceinline__ void kd_stage_tables(uint64_t *lds, const KondoDev &K, int nthreads)
{
    for (int k = threadIdx.x; k < kKondoTab * kKondoTab; k += nthreads) {
        lds[k] = K.A[k];
        lds[kKondoTab * kKondoTab + k] = K.binom[k];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_kondo_count(const KondoDev *Kp, int64_t row_begin, int64_t row_end, int32_t *cnt)
{
    __shared__ uint64_t lds[kKondoTabWords];
    const KondoDev &K = *Kp;
    kd_stage_tables(lds, K, 256);
    const uint64_t *A = lds, *binom = lds + kKondoTab * kKondoTab;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; row < row_end; row += stride) {
        uint64_t u, d, s, ru, rd;
        kd_unrank(K, A, binom, (uint64_t)row, &u, &d, &s, &ru, &rd);
        int c = 1;
        kd_row_terms(K, u, d, s, [&](uint64_t, uint64_t, uint64_t, int) { ++c; });
        cnt[row - row_begin] = c;
    }
}

// entry k of lane L at k * 64 + L; code -1 = the diagonal.  max_row (from the merged terms) bounds the entries of a row.
__global__ __launch_bounds__(kKondoFillBlock) void k_kondo_fill(const KondoDev *Kp, int max_row, int64_t row_begin, int64_t row_end,
                                                                const int64_t *ia, int32_t *ja, d2 *val)
{
    extern __shared__ uint64_t kd_lds[];
    const KondoDev &K = *Kp;
    kd_stage_tables(kd_lds, K, kKondoFillBlock);
    const uint64_t *A = kd_lds, *binom = kd_lds + kKondoTab * kKondoTab;
    int32_t *scol = reinterpret_cast<int32_t *>(kd_lds + kKondoTabWords) + threadIdx.x;
    int32_t *sent = scol + kKondoFillBlock * max_row;
    const int64_t stride = (int64_t)gridDim.x * kKondoFillBlock;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * kKondoFillBlock + threadIdx.x; row < row_end; row += stride) {
        uint64_t u, d, s, ru, rd;
        kd_unrank(K, A, binom, (uint64_t)row, &u, &d, &s, &ru, &rd);
        int n = 0;
        auto put = [&](int32_t c, int32_t code) {
            if (n >= max_row) return;                          // never: max_row counts every term of the row
            int q = n++;
            while (q > 0 && scol[(q - 1) * kKondoFillBlock] > c) {
                scol[q * kKondoFillBlock] = scol[(q - 1) * kKondoFillBlock];
                sent[q * kKondoFillBlock] = sent[(q - 1) * kKondoFillBlock];
                --q;
            }
            scol[q * kKondoFillBlock] = c;
            sent[q * kKondoFillBlock] = code;
        };
        const d2 dg = kd_row_terms(K, u, d, s, [&](uint64_t u2, uint64_t d2w, uint64_t s2, int code) {
            put((int32_t)kd_rank(K, A, binom, u2, d2w, s2), code);
        });
        put((int32_t)row, -1);
        const int64_t p0 = ia[row - row_begin];
        for (int q = 0; q < n; ++q) {
            const int code = sent[q * kKondoFillBlock];
            ja[p0 + q] = scol[q * kKondoFillBlock];
            val[p0 + q] = code < 0 ? dg : kd_value(K, code);
        }
    }
}

// ------------------------------------------------------------------------------------ matrix-free apply (kind 5) --
// y <- alpha H x + beta y + gamma x without a stored matrix.  One lane per row, grid-stride over a resident grid; A and binom
// in LDS, the merged terms read through the kernel's KondoDev pointer (uniform over the lanes).  The row is unranked once
// and its terms walked by kd_row_terms; the hook gathers x[column] and accumulates in the order the terms arrive, so a row's
// sum depends on nothing but the row.  Columns:
//   hop           one species moves inside the block of s: row + (rank' - rank) of that species, times C(n, n_up) for the
//                 down species; the difference runs over the particles between the two sites only
//   spin exchange popcount(s) stays: kd_srank(s') + the row's rank inside its block (rd C(n, n_up) + ru)
//   Kondo flip    the block changes: kd_rank of all three fields
constexpr int kMfKondoBlock = 256;
constexpr int kMfKondoPerCu = 7;         // workgroups per CU of the resident grid: 66 VGPRs admit 7 waves per SIMD

template <bool REALX>
__global__ __launch_bounds__(kMfKondoBlock) void k_mf_kondo(MfKondo t, MfVec a)
{
    __shared__ uint64_t lds[kKondoTabWords];
    __shared__ double red[3 * (kMfKondoBlock / 64)];
    const KondoDev &K = *t.K;
    kd_stage_tables(lds, K, kMfKondoBlock);
    const uint64_t *A = lds, *binom = lds + kKondoTab * kKondoTab;
    const int tid = threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kMfKondoBlock;
    for (int64_t lrow = (int64_t)blockIdx.x * kMfKondoBlock + tid; lrow < a.nrows; lrow += stride) {
        const uint64_t grow = (uint64_t)(a.row_begin + lrow);
        uint64_t u, d, s, ru, rd;
        kd_unrank(K, A, binom, grow, &u, &d, &s, &ru, &rd);
        const uint64_t cu = binom[K.n_sites * kKondoTab + K.nu0 + __popcll(s)];
        const uint64_t in_block = rd * cu + ru;
        d2 sum = {0.0, 0.0};
        const d2 dg = kd_row_terms(K, u, d, s, [&](uint64_t u2, uint64_t d2w, uint64_t s2, int code) {
            const int kind = code >> 12;
            uint64_t col;
            if (kind >= 2) {
                const uint64_t o = kind == 2 ? u : d, o2 = kind == 2 ? u2 : d2w;
                const uint64_t ends = o ^ o2;                              // the two sites of the hop
                const int lo = __ffsll((long long)ends) - 1, hi = 63 - __clzll((long long)ends);
                const uint64_t span = (2ULL << hi) - (1ULL << lo);         // sites lo .. hi
                const uint64_t dr = kd_rank_delta(binom, o & span, o2 & span, __popcll(o & ((1ULL << lo) - 1ULL)));
                col = grow + (kind == 2 ? dr : dr * cu);
            } else if (kind == 1) {
                col = kd_srank(A, s2) + in_block;
            } else {
                col = kd_rank(K, A, binom, u2, d2w, s2);
            }
            mf_gather_add<REALX>(a, sum, kd_value(K, code), (int64_t)col);
        });
        d2 yo, xi;
        mf_row_load<REALX>(a, lrow, grow, yo, xi);
        mf_row_finish(a, lrow, sum, dg.x, xi, yo, acc);                    // the diagonal is real by construction
    }
    mf_block_partials<kMfKondoBlock>(acc, red, a.partials);
}

// entries qbh_gen_kondo would store for rows [row_begin, row_end) (the diagonal always, zero amplitudes dropped elsewhere):
// what k_kondo_count counts, as one sum per workgroup
__global__ __launch_bounds__(256) void k_mf_kondo_count(const KondoDev *Kp, int64_t row_begin, int64_t row_end, unsigned long long *part)
{
    __shared__ uint64_t lds[kKondoTabWords];
    __shared__ unsigned long long red[256];
    const KondoDev &K = *Kp;
    kd_stage_tables(lds, K, 256);
    const uint64_t *A = lds, *binom = lds + kKondoTab * kKondoTab;
    unsigned long long c = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; row < row_end; row += stride) {
        uint64_t u, d, s, ru, rd;
        kd_unrank(K, A, binom, (uint64_t)row, &u, &d, &s, &ru, &rd);
        c += 1;
        kd_row_terms(K, u, d, s, [&](uint64_t, uint64_t, uint64_t, int) { ++c; });
    }
    red[threadIdx.x] = c;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

struct HipFree {
    std::vector<void *> p;
    ~HipFree() { for (void *q : p) (void)hipFree(q); }
};

}  // namespace

int launch_mf_kondo(const MfKondo &t, const MfVec &a, hipStream_t s, int *nparts_out)
{
    const int64_t nblk = (a.nrows + kMfKondoBlock - 1) / kMfKondoBlock;
    const int g = (int)std::min<int64_t>(nblk, std::min<int64_t>((int64_t)device_cu_count() * kMfKondoPerCu, kMaxRedBlocks));
    if (a.xr != nullptr) hipLaunchKernelGGL(k_mf_kondo<true>, dim3(g), dim3(kMfKondoBlock), 0, s, t, a);
    else                 hipLaunchKernelGGL(k_mf_kondo<false>, dim3(g), dim3(kMfKondoBlock), 0, s, t, a);
    QBH_HIP(hipGetLastError());
    if (nparts_out) *nparts_out = g;
    return QBH_OK;
}

int kondo_shape(const char *who, int n_sites, int n_elec, int two_sz, KondoDev &K)
{
    memset(&K, 0, sizeof(K));
    if (n_sites < 1 || n_sites > kKondoMaxSites) {
        set_error("%s: n_sites = %d outside [1, %d]", who, n_sites, kKondoMaxSites);
        return QBH_EINVAL;
    }
    if (n_elec < 0 || n_elec > 2 * n_sites) {
        set_error("%s: n_elec = %d outside [0, %d]", who, n_elec, 2 * n_sites);
        return QBH_EINVAL;
    }
    // two_sz = (n_up - n_dn) + (n - 2m) and n_up + n_dn = n_elec: 2 n_up = n_elec + two_sz - n + 2m
    if ((n_elec + two_sz - n_sites) % 2 != 0) {
        set_error("%s: no sector with n_elec = %d and two_sz = %d on %d sites (n_elec + two_sz - n_sites is odd)", who, n_elec, two_sz,
                  n_sites);
        return QBH_EINVAL;
    }
    K.n_sites = n_sites;
    K.n_elec = n_elec;
    K.two_sz = two_sz;
    K.nu0 = (n_elec + two_sz - n_sites) / 2;
    for (int p = 0; p < kKondoTab; ++p) {
        K.binom[p * kKondoTab] = 1;
        for (int k = 1; k <= p; ++k)
            K.binom[p * kKondoTab + k] = K.binom[(p - 1) * kKondoTab + k - 1] + (k <= p - 1 ? K.binom[(p - 1) * kKondoTab + k] : 0);
    }
    // blocks: 0 <= n_up(m) <= n and 0 <= n_dn(m) = n_elec - n_up(m) <= n
    K.m_lo = std::max(0, std::max(-K.nu0, n_elec - n_sites - K.nu0));
    K.m_hi = std::min(n_sites, std::min(n_sites - K.nu0, n_elec - K.nu0));
    std::vector<uint64_t> w((size_t)2 * kKondoTab, 0);
    for (int m = K.m_lo; m <= K.m_hi; ++m) {
        const int nu = K.nu0 + m;
        w[(size_t)m] = K.binom[n_sites * kKondoTab + nu] * K.binom[n_sites * kKondoTab + n_elec - nu];
        K.total += K.binom[n_sites * kKondoTab + m] * w[(size_t)m];         // < 2^63: the whole space has 2^(3n) words
    }
    for (int p = 0; p < kKondoTab; ++p)
        for (int c = 0; c < kKondoTab; ++c) {
            uint64_t a = 0;
            for (int j = 0; j <= p && c + j < kKondoTab; ++j) a += K.binom[p * kKondoTab + j] * w[(size_t)(c + j)];
            K.A[p * kKondoTab + c] = a;
        }
    if (K.total == 0) {
        set_error("%s: the sector n_elec = %d, two_sz = %d on %d sites is empty", who, n_elec, two_sz, n_sites);
        return QBH_EUNSUPP;
    }
    return QBH_OK;
}

int kondo_setup(const char *who, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites, const qbh_z *amp_up,
                const qbh_z *amp_dn, double U, const double *kz, const double *kxy, int n_sbonds, const int32_t *sbond_sites,
                const double *bz, const double *bxy, KondoDev &K, bool any_row_length)
{
    const int shape = kondo_shape(who, n_sites, n_elec, two_sz, K);
    if (shape != QBH_OK && shape != QBH_EUNSUPP) return shape;             // an empty sector is reported after the term checks
    if (n_terms < 0 || n_sbonds < 0 || (n_terms > 0 && (!term_sites || !amp_up || !amp_dn)) || !kz || !kxy ||
        (n_sbonds > 0 && (!sbond_sites || !bz || !bxy))) {
        set_error("%s: invalid term arrays", who);
        return QBH_EINVAL;
    }
    std::map<std::pair<int, int>, std::array<std::complex<double>, 2>> tmap;
    for (int t = 0; t < n_terms; ++t) {
        const int i = term_sites[2 * t], j = term_sites[2 * t + 1];
        if (i < 0 || i >= n_sites || j < 0 || j >= n_sites) {
            set_error("%s: term %d acts on a site outside the lattice", who, t);
            return QBH_EINVAL;
        }
        auto &a = tmap[{i, j}];
        a[0] += std::complex<double>(amp_up[t].re, amp_up[t].im);
        a[1] += std::complex<double>(amp_dn[t].re, amp_dn[t].im);
    }
    std::map<std::pair<int, int>, std::array<double, 2>> bmap;
    for (int e = 0; e < n_sbonds; ++e) {
        const int i = sbond_sites[2 * e], j = sbond_sites[2 * e + 1];
        if (i < 0 || i >= n_sites || j < 0 || j >= n_sites || i == j) {
            set_error("%s: local-spin bond %d needs two different sites of the lattice", who, e);
            return QBH_EINVAL;
        }
        auto &b = bmap[{std::min(i, j), std::max(i, j)}];
        b[0] += bz[e];
        b[1] += bxy[e];
    }
    const std::array<std::complex<double>, 2> none = {0.0, 0.0};
    std::map<std::pair<int, int>, int> pairs;
    for (const auto &kv : tmap) {
        const auto it = tmap.find({kv.first.second, kv.first.first});
        const auto &back = it == tmap.end() ? none : it->second;
        for (int sp = 0; sp < 2; ++sp)
            if (std::abs(kv.second[sp] - std::conj(back[sp])) > QBH_SPARSE_PRECISION) {
                set_error("%s: the merged %s terms on (%d, %d) and (%d, %d) are not Hermitian conjugates", who, sp ? "down" : "up",
                          kv.first.first, kv.first.second, kv.first.second, kv.first.first);
                return QBH_ENOTHERM;
            }
        if (kv.first.first != kv.first.second) pairs[{std::min(kv.first.first, kv.first.second), std::max(kv.first.first, kv.first.second)}] = 1;
    }
    // the longest row: one move per site pair and species, one Kondo flip per site, one exchange per local-spin bond, the diagonal
    int max_row = 1 + 2 * (int)pairs.size();
    for (int i = 0; i < n_sites; ++i) max_row += kxy[i] != 0.0 ? 1 : 0;
    for (const auto &kv : bmap) max_row += kv.second[1] != 0.0 ? 1 : 0;
    if ((max_row > kKondoMaxRow && !any_row_length) || (int)tmap.size() > kKondoMaxTerms || (int)bmap.size() > kKondoMaxSbonds) {
        set_error("%s: a row may hold %d entries; at most %d are supported", who, max_row, kKondoMaxRow);
        return QBH_EUNSUPP;
    }
    for (const auto &kv : tmap) {
        K.ti[K.n_terms] = (int8_t)kv.first.first;
        K.tj[K.n_terms] = (int8_t)kv.first.second;
        K.aup[K.n_terms][0] = kv.second[0].real();
        K.aup[K.n_terms][1] = kv.first.first == kv.first.second ? 0.0 : kv.second[0].imag();
        K.adn[K.n_terms][0] = kv.second[1].real();
        K.adn[K.n_terms][1] = kv.first.first == kv.first.second ? 0.0 : kv.second[1].imag();
        K.n_terms++;
    }
    for (const auto &kv : bmap) {
        K.bi[K.n_sbonds] = (int8_t)kv.first.first;
        K.bj[K.n_sbonds] = (int8_t)kv.first.second;
        K.bz[K.n_sbonds] = kv.second[0];
        K.bxy[K.n_sbonds] = kv.second[1];
        K.n_sbonds++;
    }
    K.U = U;
    for (int i = 0; i < n_sites; ++i) {
        K.kz[i] = kz[i];
        K.kxy[i] = kxy[i];
    }
    if (shape != QBH_OK) {
        set_error("%s: the sector n_elec = %d, two_sz = %d on %d sites is empty", who, n_elec, two_sz, n_sites);
        return shape;
    }
    return max_row;                                            // > 0: the row capacity the terms need
}

int kondo_invariant(const char *who, const KondoDev &K, int n_trans, const int32_t *perms)
{
    auto close = [](double x, double y) { return std::fabs(x - y) <= QBH_SPARSE_PRECISION * std::max(1.0, std::max(std::fabs(x), std::fabs(y))); };
    for (int g = 1; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * K.n_sites;
        for (int i = 0; i < K.n_sites; ++i)
            if (!close(K.kz[i], K.kz[pg[i]]) || !close(K.kxy[i], K.kxy[pg[i]])) {
                set_error("%s: the Kondo couplings are not invariant under translation %d: site %d and its image %d differ", who, g, i,
                          pg[i]);
                return QBH_EINVAL;
            }
        for (int t = 0; t < K.n_terms; ++t) {
            const int gi = pg[K.ti[t]], gj = pg[K.tj[t]];
            double img[4] = {0.0, 0.0, 0.0, 0.0};
            for (int q = 0; q < K.n_terms; ++q)
                if (K.ti[q] == gi && K.tj[q] == gj) {
                    img[0] = K.aup[q][0]; img[1] = K.aup[q][1]; img[2] = K.adn[q][0]; img[3] = K.adn[q][1];
                }
            if (!close(K.aup[t][0], img[0]) || !close(K.aup[t][1], img[1]) || !close(K.adn[t][0], img[2]) || !close(K.adn[t][1], img[3])) {
                set_error("%s: the terms are not invariant under translation %d: (%d, %d) and its image (%d, %d) differ", who, g,
                          (int)K.ti[t], (int)K.tj[t], gi, gj);
                return QBH_EINVAL;
            }
        }
        for (int e = 0; e < K.n_sbonds; ++e) {
            const int gi = std::min(pg[K.bi[e]], pg[K.bj[e]]), gj = std::max(pg[K.bi[e]], pg[K.bj[e]]);
            double iz = 0.0, ixy = 0.0;
            for (int q = 0; q < K.n_sbonds; ++q)
                if (K.bi[q] == gi && K.bj[q] == gj) {
                    iz = K.bz[q];
                    ixy = K.bxy[q];
                }
            if (!close(K.bz[e], iz) || !close(K.bxy[e], ixy)) {
                set_error("%s: the local-spin bonds are not invariant under translation %d: (%d, %d) and its image (%d, %d) differ", who,
                          g, (int)K.bi[e], (int)K.bj[e], gi, gj);
                return QBH_EINVAL;
            }
        }
    }
    return QBH_OK;
}

}  // namespace qbh

using qbh::d2;

#define QBH_KHIP(who, call)                                                                \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            qbh::set_error("%s: %s failed: %s", (who), #call, hipGetErrorString(_e));      \
            (void)hipGetLastError();                                                       \
            return _e == hipErrorOutOfMemory ? QBH_ENOMEM : QBH_EHIP;                      \
        }                                                                                  \
    } while (0)

extern "C" int qbh_gen_kondo(qbh_csr **out, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites,
                             const qbh_z *amp_up, const qbh_z *amp_dn, double U, const double *kz, const double *kxy, int n_sbonds,
                             const int32_t *sbond_sites, const double *bz, const double *bxy, int64_t row_begin, int64_t row_end,
                             int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    static const char *who = "qbh_gen_kondo";
    if (!out) {
        set_error("%s: out is NULL", who);
        return QBH_EINVAL;
    }
    std::vector<KondoDev> kk(1);
    KondoDev &K = kk[0];
    const int max_row = kondo_setup(who, n_sites, n_elec, two_sz, n_terms, term_sites, amp_up, amp_dn, U, kz, kxy, n_sbonds,
                                    sbond_sites, bz, bxy, K);
    if (max_row <= 0) return max_row;
    if (dim_out) *dim_out = (int64_t)K.total;
    if (K.total >= 2147483647ULL) {
        set_error("%s: dim %llu exceeds int32 columns", who, (unsigned long long)K.total);
        return QBH_EUNSUPP;
    }
    const int64_t dim = (int64_t)K.total;
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("%s: bad row range [%lld, %lld) of %lld", who, (long long)row_begin, (long long)row_end, (long long)dim);
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_KHIP(who, hipSetDevice(opts->device));

    HipFree pool;
    KondoDev *d_K = nullptr;
    QBH_KHIP(who, qbh::dev_alloc(&d_K, sizeof(KondoDev)));
    pool.p.push_back(d_K);
    QBH_KHIP(who, hipMemcpy(d_K, &K, sizeof(KondoDev), hipMemcpyHostToDevice));
    const int64_t nrows = row_end - row_begin;
    int32_t *d_cnt = nullptr;
    QBH_KHIP(who, qbh::dev_alloc(&d_cnt, (size_t)nrows * sizeof(int32_t)));
    pool.p.push_back(d_cnt);
    int64_t *d_ia = nullptr;
    QBH_KHIP(who, qbh::dev_alloc(&d_ia, (size_t)(nrows + 1) * sizeof(int64_t)));
    HipFree own;                                              // the CSR arrays until the handle adopts them
    own.p.push_back(d_ia);
    hipLaunchKernelGGL(k_kondo_count, dim3(blas_grid(nrows)), dim3(256), 0, 0, d_K, row_begin, row_end, d_cnt);
    QBH_KHIP(who, hipGetLastError());
    QBH_TRY(exclusive_scan(d_cnt, nrows, d_ia, 0));
    int64_t nnz = 0;
    QBH_KHIP(who, hipMemcpy(&nnz, d_ia + nrows, sizeof(int64_t), hipMemcpyDeviceToHost));
    int32_t *d_ja = nullptr;
    d2 *d_val = nullptr;
    QBH_KHIP(who, qbh::dev_alloc(&d_ja, (size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
    own.p.push_back(d_ja);
    QBH_KHIP(who, qbh::dev_alloc(&d_val, (size_t)std::max<int64_t>(nnz, 1) * sizeof(d2)));
    own.p.push_back(d_val);
    const size_t fill_lds = (size_t)kKondoTabWords * sizeof(uint64_t) + (size_t)kKondoFillBlock * max_row * 8;
    QBH_KHIP(who, hipFuncSetAttribute(reinterpret_cast<const void *>(k_kondo_fill), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)fill_lds));
    int64_t grid = (nrows + kKondoFillBlock - 1) / kKondoFillBlock;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(k_kondo_fill, dim3((unsigned)grid), dim3(kKondoFillBlock), fill_lds, 0, d_K, max_row, row_begin, row_end, d_ia,
                       d_ja, d_val);
    QBH_KHIP(who, hipGetLastError());
    QBH_KHIP(who, hipDeviceSynchronize());
    own.p.clear();                                            // ownership passes with the call (freed by it on failure)
    qbh_opts og;
    opts_generated(opts, &og);
    return qbh_csr_create_device(out, nrows, dim, row_begin, nnz, d_ia, d_ja, reinterpret_cast<qbh_z *>(d_val), 1, &og);
}

extern "C" int qbh_mf_kondo(qbh_csr **out, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites,
                            const qbh_z *amp_up, const qbh_z *amp_dn, double U, const double *kz, const double *kxy, int n_sbonds,
                            const int32_t *sbond_sites, const double *bz, const double *bxy, int64_t row_begin, int64_t row_end,
                            int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    static const char *who = "qbh_mf_kondo";
    if (!out) {
        set_error("%s: out is NULL", who);
        return QBH_EINVAL;
    }
    std::vector<KondoDev> kk(1);
    KondoDev &K = kk[0];
    const int max_row = kondo_setup(who, n_sites, n_elec, two_sz, n_terms, term_sites, amp_up, amp_dn, U, kz, kxy, n_sbonds,
                                    sbond_sites, bz, bxy, K, true);       // no row is staged: any row length
    if (max_row <= 0) return max_row;
    if (dim_out) *dim_out = (int64_t)K.total;                 // < 2^63: rows, ranks and rank differences are 64-bit
    const int64_t dim = (int64_t)K.total;
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("%s: bad row range [%lld, %lld) of %lld", who, (long long)row_begin, (long long)row_end, (long long)dim);
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_KHIP(who, hipSetDevice(opts->device));

    bool values_real = true;                                  // kxy, bxy and the diagonal are real by construction
    for (int t = 0; t < K.n_terms; ++t)
        if (K.aup[t][1] != 0.0 || K.adn[t][1] != 0.0) values_real = false;
    HipFree pool;
    MfKondo t;
    QBH_KHIP(who, qbh::dev_alloc(&t.K, sizeof(KondoDev)));
    pool.p.push_back(t.K);
    QBH_KHIP(who, hipMemcpy(t.K, &K, sizeof(KondoDev), hipMemcpyHostToDevice));

    const int64_t nrows = row_end - row_begin;
    const int cgrid = blas_grid(nrows);
    unsigned long long *d_part = nullptr;
    QBH_KHIP(who, qbh::dev_alloc(&d_part, (size_t)cgrid * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_mf_kondo_count, dim3(cgrid), dim3(256), 0, 0, t.K, row_begin, row_end, d_part);
    std::vector<unsigned long long> part((size_t)cgrid);
    hipError_t ce = hipGetLastError();
    if (ce == hipSuccess) ce = hipMemcpy(part.data(), d_part, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d_part);
    QBH_KHIP(who, ce);
    int64_t nnz = 0;
    for (unsigned long long v : part) nnz += (int64_t)v;

    const int rc = adopt_mf(out, 5, &qbh_csr::mfk, t, pool.p, (int64_t)sizeof(KondoDev), values_real, nrows, dim, row_begin, nnz, opts);
    if (rc == QBH_OK) pool.p.clear();                         // the handle owns the tables now
    return rc;
}
