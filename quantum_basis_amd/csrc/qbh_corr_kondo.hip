// qbh_corr_kondo.hip -- all-pair static correlations of a resident state of the Kondo lattice (conduction electrons plus a local
// spin-1/2 on every site; the sector (n_elec, two_sz) of qbh_gen_kondo / qbh_mf_kondo) in one pass over it: qbh_corr_kondo_dev.
// A launch is a grid of (row blocks) x (passes); a pass owns a fixed group of pairs or sites and a per-lane accumulator array
// indexed by compile-time constants only.  The block reduction, the launch with its second stage
// (corr_reduce_launch), the pass layout (CorrPasses) and the shared fills and checks are those of qbh_corr.hpp.  No atomics.
//
// One kernel instance per pass kind (a kind has registers of its own), one launch per kind that is asked for:
//   DIAG  no gather, 32 accumulators; the pass's sub-kind is uniform over the workgroup:
//           SITE  5 sites:  [6g .. 6g+5] = n_up, n_dn, n_up n_dn, S^z, S^z n_up, S^z n_dn of site g;  [30] = sum |psi|^2
//           NN    8 pairs i < j:  [4g .. 4g+3] = n_{i,up} n_{j,up}, n_{i,up} n_{j,dn}, n_{i,dn} n_{j,up}, n_{i,dn} n_{j,dn}
//           ZN    8 pairs i < j:  [4g .. 4g+3] = S^z_i n_{j,up}, S^z_i n_{j,dn}, S^z_j n_{i,up}, S^z_j n_{i,dn}
//           ZZ    32 pairs i < j: [g] = sum |psi|^2 [local spins i and j differ]           (zz = (norm2 - 2 D) / 4 on the host)
//   HOP / EE / LL  16 pairs i < j, LE 16 ordered pairs (i, j), the diagonal included:  [g] re, [16+g] im (complex vector only) of
//         sum_w conj(psi(w')) sign psi(w), one gather per hit:
//           HOP  c+_{i,sp} c_j,sp}: j occupied and i empty in the species (uniform per pass), sign = parity of the species'
//                particles between; w' = row + (rank' - rank) of the species over the sites i .. j (kd_rank_delta), times
//                C(n, n_up) for the down species -- the column of k_mf_kondo
//           EE   s^+_i s^-_j = c+_{i,up} c_{i,dn} c+_{j,dn} c_{j,up}: up moves j -> i, down moves i -> j, both differences at
//                once, the row's block stays; sign = -(-1)^(particles of both species between)
//           LL   S^+_i S^-_j: local spin i down, j up; w' = row + (kd_srank(s') - kd_srank(s)), the difference walks the down
//                spins between the two sites only (their count of down spins above grows by one); no sign
//           LE   S^+_i s^-_j: local spin i down, electron j up alone; the target lies in the block popcount(s) - 1, n_up - 1:
//                kd_rank of all three fields; sign of s^-_j as in KondoSiteOp (op 5)
// Rows: tiles of 256 x kKcRows consecutive rows (the scheme: qbh_corr.hpp); a lane unranks one row (kd_unrank: a dependent LDS walk and a
// 64-bit division) and steps to the next words with kc_next.  kKcRows = 1 is re-unranking every row in every pass: 40 % slower
// for the whole call at 10 sites.
#include <algorithm>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_device.hpp"
#include "qbh_gen_util.hpp"
#include "qbh_kondo.hpp"
#include "qbh_kondo_lds.hpp"                                 // krepr_stage: A and binom into LDS
#include "qbh_corr.hpp"

namespace qbh {
namespace {

constexpr int kKcGroup = 16;             // pairs of a gathered pass
constexpr int kKcItems = 32;             // descriptors of a pass (gathered kinds use 16, SITE 5, NN and ZN 8, ZZ 32)
constexpr int kKcRows = 8;               // rows per lane and tile (measured at 10 sites: 1: 43.9 ms, 2: 38.8, 4: 33.6, 8: 31.3)
constexpr int kKcSites = 5, kKcQuads = 8;
enum { kKcDiag = 0, kKcHop = 1, kKcEE = 2, kKcLL = 3, kKcLE = 4, kKcKinds = 5 };
enum { kKcSite = 0, kKcNN = 1, kKcZN = 2, kKcZZ = 3, kKcSubs = 4 };
constexpr uint32_t kKcValid = 1u << 31;  // item: i | j << 8 | sub << 16 | valid; sub = the DIAG sub-kind, or the species of a HOP pass

struct CorrKondo {
    int n_sites, n_elec, nu0, m_lo, m_hi;
    int64_t dim;
    const KondoDev *K;                   // shape and counting tables (no terms)
    const uint32_t *item;                // [gridDim.y * kKcItems]: this launch's passes
    const d2 *xg;                        // exactly one of xg / xr
    const double *xr;
    double *partials;
};

template <bool REALX, int KIND>
constexpr int kc_acc() { return KIND == kKcDiag ? 32 : (REALX ? 1 : 2) * kKcGroup; }

constexpr size_t kCorrKondoLds = ((size_t)2 * kKondoTabEntries + (size_t)kCorrBlock * (kKcRows + 1)) * 8;
static_assert(kCorrKondoLds <= kCorrLdsCap, "the counting tables and one tile of words fit LDS for every shape");

// the next larger pattern with as many bits (c != 0 and not the last pattern)
__device__ __forceinline__ uint32_t kc_next_comb(uint32_t c)
{
    const uint32_t t = c | (c - 1u);
    return (t + 1u) | ((((~t & (t + 1u)) - 1u) >> (__ffs((int)c) - 1)) >> 1);
}

// the sector's next word: u runs fastest, then d, then s over the patterns with m_lo <= popcount <= m_hi, ascending; a new s
// starts with the lowest patterns of its own n_up, n_dn.  Past the last word the result is unused.
__device__ __forceinline__ void kc_next(const CorrKondo &t, uint32_t &u, uint32_t &d, uint32_t &s)
{
    const int n = t.n_sites, nu = t.nu0 + __popc(s), nd = t.n_elec - nu;
    if (u != ((1u << nu) - 1u) << (n - nu)) {
        u = kc_next_comb(u);
        return;
    }
    u = (1u << nu) - 1u;
    if (d != ((1u << nd) - 1u) << (n - nd)) {
        d = kc_next_comb(d);
        return;
    }
    // the smallest v > s with popcount in [m_lo, m_hi]: too many bits -> carry out of the lowest one (nothing between has
    // fewer); too few -> fill the lowest clear bits.  At most n steps of each.
    uint32_t v = s + 1u;
    for (int step = 0; step < 2 * kKondoMaxSites + 2; ++step) {
        const int pc = __popc(v);
        if (pc > t.m_hi) v += v & (0u - v);
        else if (pc < t.m_lo) v |= v + 1u;
        else break;
    }
    s = v;
    const int nu2 = (t.nu0 + __popc(v)) & 31, nd2 = (t.n_elec - nu2) & 31;
    u = (1u << nu2) - 1u;
    d = (1u << nd2) - 1u;
}

// kd_srank(to) - kd_srank(from) (mod 2^64) of two s patterns with the same popcount that stand below c0 set bits
__device__ __forceinline__ uint64_t kc_srank_delta(const uint64_t *A, uint32_t from, uint32_t to, int c0)
{
    uint64_t r = 0;
    for (int c = c0; to; ++c) {
        const int p2 = 31 - __clz((int)to), p1 = 31 - __clz((int)from);
        to ^= 1u << p2;
        from ^= 1u << p1;
        r += A[p2 * kKondoTab + c] - A[p1 * kKondoTab + c];
    }
    return r;
}

template <bool REALX, int KIND>
__global__ __launch_bounds__(kCorrBlock) void k_corr_kondo(CorrKondo t)
{
    constexpr int G = kKcGroup, NA = kc_acc<REALX, KIND>(), R = kKcRows;
    extern __shared__ __attribute__((aligned(16))) unsigned long long kc_lds[];
    __shared__ double red[NA * (kCorrBlock / 64)];
    const KondoDev &K = *t.K;
    const int tid = threadIdx.x, pass = blockIdx.y, n = t.n_sites;
    const uint64_t *tab, *A, *binom;
    krepr_stage(nullptr, 0, K, reinterpret_cast<uint64_t *>(kc_lds), kCorrBlock, tab, A, binom);
    uint64_t *stage = reinterpret_cast<uint64_t *>(kc_lds) + 2 * kKondoTabEntries;        // [kCorrBlock * (R + 1)]
    uint32_t it[kKcItems];                                                // this pass's pairs or sites: scalar registers
#pragma unroll
    for (int g = 0; g < kKcItems; ++g) it[g] = corr_uniform(t.item[(size_t)pass * kKcItems + g]);
    const uint32_t sub = (it[0] >> 16) & 7u, fm = (1u << n) - 1u;
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int64_t tile_rows = (int64_t)kCorrBlock * R, n_tiles = (t.dim + tile_rows - 1) / tile_rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t base = tile * tile_rows;
      __syncthreads();                               // the last tile's words have been read
      if (base + (int64_t)tid * R < t.dim) {
          uint64_t u64, d64, s64, ru, rd;
          kd_unrank(K, A, binom, (uint64_t)(base + (int64_t)tid * R), &u64, &d64, &s64, &ru, &rd);
          uint32_t u = (uint32_t)u64, d = (uint32_t)d64, s = (uint32_t)s64;
#pragma unroll 1
          for (int q = 0; q < R; ++q) {
              stage[tid * (R + 1) + q] = (uint64_t)u | ((uint64_t)d << n) | ((uint64_t)s << (2 * n));
              if (q + 1 < R) kc_next(t, u, d, s);
          }
      }
      __syncthreads();
#pragma unroll 1
      for (int q = 0; q < R; ++q) {
        const int local = q * kCorrBlock + tid;                           // made by lane local / R at its step local % R
        const int64_t row = base + local;
        if (row >= t.dim) break;
        const uint64_t word = stage[(local / R) * (R + 1) + local % R];
        const uint32_t u = (uint32_t)word & fm, d = (uint32_t)(word >> n) & fm, s = (uint32_t)(word >> (2 * n));
        const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
        if (KIND == kKcDiag) {
            const double w = fma(x.x, x.x, x.y * x.y);
            if (sub == kKcSite) {
#pragma unroll
                for (int g = 0; g < kKcSites; ++g) {
                    const uint32_t e = it[g];
                    if (e & kKcValid) {
                        const int i = (int)(e & 255u);
                        const bool bu = (u >> i) & 1u, bd = (d >> i) & 1u;
                        const double z = ((s >> i) & 1u) ? -0.5 * w : 0.5 * w;
                        acc[6 * g + 0] += bu ? w : 0.0;
                        acc[6 * g + 1] += bd ? w : 0.0;
                        acc[6 * g + 2] += (bu && bd) ? w : 0.0;
                        acc[6 * g + 3] += z;
                        acc[6 * g + 4] += bu ? z : 0.0;
                        acc[6 * g + 5] += bd ? z : 0.0;
                    }
                }
                acc[30] += w;
            } else if (sub == kKcNN) {
#pragma unroll
                for (int g = 0; g < kKcQuads; ++g) {
                    const uint32_t e = it[g];
                    if (e & kKcValid) {
                        const int i = (int)(e & 255u), j = (int)((e >> 8) & 255u);
                        const bool ui = (u >> i) & 1u, uj = (u >> j) & 1u, di = (d >> i) & 1u, dj = (d >> j) & 1u;
                        acc[4 * g + 0] += (ui && uj) ? w : 0.0;
                        acc[4 * g + 1] += (ui && dj) ? w : 0.0;
                        acc[4 * g + 2] += (di && uj) ? w : 0.0;
                        acc[4 * g + 3] += (di && dj) ? w : 0.0;
                    }
                }
            } else if (sub == kKcZN) {
#pragma unroll
                for (int g = 0; g < kKcQuads; ++g) {
                    const uint32_t e = it[g];
                    if (e & kKcValid) {
                        const int i = (int)(e & 255u), j = (int)((e >> 8) & 255u);
                        const double zi = ((s >> i) & 1u) ? -0.5 * w : 0.5 * w, zj = ((s >> j) & 1u) ? -0.5 * w : 0.5 * w;
                        acc[4 * g + 0] += ((u >> j) & 1u) ? zi : 0.0;
                        acc[4 * g + 1] += ((d >> j) & 1u) ? zi : 0.0;
                        acc[4 * g + 2] += ((u >> i) & 1u) ? zj : 0.0;
                        acc[4 * g + 3] += ((d >> i) & 1u) ? zj : 0.0;
                    }
                }
            } else {
#pragma unroll
                for (int g = 0; g < kKcItems; ++g) {
                    const uint32_t e = it[g];
                    if (e & kKcValid) acc[g] += (((s >> (e & 255u)) ^ (s >> ((e >> 8) & 255u))) & 1u) ? w : 0.0;
                }
            }
            continue;
        }
        const int m = __popc(s);
        const uint64_t cu = binom[n * kKondoTab + t.nu0 + m];              // C(n, n_up) of the row's block
#pragma unroll
        for (int g0 = 0; g0 < G; g0 += 8) {
            uint64_t idx[8];
            bool hits[8], neg[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const uint32_t e = it[g0 + jj];
                hits[jj] = false;
                neg[jj] = false;
                idx[jj] = 0;                           // read under hits[jj] only
                if (e & kKcValid) {                    // uniform; padding items close the last pass
                    const int i = (int)(e & 255u), j = (int)((e >> 8) & 255u);
                    const uint32_t bi = 1u << i, bj = 1u << j;
                    const uint32_t span = (2u << j) - bi, btw = span & ~(bi | bj);        // i < j except in LE, which uses neither
                    if (KIND == kKcHop) {
                        const bool dn = (e >> 16) & 1u;
                        const uint32_t o = dn ? d : u;
                        if ((o & bj) && !(o & bi)) {
                            const uint64_t dr = kd_rank_delta(binom, o & span, (o ^ bi ^ bj) & span, __popc(o & (bi - 1u)));
                            hits[jj] = true;
                            neg[jj] = __popc(o & btw) & 1;
                            idx[jj] = (uint64_t)row + (dn ? dr * cu : dr);
                        }
                    } else if (KIND == kKcEE) {
                        if ((u & bj) && !(d & bj) && (d & bi) && !(u & bi)) {
                            const uint64_t du = kd_rank_delta(binom, u & span, (u ^ bi ^ bj) & span, __popc(u & (bi - 1u)));
                            const uint64_t dd = kd_rank_delta(binom, d & span, (d ^ bi ^ bj) & span, __popc(d & (bi - 1u)));
                            hits[jj] = true;
                            neg[jj] = !(__popc((u ^ d) & btw) & 1);
                            idx[jj] = (uint64_t)row + du + dd * cu;
                        }
                    } else if (KIND == kKcLL) {
                        if ((s & bi) && !(s & bj)) {
                            hits[jj] = true;
                            idx[jj] = (uint64_t)row + kc_srank_delta(A, s & span, (s ^ bi ^ bj) & span, __popc(s >> (j + 1)));
                        }
                    } else {
                        if ((s & bi) && (u & bj) && !(d & bj)) {
                            hits[jj] = true;
                            neg[jj] = (__popc(u & (bj - 1u)) + __popc(d & (bj - 1u)) + t.nu0 + m - 1) & 1;
                            idx[jj] = kd_rank(K, A, binom, (uint64_t)(u ^ bj), (uint64_t)(d ^ bj), (uint64_t)(s ^ bi));
                        }
                    }
                }
            }
            // only the lanes with a hit load and accumulate: no line is fetched for a lane that adds nothing
            if (REALX) {
                double xv[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                    if (hits[jj]) xv[jj] = t.xr[idx[jj]];             // xv[jj] is written and read under hits[jj] only
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                    if (hits[jj]) {
                        const double v = xv[jj] * x.x;
                        acc[g0 + jj] += neg[jj] ? -v : v;
                    }
            } else {
                d2 xv[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                    if (hits[jj]) xv[jj] = t.xg[idx[jj]];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj)
                    if (hits[jj]) {
                        const double re = fma(xv[jj].x, x.x, xv[jj].y * x.y), im = xv[jj].x * x.y - xv[jj].y * x.x;
                        acc[g0 + jj] += neg[jj] ? -re : re;
                        acc[(NA - G) + g0 + jj] += neg[jj] ? -im : im;
                    }
            }
        }
      }
    }
    corr_block_partials<NA>(acc, red, t.partials);
}

template <int KIND>
void (*kc_kernel(bool rx))(CorrKondo)
{
    return rx ? k_corr_kondo<true, KIND> : k_corr_kondo<false, KIND>;
}

// comp[kind]: the sums of the kind's passes in pass order (empty for a kind that was not asked for); dp: the sub-kinds of the
// DIAG launch, hp: the two species of the HOP launch
int corr_kondo_run(const char *who, const KondoDev &K, const d2 *xg, const double *xr, const bool want_sub[kKcSubs],
                   const bool want_kind[kKcKinds], std::vector<double> comp[kKcKinds], CorrPasses &dp, CorrPasses &hp, hipStream_t s,
                   std::vector<void *> &pool)
{
    const int N = K.n_sites, n_pairs = N * (N - 1) / 2;
    std::vector<uint32_t> item[kKcKinds];
    auto close_pass = [](std::vector<uint32_t> &v) { v.resize((v.size() + kKcItems - 1) / kKcItems * kKcItems, 0u); };
    auto pairs = [&](std::vector<uint32_t> &v, int per_pass, uint32_t sub) {
        int k = 0;
        for (int i = 0; i < N; ++i)
            for (int j = i + 1; j < N; ++j) {
                v.push_back(kKcValid | (uint32_t)i | ((uint32_t)j << 8) | (sub << 16));
                if (++k % per_pass == 0) close_pass(v);
            }
        close_pass(v);
    };
    {
        std::vector<uint32_t> &v = item[kKcDiag];
        const int per[kKcSubs] = {kKcSites, kKcQuads, kKcQuads, kKcItems};
        for (int sub = 0; sub < kKcSubs; ++sub) {
            dp.add(sub, sub == kKcSite ? N : want_sub[sub] ? n_pairs : 0, per[sub]);
            if (sub == kKcSite) {
                for (int i = 0; i < N; ++i) {
                    v.push_back(kKcValid | (uint32_t)i | ((uint32_t)sub << 16));
                    if ((i + 1) % kKcSites == 0) close_pass(v);
                }
                close_pass(v);
            } else if (want_sub[sub]) {
                pairs(v, per[sub], (uint32_t)sub);
            }
        }
    }
    if (want_kind[kKcHop])
        for (int species = 0; species < 2; ++species) {
            hp.add(species, n_pairs, kKcGroup);
            pairs(item[kKcHop], kKcGroup, (uint32_t)species);
        }
    if ((int)(item[kKcDiag].size() / kKcItems) != dp.n_pass || (int)(item[kKcHop].size() / kKcItems) != hp.n_pass) {
        set_error("%s: internal: the pass layout and the item lists disagree", who);
        return QBH_EHIP;
    }
    if (want_kind[kKcEE]) pairs(item[kKcEE], kKcGroup, 0u);
    if (want_kind[kKcLL]) pairs(item[kKcLL], kKcGroup, 0u);
    if (want_kind[kKcLE]) {
        std::vector<uint32_t> &v = item[kKcLE];
        for (int q = 0; q < N * N; ++q) {
            v.push_back(kKcValid | (uint32_t)(q / N) | ((uint32_t)(q % N) << 8));
            if ((q + 1) % kKcGroup == 0) close_pass(v);
        }
        close_pass(v);
    }
    CorrKondo t{};
    t.n_sites = N;
    t.n_elec = K.n_elec;
    t.nu0 = K.nu0;
    t.m_lo = K.m_lo;
    t.m_hi = K.m_hi;
    t.dim = (int64_t)K.total;
    t.xg = xg;
    t.xr = xr;
    KondoDev *d_K = nullptr;
    QBH_TRY(upload(std::vector<KondoDev>(1, K), &d_K, pool));
    t.K = d_K;
    const bool rx = xr != nullptr;
    const int gx = corr_grid(t.dim, kCorrKondoLds, kCorrBlock * kKcRows);
    for (int k = 0; k < kKcKinds; ++k) {
        comp[k].clear();
        const int n_pass = (int)(item[k].size() / kKcItems);
        if (n_pass == 0) continue;
        const int NA = k == kKcDiag ? 32 : (rx ? 1 : 2) * kKcGroup;
        uint32_t *d_item = nullptr;
        QBH_TRY(upload(item[k], &d_item, pool));
        t.item = d_item;
        void (*kernel)(CorrKondo) = k == kKcDiag ? kc_kernel<kKcDiag>(rx) : k == kKcHop ? kc_kernel<kKcHop>(rx) : k == kKcEE ? kc_kernel<kKcEE>(rx)
                             : k == kKcLL ? kc_kernel<kKcLL>(rx) : kc_kernel<kKcLE>(rx);
        QBH_TRY(corr_reduce_launch(who, kernel, gx, n_pass, NA, kCorrBlock, kCorrKondoLds, s, t, nullptr, pool, comp[k]));
    }
    return QBH_OK;
}

}  // namespace
}  // namespace qbh

extern "C" int qbh_corr_kondo_dev(int n_sites, int n_elec, int two_sz, const qbh_z *d_vec, const double *d_vec_re, double *norm2,
                                  double *site, double *nn, double *zn, double *zz, qbh_z *hop, qbh_z *ee, qbh_z *ll, qbh_z *le, void *stream)
{
    using namespace qbh;
    static const char *who = "qbh_corr_kondo_dev";
    std::vector<KondoDev> Kv(1);
    KondoDev &K = Kv[0];
    QBH_TRY(kondo_shape(who, n_sites, n_elec, two_sz, K));         // the shape (QBH_EINVAL), then an empty sector (QBH_EUNSUPP)
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    QBH_TRY(corr_check_norm2(who, norm2));
    QBH_TRY(corr_check_device());
    const int N = n_sites, G = kKcGroup;
    const size_t NN = (size_t)N * N;
    const bool want_sub[kKcSubs] = {true, nn != nullptr, zn != nullptr, zz != nullptr};
    const bool want_kind[kKcKinds] = {true, hop != nullptr, ee != nullptr, ll != nullptr, le != nullptr};
    std::vector<void *> pool;
    std::vector<double> comp[kKcKinds];
    CorrPasses dp, hp;
    const CorrPasses lone;                                         // the layout of a launch of one kind: its passes begin at 0
    const int rc = corr_kondo_run(who, K, reinterpret_cast<const d2 *>(d_vec), d_vec_re, want_sub, want_kind, comp, dp, hp,
                                  (hipStream_t)stream, pool);
    free_pool(pool);
    if (rc != QBH_OK) return rc;
    const bool rx = d_vec_re != nullptr;
    const int NG = (rx ? 1 : 2) * G;                               // accumulators of a gathered pass
    auto diag = [&](int sub, int item, int per_pass, int per_item, int slot) {
        return dp.at_item(comp[kKcDiag], sub, item, per_pass, per_item, slot, 32);
    };
    auto site_v = [&](int i, int c) { return diag(kKcSite, i, kKcSites, 6, c); };
    // part: the species in the HOP launch (layout hp), 0 in the launches of one kind (layout lone)
    auto gathered = [&](const CorrPasses &lay, int kind, int part, int q) {
        return qbh_z{lay.at(comp[kind], part, q, G, 0, NG), rx ? 0.0 : lay.at(comp[kind], part, q, G, 1, NG)};
    };
    const double n2 = site_v(0, 30);
    *norm2 = n2;
    int q = 0;
    for (int i = 0; i < N; ++i) {
        const size_t ii = (size_t)i * N + i;
        const double nu = site_v(i, 0), nd = site_v(i, 1), docc = site_v(i, 2), sz = site_v(i, 3);
        if (site) {
            site[0 * N + i] = nu;
            site[1 * N + i] = nd;
            site[2 * N + i] = docc;
            site[3 * N + i] = sz;
        }
        if (nn) corr_put_nn_diag(nn, N, i, nu, docc, nd);
        if (zn) {
            zn[0 * NN + ii] = site_v(i, 4);
            zn[1 * NN + ii] = site_v(i, 5);
        }
        if (zz) zz[ii] = 0.25 * n2;
        corr_put_onsite_diag(hop, ee, N, i, nu, nd, docc);
        if (ll) ll[ii] = qbh_z{0.5 * n2 + sz, 0.0};
        for (int j = i + 1; j < N; ++j, ++q) {
            const size_t ij = (size_t)i * N + j, ji = (size_t)j * N + i;
            auto quad = [&](int sub, int c) { return diag(sub, q, kKcQuads, 4, c); };
            if (nn) corr_put_nn_pair(nn, N, i, j, quad(kKcNN, 0), quad(kKcNN, 1), quad(kKcNN, 2), quad(kKcNN, 3));
            if (zn) {
                zn[0 * NN + ij] = quad(kKcZN, 0);
                zn[1 * NN + ij] = quad(kKcZN, 1);
                zn[0 * NN + ji] = quad(kKcZN, 2);
                zn[1 * NN + ji] = quad(kKcZN, 3);
            }
            if (zz) zz[ij] = zz[ji] = corr_zz_pair(n2, dp.at(comp[kKcDiag], kKcZZ, q, kKcItems, 0, 32));
            auto herm = [&](qbh_z *out, const CorrPasses &lay, int kind, int part) {
                const qbh_z v = gathered(lay, kind, part, q);
                corr_put_herm(out, N, i, j, v.re, v.im);
            };
            if (hop) {
                herm(hop, hp, kKcHop, 0);
                herm(hop + NN, hp, kKcHop, 1);
            }
            if (ee) herm(ee, lone, kKcEE, 0);
            if (ll) herm(ll, lone, kKcLL, 0);
        }
    }
    if (le)
        for (int k = 0; k < N * N; ++k) le[k] = gathered(lone, kKcLE, 0, k);
    return QBH_OK;
}
