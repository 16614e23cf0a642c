// qbh_corr_qudit.hip -- all-pair static correlations of a resident state of d-level sites (the sector `total` of qbh_gen_qudit)
// in one pass over it: qbh_corr_qudit_dev.  A launch is a grid of (row blocks) x (passes); a pass owns a fixed group of pairs or
// sites and a per-lane accumulator array indexed by compile-time constants only.  The block
// reduction, the launch with its second stage (corr_reduce_launch), the pass layout (CorrPasses) and the shared fills and checks
// are those of qbh_corr.hpp.  No atomics.
//
// Pass kinds (NA = 32 accumulators for a packed-real vector, 48 for a complex one; the diagonal kinds use the first 32):
//   PAIR  16 pairs i < j, consecutive in the order (0,1) (0,2) .. (0,N-1) (1,2) ..:
//           [g]            str_ij = sum |psi|^2 h(l_i) prod_{i<k<j} g(l_k) h(l_j)                               no gather
//           [16+g] [32+g]  aa_ij  = sum_{l_i >= 1, l_j <= d-2} conj(psi(w')) psi(w) lower[l_i] lower[l_j + 1]    one gather
//         Both walk j upwards for a fixed i, so the string product and the rank difference of the move (l_i - 1, l_j + 1) are
//         RUNNING values: going from (i, j) to (i, j + 1) multiplies the product by g(l_j) and adds site j's term to the
//         difference.  The difference is the one of qd_move_delta for nj = lj + 1: every charge Q_t, i <= t < j, shifts by -1,
//             target = row + (c_j[Q_j - l_j] - c_j[Q_j - l_j - 1]) + sum_{i<t<j} D_t + (c_i[Q_i - 1] - c_i[Q_i]),
//             D_t = (c_t[Q_t - 1] - c_t[Q_t - 1 - l_t]) - (c_t[Q_t] - c_t[Q_t - l_t]),
//         so a pair costs four reads of the counting table whatever j - i is (qd_move_delta walks j - i sites), and site j's
//         four values serve both its own term and D_j.  The table is stored with one more column in front, c[-1] = 0, so that
//         Q - 1 - l >= -1 needs no clamp in rows that do not hit.
//   DD    8 quads (i < j; a0, b0 in {0, 2}):  [4q + 2u + v] = sum |psi|^2 f_{a0+u}(l_i) f_{b0+v}(l_j): four table reads serve four
//         accumulators.  K = n_diag is rounded up to an even number with zero tables; K = 2 takes one quad per pair.
//   SITE  32 items: [0] of the first pass = sum |psi|^2, the others sum |psi|^2 [l_s = l] (compare and select, no table).
// Rows: tiles of 256 x 4 consecutive rows (the scheme: qbh_corr.hpp); a lane unranks one row (qd_unrank: a dependent LDS walk per site)
// and steps to the next three words with qd_next.
#include <algorithm>
#include <cmath>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_device.hpp"
#include "qbh_gen_util.hpp"
#include "qbh_qudit.hpp"
#include "qbh_corr.hpp"

namespace qbh {
namespace {

constexpr int kQcGroup = 16;             // pairs of a PAIR pass
constexpr int kQcItems = 32;             // descriptors of a pass (PAIR uses 16, DD 8)
constexpr int kQcRows = 4;               // rows per lane and tile
constexpr int kQcTabStride = 8;          // entries per operator table (d <= 8)
enum { kQcEnd = 0, kQcMid = 1, kQcLow = 2, kQcUp = 3, kQcDiag = 4, kQcTables = 8 };       // tab[T * 8 + l]
enum { kQcPair = 0, kQcDD = 1, kQcSite = 2 };
constexpr uint32_t kQcValid = 1u << 31, kQcNewI = 1u << 12;

struct CorrQudit {
    int n_sites, d, bits, total, tw, want_str, want_aa;
    int64_t dim;
    const uint64_t *cum;                 // [n_sites * (tw + 1)]: column 0 holds 0 (charge -1), column q + 1 = cum[s][q]
    const double *tab;                   // [kQcTables * 8]
    const uint32_t *item;                // [gridDim.y * kQcItems]: this launch's passes
    const d2 *xg;                        // exactly one of xg / xr
    const double *xr;
    double *partials;
};

template <bool REALX>
constexpr int qc_acc() { return (REALX ? 2 : 3) * kQcGroup; }

inline size_t corr_qudit_lds(int n_sites, int total)
{
    return ((size_t)n_sites * (total + 2) + kQcTables * kQcTabStride + (size_t)kCorrBlock * (kQcRows + 1)) * 8;
}

template <bool REALX, int KIND>
__global__ __launch_bounds__(kCorrBlock) void k_corr_qudit(CorrQudit t)
{
    constexpr int G = kQcGroup, NA = qc_acc<REALX>(), R = kQcRows, kind = KIND;
    extern __shared__ __attribute__((aligned(16))) unsigned long long qc_lds[];
    __shared__ double red[NA * (kCorrBlock / 64)];
    const int tid = threadIdx.x, pass = blockIdx.y;
    const int d = t.d, bits = t.bits, tws = t.tw + 1, ncum = t.n_sites * tws;
    uint64_t *cum = reinterpret_cast<uint64_t *>(qc_lds);                 // [n_sites * tws]
    double *tab = reinterpret_cast<double *>(cum + ncum);                 // [kQcTables * 8]
    uint64_t *stage = reinterpret_cast<uint64_t *>(tab + kQcTables * kQcTabStride);       // [kCorrBlock * (R + 1)]
    for (int k = tid; k < ncum; k += kCorrBlock) cum[k] = t.cum[k];
    if (tid < kQcTables * kQcTabStride) tab[tid] = t.tab[tid];
    uint32_t it[kQcItems];                                                // this pass's pairs, quads or items: scalar registers
#pragma unroll
    for (int g = 0; g < kQcItems; ++g) it[g] = corr_uniform(t.item[(size_t)pass * kQcItems + g]);
    const bool want_str = t.want_str != 0, want_aa = t.want_aa != 0;
    const uint32_t lm = (1u << bits) - 1u;
    const uint64_t *cum1 = cum + 1;                                       // cum1[s * tws + q], q >= -1
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int64_t tile_rows = (int64_t)kCorrBlock * R, n_tiles = (t.dim + tile_rows - 1) / tile_rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t base = tile * tile_rows;
      __syncthreads();                               // the tables are in place; the last tile's words have been read
      if (base + (int64_t)tid * R < t.dim) {
          uint64_t w = qd_unrank(cum1, t.n_sites, d, bits, tws, t.total, (uint64_t)(base + (int64_t)tid * R));
#pragma unroll 1
          for (int q = 0; q < R; ++q) {
              stage[tid * (R + 1) + q] = w;
              w = qd_next(w, t.n_sites, d, bits);                         // past the last row: unchanged and unused
          }
      }
      __syncthreads();
#pragma unroll 1
      for (int q = 0; q < R; ++q) {
        const int local = q * kCorrBlock + tid;                           // made by lane local / R at its step local % R
        const int64_t row = base + local;
        if (row >= t.dim) break;
        const uint64_t s = stage[(local / R) * (R + 1) + local % R];
        const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
        const double w = fma(x.x, x.x, x.y * x.y);
        if (kind == kQcSite) {
#pragma unroll
            for (int g = 0; g < kQcItems; ++g) {      // shift | level << 8 | mask << 16; mask 0: level 0 = every row, 1 = none
                const uint32_t e = it[g];
                acc[g] += (((uint32_t)(s >> (e & 63u)) & (e >> 16)) == ((e >> 8) & 15u)) ? w : 0.0;
            }
            continue;
        }
        if (kind == kQcDD) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {             // shift_i | shift_j << 6 | a0 << 12 | b0 << 14
                const uint32_t e = it[g];
                if (e & kQcValid) {
                    const int li = (int)((uint32_t)(s >> (e & 63u)) & lm), lj = (int)((uint32_t)(s >> ((e >> 6) & 63u)) & lm);
                    const double *fa = tab + (kQcDiag + ((e >> 12) & 3u)) * kQcTabStride + li;
                    const double *fb = tab + (kQcDiag + ((e >> 14) & 3u)) * kQcTabStride + lj;
                    const double p0 = w * fa[0], p1 = w * fa[kQcTabStride], b0 = fb[0], b1 = fb[kQcTabStride];
                    acc[4 * g + 0] = fma(p0, b0, acc[4 * g + 0]);
                    acc[4 * g + 1] = fma(p0, b1, acc[4 * g + 1]);
                    acc[4 * g + 2] = fma(p1, b0, acc[4 * g + 2]);
                    acc[4 * g + 3] = fma(p1, b1, acc[4 * g + 3]);
                }
            }
            continue;
        }
        // PAIR: i | j << 6 | kQcNewI (the first pair of a new i; the pass's first pair is treated so too)
        int li = 0, Q = 0;
        uint64_t S = 0, ti = 0;
        double P = 1.0, hw = 0.0, ai = 0.0;
#pragma unroll
        for (int g0 = 0; g0 < G; g0 += 8) {
            uint64_t idx[8];
            bool hits[8];
            double wg[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int g = g0 + jj;
                const uint32_t e = it[g];
                hits[jj] = false;
                idx[jj] = 0;                           // read under hits[jj] only
                wg[jj] = 0.0;
                if (e & kQcValid) {                    // uniform; padding pairs close the last pass
                    const int i = (int)(e & 63u), j = (int)((e >> 6) & 63u);
                    if (g == 0 || (e & kQcNewI)) {
                        li = (int)((uint32_t)(s >> (i * bits)) & lm);
                        if (want_aa) {
                            Q = qd_charge(s, bits, i);
                            const uint64_t *ci = cum1 + i * tws;
                            ti = ci[Q - 1] - ci[Q];
                            ai = tab[kQcLow * kQcTabStride + li];
                            S = 0;
                        }
                        if (want_str) {
                            hw = w * tab[kQcEnd * kQcTabStride + li];
                            P = 1.0;
                        }
                        if (g == 0)                    // a pass may begin in the middle of an i: catch up over i < k < j
                            for (int k = i + 1; k < j; ++k) {
                                const int lk = (int)((uint32_t)(s >> (k * bits)) & lm);
                                if (want_aa) {
                                    Q += lk;
                                    const uint64_t *ck = cum1 + k * tws;
                                    S += (ck[Q - 1] - ck[Q - 1 - lk]) - (ck[Q] - ck[Q - lk]);
                                }
                                if (want_str) P *= tab[kQcMid * kQcTabStride + lk];
                            }
                    }
                    const int lj = (int)((uint32_t)(s >> (j * bits)) & lm);
                    if (want_str) {
                        acc[g] = fma(hw * P, tab[kQcEnd * kQcTabStride + lj], acc[g]);
                        P *= tab[kQcMid * kQcTabStride + lj];
                    }
                    if (want_aa) {
                        Q += lj;
                        const uint64_t *cj = cum1 + j * tws;
                        const uint64_t c0 = cj[Q], c1 = cj[Q - 1], c2 = cj[Q - lj], c3 = cj[Q - lj - 1];
                        hits[jj] = li >= 1 && lj <= d - 2;
                        idx[jj] = (uint64_t)row + (c2 - c3) + S + ti;
                        wg[jj] = ai * tab[kQcUp * kQcTabStride + lj];
                        S += (c1 - c3) - (c0 - c2);
                    }
                }
            }
            // only the lanes with a hit load and accumulate: no line is fetched for a lane that adds nothing
            if (want_aa) {
                if (REALX) {
                    double xv[8];
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj)
                        if (hits[jj]) xv[jj] = t.xr[idx[jj]];         // xv[jj] is written and read under hits[jj] only
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj)
                        if (hits[jj]) acc[G + g0 + jj] = fma(wg[jj] * xv[jj], x.x, acc[G + g0 + jj]);
                } else {
                    d2 xv[8];
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj)
                        if (hits[jj]) xv[jj] = t.xg[idx[jj]];
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj)
                        if (hits[jj]) {
                            acc[G + g0 + jj] += wg[jj] * fma(xv[jj].x, x.x, xv[jj].y * x.y);
                            acc[2 * G + g0 + jj] += wg[jj] * (xv[jj].x * x.y - xv[jj].y * x.x);
                        }
                }
            }
        }
      }
    }
    corr_block_partials<NA>(acc, red, t.partials);
}

template <int KIND>
void (*qc_kernel(bool rx))(CorrQudit)
{
    return rx ? k_corr_qudit<true, KIND> : k_corr_qudit<false, KIND>;
}

int corr_qudit_run(const char *who, int n_sites, int d, int total, const std::vector<uint64_t> &cum_raw, int64_t dim, const d2 *xg,
                   const double *xr, int n_diag, const double *diag, const double *hend, const double *gmid, const double *lower,
                   bool want_pop, bool want_dd, bool want_str, bool want_aa, std::vector<double> &comp, CorrPasses &qp, hipStream_t s,
                   std::vector<void *> &pool)
{
    const int N = n_sites, bits = bits_per_level(d), tw = total + 1, tws = tw + 1;
    std::vector<uint64_t> cum((size_t)N * tws, 0ULL);
    for (int k = 0; k < N; ++k)
        for (int q = 0; q < tw; ++q) cum[(size_t)k * tws + q + 1] = cum_raw[(size_t)k * tw + q];
    std::vector<double> tab((size_t)kQcTables * kQcTabStride, 0.0);
    for (int l = 0; l < d; ++l) {
        if (hend) tab[kQcEnd * kQcTabStride + l] = hend[l];
        if (gmid) tab[kQcMid * kQcTabStride + l] = gmid[l];
        if (lower && l >= 1) tab[kQcLow * kQcTabStride + l] = lower[l];
        if (lower && l + 1 < d) tab[kQcUp * kQcTabStride + l] = lower[l + 1];
        for (int a = 0; a < n_diag; ++a) tab[(kQcDiag + a) * kQcTabStride + l] = diag[a * d + l];
    }
    const int n_pairs = N * (N - 1) / 2, half = (n_diag + 1) / 2, nq = half * half;       // half^2 quads per pair
    const int n_site_items = 1 + (want_pop ? N * d : 0);
    qp.add(kQcPair, (want_str || want_aa) ? n_pairs : 0, kQcGroup);
    qp.add(kQcDD, want_dd ? n_pairs * nq : 0, 8);
    qp.add(kQcSite, n_site_items, kQcItems);
    CorrQudit t{};
    std::vector<uint32_t> item((size_t)qp.n_pass * kQcItems, 0u);
    {
        size_t q = 0;
        for (int i = 0; i < N; ++i)
            for (int j = i + 1; j < N; ++j, ++q) {
                if (qp.count[kQcPair])
                    item[(size_t)(qp.first[kQcPair] + q / kQcGroup) * kQcItems + q % kQcGroup] =
                        kQcValid | (uint32_t)i | ((uint32_t)j << 6) | (j == i + 1 ? kQcNewI : 0u);
                if (qp.count[kQcDD])
                    for (int A = 0; A < half; ++A)
                        for (int B = 0; B < half; ++B) {
                            const size_t quad = q * nq + (size_t)A * half + B;
                            item[(size_t)(qp.first[kQcDD] + quad / 8) * kQcItems + quad % 8] =
                                kQcValid | (uint32_t)(i * bits) | ((uint32_t)(j * bits) << 6) | ((uint32_t)(2 * A) << 12) | ((uint32_t)(2 * B) << 14);
                        }
            }
        const uint32_t lm = (1u << bits) - 1u;
        uint32_t *site = item.data() + (size_t)qp.first[kQcSite] * kQcItems;
        for (int k = 0; k < qp.count[kQcSite] * kQcItems; ++k) site[k] = 1u << 8;              // mask 0, level 1: no row
        site[0] = 0u;                                                                         // mask 0, level 0: every row
        for (int k = 1; k < n_site_items; ++k) {
            const int st = (k - 1) / d, l = (k - 1) % d;
            site[k] = (uint32_t)(st * bits) | ((uint32_t)l << 8) | (lm << 16);
        }
    }
    t.n_sites = N;
    t.d = d;
    t.bits = bits;
    t.total = total;
    t.tw = tw;
    t.want_str = want_str ? 1 : 0;
    t.want_aa = want_aa ? 1 : 0;
    t.dim = dim;
    t.xg = xg;
    t.xr = xr;
    uint64_t *d_cum = nullptr;
    double *d_tab = nullptr;
    uint32_t *d_item = nullptr;
    QBH_TRY(upload(cum, &d_cum, pool));
    QBH_TRY(upload(tab, &d_tab, pool));
    QBH_TRY(upload(item, &d_item, pool));
    t.cum = d_cum;
    t.tab = d_tab;
    t.item = d_item;
    const size_t lds = corr_qudit_lds(N, total);
    const int NA = xr ? qc_acc<true>() : qc_acc<false>();
    const int gx = corr_grid(dim, lds, kCorrBlock * kQcRows);
    // one launch per kind (a kind is a kernel instance with registers of its own), each a reduced launch in its slice of one
    // allocation; comp holds the sums of all passes in pass order
    double *d_partials = nullptr;
    QBH_HIP_WHO(who, qbh::dev_alloc(&d_partials, corr_reduce_doubles(gx, qp.n_pass, NA) * sizeof(double)));
    pool.push_back(d_partials);
    comp.clear();
    std::vector<double> part;
    for (int k = 0; k < 3; ++k) {
        if (qp.count[k] == 0) continue;
        t.item = d_item + (size_t)qp.first[k] * kQcItems;
        t.partials = d_partials + corr_reduce_doubles(gx, qp.first[k], NA);
        void (*kernel)(CorrQudit) = k == kQcPair ? qc_kernel<kQcPair>(xr != nullptr) : k == kQcDD ? qc_kernel<kQcDD>(xr != nullptr) : qc_kernel<kQcSite>(xr != nullptr);
        QBH_TRY(corr_reduce_launch(who, kernel, gx, qp.count[k], NA, kCorrBlock, lds, s, t, t.partials, pool, part));
        comp.insert(comp.end(), part.begin(), part.end());
    }
    return QBH_OK;
}

}  // namespace
}  // namespace qbh

extern "C" int qbh_corr_qudit_dev(int n_sites, int d, int total, const qbh_z *d_vec, const double *d_vec_re, int n_diag, const double *diag,
                                  const double *string_end, const double *string_mid, const double *lower, double *norm2, double *pop,
                                  double *dd, double *str, qbh_z *aa, void *stream)
{
    using namespace qbh;
    static const char *who = "qbh_corr_qudit_dev";
    QBH_TRY(qudit_check_shape(who, n_sites, d));
    if (total < 0 || total > n_sites * (d - 1)) {
        set_error("%s: total = %d (0 .. %d allowed)", who, total, n_sites * (d - 1));
        return QBH_EINVAL;
    }
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    QBH_TRY(qudit_corr_check_tables(who, d, n_diag, diag, string_end, string_mid, lower, dd != nullptr, str != nullptr, aa != nullptr));
    const int tw = total + 1;
    std::vector<uint64_t> cum, dims;
    qudit_table(n_sites, d, tw, cum, dims);
    if (dims[(size_t)total] >= (1ULL << 62)) {
        set_error("%s: a sector of 2^62 rows or more", who);
        return QBH_EUNSUPP;
    }
    // 64 sites x 66 columns x 8 B + tables + one tile of words = 45 KB at most: unreachable for the shapes accepted above
    const size_t lds = corr_qudit_lds(n_sites, total);
    if (lds > kCorrLdsCap) {
        set_error("%s: tables (%zu bytes) do not fit LDS", who, lds);
        return QBH_EUNSUPP;
    }
    QBH_TRY(corr_check_device());
    const int N = n_sites, K = n_diag;
    const bool want_pop = pop || dd || str || aa;                 // the diagonals of dd, str and aa follow from pop
    std::vector<void *> pool;
    std::vector<double> comp;
    CorrPasses qp;
    const int rc = corr_qudit_run(who, N, d, total, cum, (int64_t)dims[(size_t)total], reinterpret_cast<const d2 *>(d_vec), d_vec_re, K,
                                  diag, string_end, string_mid, lower, want_pop, dd != nullptr, str != nullptr, aa != nullptr, comp, qp,
                                  (hipStream_t)stream, pool);
    free_pool(pool);
    if (rc != QBH_OK) return rc;
    const bool rx = d_vec_re != nullptr;
    const int NA = rx ? qc_acc<true>() : qc_acc<false>(), G = kQcGroup;
    auto site_item = [&](int k) { return qp.at(comp, kQcSite, k, kQcItems, 0, NA); };
    if (norm2) *norm2 = site_item(0);
    const size_t NN = (size_t)N * N;
    const int half = (K + 1) / 2, nq = half * half;
    std::vector<double> pi((size_t)d);
    int q = 0;
    for (int i = 0; i < N; ++i) {
        for (int l = 0; want_pop && l < d; ++l) pi[(size_t)l] = site_item(1 + i * d + l);
        if (pop) std::copy(pi.begin(), pi.end(), pop + i * d);
        qudit_corr_put_diag(N, i, d, K, pi.data(), diag, string_end, lower, dd, str, aa);
        for (int j = i + 1; j < N; ++j, ++q) {
            const size_t ij = (size_t)i * N + j, ji = (size_t)j * N + i;
            if (str) str[ij] = str[ji] = qp.at(comp, kQcPair, q, G, 0, NA);
            if (aa) corr_put_herm(aa, N, i, j, qp.at(comp, kQcPair, q, G, 1, NA), rx ? 0.0 : qp.at(comp, kQcPair, q, G, 2, NA));
            if (dd)
                for (int a = 0; a < K; ++a)
                    for (int b = 0; b < K; ++b) {
                        const double v = qp.at_item(comp, kQcDD, q * nq + (a / 2) * half + b / 2, 8, 4, (a % 2) * 2 + b % 2, NA);
                        dd[(size_t)(a * K + b) * NN + ij] = v;           // <f_a(i) f_b(j)> ...
                        dd[(size_t)(b * K + a) * NN + ji] = v;           // ... = <f_b(j) f_a(i)>
                    }
        }
    }
    return QBH_OK;
}
