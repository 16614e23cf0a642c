// qbh_qudit.hip -- sites with d local levels and one conserved charge (spin S, bosons with at most n_max per site): device
// assembly (qbh_gen_qudit), the same operator applied without a stored matrix (qbh_mf_qudit, k_mf_qudit) and the operator x
// vector step qbh_mopr_qudit_dev.
//
// Basis (documented in include/qbhip.h): site s holds a level l_s in [0, d), the charge of a word is sum_s l_s, and the
// words of one charge are ranked in ascending order of sum_s l_s d^s (site n-1 most significant).  With
//     cnt[s][q] = number of words on sites 0..s-1 of charge q,   cum[s][q] = sum_{q' <= q} cnt[s][q'],
// the rank of a word is  sum_s ( cum[s][Q_s] - cum[s][Q_s - l_s] ),  Q_s = l_0 + ... + l_s the charge of sites 0..s: the
// words that agree with it above s and hold a smaller level at s.  The table cum[s][q] does not depend on the sector
// (at most 64 x 65 x 8 B = 33 KB for every allowed (n_sites, d)) and sits in LDS in every kernel here.
//
// A two-site move on sites i < j changes the levels of i and j and the charges Q_i .. Q_{j-1}; every other site keeps its
// contribution, so the column of a neighbour is the row plus a difference over sites i..j only (qd_move_delta).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_qudit.hpp"
#include "qbh_mf_row.hpp"

namespace qbh {
namespace {

constexpr int kQuditMaxRow = 240;        // entries of one row, diagonal included (the fill kernel stages 64 rows in LDS)
constexpr int kQuditFillBlock = 64;      // one wave per workgroup in the fill kernel: lane = row, LDS column = lane

struct QuditDev {
    int n_sites, d, bits, total, tw, n_pairs, max_row;
    const uint64_t *cum;        // [n_sites * tw]
    const int32_t *pair_ij;     // [n_pairs] i | j << 8, i < j
    const double *pdiag;        // [n_pairs * d^2] diagonal M[in][in] of pair p, in = l_i d + l_j
    const int32_t *eoff;        // [n_pairs * d^2 + 1] off-diagonal nonzeros of row `in` of pair p: eoff[p d^2 + in] ..
    const int32_t *eout;        // [n_ent] the column's levels l'_i | l'_j << 8
    const d2 *eval;             // [n_ent] M[in][out] = <in|M|out>, the row's entry
    const double *sdiag;        // [n_sites * d] single-site diagonal
};

__device__ __forceinline__ void qd_stage_table(uint64_t *dst, const uint64_t *src, int n, int nthreads)
{
    for (int k = threadIdx.x; k < n; k += nthreads) dst[k] = src[k];
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_qudit_count(QuditDev h, int64_t row_begin, int64_t row_end, int32_t *cnt)
{
    extern __shared__ uint64_t qd_lds[];
    qd_stage_table(qd_lds, h.cum, h.n_sites * h.tw, 256);
    const int d2n = h.d * h.d;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; row < row_end; row += stride) {
        const uint64_t w = qd_unrank(qd_lds, h.n_sites, h.d, h.bits, h.tw, h.total, (uint64_t)row);
        int c = 1;
        for (int p = 0; p < h.n_pairs; ++p) {                 // uniform: the pair's sites come through scalar loads
            const int ij = h.pair_ij[p];
            const int in = qd_level(w, h.bits, ij & 0xff) * h.d + qd_level(w, h.bits, ij >> 8);
            const int32_t *o = h.eoff + p * d2n + in;
            c += o[1] - o[0];
        }
        cnt[row - row_begin] = c;
    }
}

// One row per lane; its entries are insertion-sorted by column in the lane's own LDS column (entry k of lane L at k * 64 + L),
// as (column, entry index; -1 = the diagonal), then written out.  No private array: nothing spills to scratch.
__global__ __launch_bounds__(kQuditFillBlock) void k_qudit_fill(QuditDev h, int64_t row_begin, int64_t row_end, const int64_t *ia,
                                                                int32_t *ja, d2 *val)
{
    extern __shared__ uint64_t qd_lds[];
    const int ntab = h.n_sites * h.tw;
    qd_stage_table(qd_lds, h.cum, ntab, kQuditFillBlock);
    int32_t *scol = reinterpret_cast<int32_t *>(qd_lds + ntab) + threadIdx.x;
    int32_t *sent = scol + kQuditFillBlock * h.max_row;
    const int d2n = h.d * h.d;
    const int64_t stride = (int64_t)gridDim.x * kQuditFillBlock;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * kQuditFillBlock + threadIdx.x; row < row_end; row += stride) {
        const uint64_t w = qd_unrank(qd_lds, h.n_sites, h.d, h.bits, h.tw, h.total, (uint64_t)row);
        double dg = 0.0;
        for (int s = 0; s < h.n_sites; ++s) dg += h.sdiag[s * h.d + qd_level(w, h.bits, s)];
        int n = 0;
        for (int p = 0; p < h.n_pairs; ++p) {
            const int ij = h.pair_ij[p];
            const int i = ij & 0xff, j = ij >> 8;
            const int li = qd_level(w, h.bits, i), lj = qd_level(w, h.bits, j);
            const int in = li * h.d + lj;
            dg += h.pdiag[p * d2n + in];
            const int e0 = h.eoff[p * d2n + in], e1 = h.eoff[p * d2n + in + 1];
            if (e0 == e1) continue;
            const int Q = qd_charge(w, h.bits, j);
            for (int e = e0; e < e1; ++e) {
                const int o = h.eout[e];
                const int32_t c = (int32_t)((uint64_t)row + qd_move_delta(qd_lds, h.tw, h.bits, w, i, j, Q, lj, o & 0xff, o >> 8));
                int q = n++;
                while (q > 0 && scol[(q - 1) * kQuditFillBlock] > c) {
                    scol[q * kQuditFillBlock] = scol[(q - 1) * kQuditFillBlock];
                    sent[q * kQuditFillBlock] = sent[(q - 1) * kQuditFillBlock];
                    --q;
                }
                scol[q * kQuditFillBlock] = c;
                sent[q * kQuditFillBlock] = e;
            }
        }
        {
            const int32_t c = (int32_t)row;
            int q = n++;
            while (q > 0 && scol[(q - 1) * kQuditFillBlock] > c) {
                scol[q * kQuditFillBlock] = scol[(q - 1) * kQuditFillBlock];
                sent[q * kQuditFillBlock] = sent[(q - 1) * kQuditFillBlock];
                --q;
            }
            scol[q * kQuditFillBlock] = c;
            sent[q * kQuditFillBlock] = -1;
        }
        const int64_t p0 = ia[row - row_begin];
        for (int q = 0; q < n; ++q) {
            const int e = sent[q * kQuditFillBlock];
            ja[p0 + q] = scol[q * kQuditFillBlock];
            val[p0 + q] = e < 0 ? d2{dg, 0.0} : h.eval[e];
        }
    }
}

// vec_new[row] = sum_s coef[s] a(l'_s) vec_old[rank_old(row's word with l'_s -> l'_s - dq)], a(l') = local[l' d + l' - dq].
// The old rank is (contributions of the sites below s, charges unchanged) + (site s) + (sites above s, charges shifted by
// -dq): the shifted sum is formed over all sites first and the sites <= s are taken out of it on the way up.  Indices of
// terms that are taken out again or never used may leave [0, qmax]: they are clamped, never read out of the table.

__global__ __launch_bounds__(256) void k_qudit_mopr(int n_sites, int d, int bits, int tw, int total_new, int dq, QuditMopr cf,
                                                    const uint64_t *cum_g, const d2 *x_old, d2 *y_new, int64_t dim_new)
{
    extern __shared__ uint64_t qd_lds[];
    qd_stage_table(qd_lds, cum_g, n_sites * tw, 256);
    const int qmax = tw - 1;
    auto T = [&](int s, int q) -> uint64_t { return qd_lds[s * tw + min(max(q, 0), qmax)]; };
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < dim_new; row += stride) {
        const uint64_t w = qd_unrank(qd_lds, n_sites, d, bits, tw, total_new, (uint64_t)row);
        uint64_t hi = 0;                                      // sum over all sites of the shifted contributions
        int Q = 0;
        for (int s = 0; s < n_sites; ++s) {
            const int l = qd_level(w, bits, s);
            Q += l;
            hi += T(s, Q - dq) - T(s, Q - dq - l);
        }
        uint64_t lo = 0;
        double ar = 0.0, ai = 0.0;
        Q = 0;
        for (int s = 0; s < n_sites; ++s) {
            const int l = qd_level(w, bits, s), ls = l - dq;
            Q += l;
            hi -= T(s, Q - dq) - T(s, Q - dq - l);
            if (ls >= 0 && ls < d) {
                const double a_re = cf.la[l], a_im = cf.lb[l];
                if (a_re != 0.0 || a_im != 0.0) {
                    const uint64_t src = lo + (T(s, Q - dq) - T(s, Q - dq - ls)) + hi;
                    const double cr = cf.ca[s] * a_re - cf.cb[s] * a_im, ci = cf.ca[s] * a_im + cf.cb[s] * a_re;
                    const d2 x = x_old[src];
                    ar += cr * x.x - ci * x.y;
                    ai += cr * x.y + ci * x.x;
                }
            }
            lo += T(s, Q) - T(s, Q - l);
        }
        y_new[row] = d2{ar, ai};
    }
}

// ------------------------------------------------------------------------------------ matrix-free apply (kind 4) --
// y <- alpha H x + beta y + gamma x without a stored matrix.  One lane per row, grid-stride over a resident grid.  LDS holds
// cum, the single-site diagonal and the slot list; the class tables (pdiag, eout, eval) too when they fit (TLDS), else
// they are read from global memory (read-only, cached: every lane of every workgroup reads the same few hundred KB).
// A slot is uniform over the lanes: (pair, k) = entry k of the row `in` of the pair's class, amplitude 0 where that row
// has fewer entries -- then the lane gathers x[row] with weight 0, as k_mf_heis does for a bond that does not flip.
// Eight slots form a batch: indices and amplitudes first, then the eight x loads, then the FMAs.
constexpr int kMfQuditBlock = 512;
constexpr size_t kMfQuditLdsCap = (size_t)150 * 1024;        // the budget of launch_mf_heis

// LDS layout, 16-byte items first: eval[n_ent] (TLDS) | cum | sdiag | pdiag (TLDS) | slot | eout (TLDS)
inline size_t mf_qudit_lds_bytes(const MfQudit &t, bool tables)
{
    const size_t d2n = (size_t)t.d * t.d;
    size_t b = ((size_t)t.n_sites * t.tw + (size_t)t.n_sites * t.d) * 8 + (size_t)t.n_slots * 8;
    if (tables) b += (size_t)t.n_ent * 20 + (size_t)t.n_cls * d2n * 8;
    return b;
}

template <bool REALX, bool TLDS>
__global__ __launch_bounds__(kMfQuditBlock) void k_mf_qudit(MfQudit t, MfVec a)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t qd_lds[];
    __shared__ double red[3 * (kMfQuditBlock / 64)];
    const int tid = threadIdx.x;
    const int d = t.d, bits = t.bits, tw = t.tw, d2n = d * d;
    const int ncum = t.n_sites * tw, nsd = t.n_sites * d, npd = t.n_cls * d2n;
    d2 *l_eval = reinterpret_cast<d2 *>(qd_lds);
    uint64_t *cum = qd_lds + (TLDS ? 2 * (size_t)t.n_ent : 0);
    double *sdiag = reinterpret_cast<double *>(cum + ncum);
    double *l_pdiag = sdiag + nsd;
    int32_t *slot = reinterpret_cast<int32_t *>(l_pdiag + (TLDS ? npd : 0));
    int32_t *l_eout = slot + 2 * t.n_slots;
    for (int k = tid; k < ncum; k += kMfQuditBlock) cum[k] = t.cum[k];
    for (int k = tid; k < nsd; k += kMfQuditBlock) sdiag[k] = t.sdiag[k];
    for (int k = tid; k < 2 * t.n_slots; k += kMfQuditBlock) slot[k] = t.slot[k];
    if (TLDS) {
        for (int k = tid; k < npd; k += kMfQuditBlock) l_pdiag[k] = t.pdiag[k];
        for (int k = tid; k < t.n_ent; k += kMfQuditBlock) {
            l_eval[k] = t.eval[k];
            l_eout[k] = t.eout[k];
        }
    }
    __syncthreads();
    const double *pdiag = TLDS ? l_pdiag : t.pdiag;
    const int32_t *eout = TLDS ? l_eout : t.eout;
    const d2 *eval = TLDS ? l_eval : t.eval;
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kMfQuditBlock;
    for (int64_t lrow = (int64_t)blockIdx.x * kMfQuditBlock + tid; lrow < a.nrows; lrow += stride) {
        const int64_t grow = a.row_begin + lrow;
        const uint64_t w = qd_unrank(cum, t.n_sites, d, bits, tw, t.total, (uint64_t)grow);
        double dg = 0.0;
        if (t.has_single)
            for (int s = 0; s < t.n_sites; ++s) dg += sdiag[s * d + qd_level(w, bits, s)];
        d2 sum = {0.0, 0.0};
        for (int b0 = 0; b0 < t.n_slots; b0 += 8) {
            long long idx[8];
            d2 amp[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int sw = slot[2 * (b0 + j)], base = slot[2 * (b0 + j) + 1];
                const int si = sw & 0xff, sj = (sw >> 8) & 0xff;
                const int lj = qd_level(w, bits, sj);
                const int in = qd_level(w, bits, si) * d + lj;
                if (sw & (1 << 30)) dg += pdiag[((sw >> 16) & 0x3ff) * d2n + in];
                d2 v = {0.0, 0.0};
                if (REALX) v.x = eval[base + in].x;
                else       v = eval[base + in];
                long long q = grow;
                if (v.x != 0.0 || v.y != 0.0)
                    q = (long long)((uint64_t)grow +
                                    qd_move_delta(cum, tw, bits, w, si, sj, qd_charge(w, bits, sj), lj, 0, eout[base + in]));
                amp[j] = v;
                idx[j] = q;
            }
            if (REALX) {
                double xv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] = a.xr[idx[j]];
#pragma unroll
                for (int j = 0; j < 8; ++j) sum.x += amp[j].x * xv[j];
            } else {
                d2 xv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] = a.xg[idx[j]];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sum.x += amp[j].x * xv[j].x - amp[j].y * xv[j].y;
                    sum.y += amp[j].x * xv[j].y + amp[j].y * xv[j].x;
                }
            }
        }
        d2 yo, xi;
        mf_row_load<REALX>(a, lrow, grow, yo, xi);
        mf_row_finish(a, lrow, sum, dg, xi, yo, acc);
    }
    mf_block_partials<kMfQuditBlock>(acc, red, a.partials);
}

// entries a stored CSR of rows [row_begin, row_end) would hold (the diagonal always, exact zeros dropped): one sum per workgroup
__global__ __launch_bounds__(256) void k_mf_qudit_count(MfQudit t, int64_t row_begin, int64_t row_end, unsigned long long *part)
{
    extern __shared__ uint64_t qd_lds[];
    __shared__ unsigned long long red[256];
    qd_stage_table(qd_lds, t.cum, t.n_sites * t.tw, 256);
    const int d2n = t.d * t.d;
    unsigned long long c = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; row < row_end; row += stride) {
        const uint64_t w = qd_unrank(qd_lds, t.n_sites, t.d, t.bits, t.tw, t.total, (uint64_t)row);
        c += 1;
        for (int p = 0; p < t.n_pairs; ++p) {
            const int ij = t.pairs[p];
            c += t.nrow[(ij >> 16) * d2n + qd_level(w, t.bits, ij & 0xff) * t.d + qd_level(w, t.bits, (ij >> 8) & 0xff)];
        }
    }
    red[threadIdx.x] = c;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// ------------------------------------------------------------------------------------------------------- host side --
struct HipFree {
    std::vector<void *> p;
    ~HipFree() { for (void *q : p) (void)hipFree(q); }
};

template <typename T>
hipError_t up(HipFree &pool, T **d, const std::vector<T> &h)
{
    hipError_t e = qbh::dev_alloc(d, std::max<size_t>(h.size(), 1) * sizeof(T));
    if (e != hipSuccess) return e;
    pool.p.push_back(*d);
    return h.empty() ? hipSuccess : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace

int qudit_check_shape(const char *who, int n_sites, int d)
{
    if (n_sites <= 0 || d < 2) {
        set_error("%s: need n_sites >= 1 and d >= 2 (got %d, %d)", who, n_sites, d);
        return QBH_EINVAL;
    }
    if (d > kQuditMaxD) {
        set_error("%s: d = %d local levels; at most %d are supported", who, d, kQuditMaxD);
        return QBH_EUNSUPP;
    }
    if (n_sites * bits_per_level(d) > 64 || n_sites > 64) {
        set_error("%s: %d sites of %d bits do not pack into 64 bits", who, n_sites, bits_per_level(d));
        return QBH_EUNSUPP;
    }
    return QBH_OK;
}

int qudit_merge_terms(const char *who, int n_sites, int d, int n_pairs, const int32_t *pair_sites, const qbh_z *pair_mat,
                      int n_single, const int32_t *single_sites, const double *single_diag, QuditTerms &T)
{
    const int d2n = d * d;
    // merge the pair terms into (i < j) order; (j, i) is transposed: element [(a' d + b'), (a d + b)] -> [(b' d + a'), (b d + a)]
    for (int p = 0; p < n_pairs; ++p) {
        const int a = pair_sites[2 * p], b = pair_sites[2 * p + 1];
        if (a < 0 || b < 0 || a >= n_sites || b >= n_sites || a == b) {
            set_error("%s: pair %d = (%d, %d) is invalid for %d sites", who, p, a, b, n_sites);
            return QBH_EINVAL;
        }
        std::vector<std::complex<double>> &M = T.pm[{std::min(a, b), std::max(a, b)}];
        if (M.empty()) M.assign((size_t)d2n * d2n, 0.0);
        const qbh_z *src = pair_mat + (size_t)p * d2n * d2n;
        for (int r = 0; r < d2n; ++r)
            for (int c = 0; c < d2n; ++c) {
                const qbh_z z = src[(size_t)r * d2n + c];
                if (z.re == 0.0 && z.im == 0.0) continue;
                if (r / d + r % d != c / d + c % d) {
                    set_error("%s: pair %d element [%d][%d] = (%g, %g) changes the charge", who, p, r, c, z.re, z.im);
                    return QBH_EINVAL;
                }
                const int rr = a < b ? r : (r % d) * d + r / d, cc = a < b ? c : (c % d) * d + c / d;
                M[(size_t)rr * d2n + cc] += std::complex<double>(z.re, z.im);
            }
    }
    for (const auto &kv : T.pm)
        for (int r = 0; r < d2n; ++r)
            for (int c = r; c < d2n; ++c) {
                const std::complex<double> x = kv.second[(size_t)r * d2n + c], y = kv.second[(size_t)c * d2n + r];
                if (std::abs(x - std::conj(y)) > QBH_SPARSE_PRECISION) {
                    set_error("%s: the merged pair (%d, %d) is not Hermitian at [%d][%d]", who, kv.first.first, kv.first.second, r, c);
                    return QBH_ENOTHERM;
                }
            }
    std::vector<double> &sdiag = T.sdiag;
    sdiag.assign((size_t)n_sites * d, 0.0);
    for (int k = 0; k < n_single; ++k) {
        const int s = single_sites[k];
        if (s < 0 || s >= n_sites) {
            set_error("%s: single-site term %d names site %d of %d", who, k, s, n_sites);
            return QBH_EINVAL;
        }
        for (int l = 0; l < d; ++l) sdiag[(size_t)s * d + l] += single_diag[(size_t)k * d + l];
    }
    if ((int)T.pm.size() > kQuditMaxPairs) {
        set_error("%s: %d distinct site pairs; at most %d are supported", who, (int)T.pm.size(), kQuditMaxPairs);
        return QBH_EUNSUPP;
    }
    // term tables: per pair and state `in` of the row's word, the off-diagonal nonzeros <in|M|o> of that row (ascending o)
    std::vector<int32_t> &pair_ij = T.pair_ij, &eoff = T.eoff, &eout = T.eout;
    std::vector<double> &pdiag = T.pdiag;
    std::vector<d2> &eval = T.eval;
    int &max_row = T.max_row;
    eoff.assign(1, 0);
    for (const auto &kv : T.pm) {
        pair_ij.push_back(kv.first.first | (kv.first.second << 8));
        int worst = 0;
        for (int in = 0; in < d2n; ++in) {
            pdiag.push_back(kv.second[(size_t)in * d2n + in].real());
            int k = 0;
            for (int o = 0; o < d2n; ++o) {
                const std::complex<double> z = kv.second[(size_t)in * d2n + o];
                if (o == in || (z.real() == 0.0 && z.imag() == 0.0)) continue;
                eout.push_back((o / d) | ((o % d) << 8));
                eval.push_back(d2{z.real(), z.imag()});
                ++k;
            }
            eoff.push_back((int32_t)eout.size());
            worst = std::max(worst, k);
        }
        max_row += worst;
    }
    return QBH_OK;
}

int launch_mf_qudit(const MfQudit &t, const MfVec &a, hipStream_t s, int *nparts_out)
{
    const int ncu = device_cu_count();
    const bool tl = t.tables_lds != 0;
    const size_t lds = mf_qudit_lds_bytes(t, tl);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, ((size_t)158 * 1024) / (lds + 1024)));
    const int64_t nblk = (a.nrows + kMfQuditBlock - 1) / kMfQuditBlock;
    const int g = (int)std::min<int64_t>(nblk, (int64_t)ncu * per_cu);
#define QBH_QUDIT_LAUNCH(RX, TL)                                                                                                   \
    do {                                                                                                                          \
        QBH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mf_qudit<RX, TL>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                    (int)lds));                                                                                   \
        hipLaunchKernelGGL((k_mf_qudit<RX, TL>), dim3(g), dim3(kMfQuditBlock), lds, s, t, a);                                     \
    } while (0)
    if (a.xr != nullptr) {
        if (tl) QBH_QUDIT_LAUNCH(true, true); else QBH_QUDIT_LAUNCH(true, false);
    } else {
        if (tl) QBH_QUDIT_LAUNCH(false, true); else QBH_QUDIT_LAUNCH(false, false);
    }
#undef QBH_QUDIT_LAUNCH
    QBH_HIP(hipGetLastError());
    if (nparts_out) *nparts_out = g;
    return QBH_OK;
}

int qudit_corr_check_tables(const char *who, int d, int n_diag, const double *diag, const double *string_end, const double *string_mid,
                            const double *lower, bool want_dd, bool want_str, bool want_aa)
{
    auto refuse = [&](const char *fmt, auto... a) {
        set_error(fmt, who, a...);
        return QBH_EINVAL;
    };
    if (n_diag < 0 || n_diag > 4) return refuse("%s: n_diag = %d (0 .. 4 allowed)", n_diag);
    if (n_diag > 0 && diag == nullptr) return refuse("%s: diag is NULL with n_diag = %d", n_diag);
    if ((string_end != nullptr) != (string_mid != nullptr)) return refuse("%s: string_end and string_mid must both be given or both be NULL");
    if (want_dd && n_diag == 0) return refuse("%s: dd is wanted but n_diag = 0");
    if (want_str && string_end == nullptr) return refuse("%s: str is wanted but string_end and string_mid are NULL");
    if (want_aa && lower == nullptr) return refuse("%s: aa is wanted but lower is NULL");
    const struct { const char *name; const double *v; int first, n; } tabs[4] = {
        {"diag", diag, 0, n_diag * d}, {"string_end", string_end, 0, d}, {"string_mid", string_mid, 0, d}, {"lower", lower, 1, d}};
    for (const auto &tb : tabs)
        for (int k = tb.first; tb.v && k < tb.n; ++k)
            if (!std::isfinite(tb.v[k])) return refuse("%s: %s[%d] is not finite", tb.name, k);
    return QBH_OK;
}

}  // namespace qbh

using qbh::d2;

#define QBH_QHIP(who, call)                                                                \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            qbh::set_error("%s: %s failed: %s", (who), #call, hipGetErrorString(_e));      \
            (void)hipGetLastError();                                                       \
            return _e == hipErrorOutOfMemory ? QBH_ENOMEM : QBH_EHIP;                      \
        }                                                                                  \
    } while (0)

extern "C" int qbh_gen_qudit(qbh_csr **out, int n_sites, int d, int total, int n_pairs, const int32_t *pair_sites,
                             const qbh_z *pair_mat, int n_single, const int32_t *single_sites, const double *single_diag,
                             int64_t row_begin, int64_t row_end, int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    static const char *who = "qbh_gen_qudit";
    if (!out) {
        set_error("%s: out is NULL", who);
        return QBH_EINVAL;
    }
    QBH_TRY(qudit_check_shape(who, n_sites, d));
    if (total < 0 || total > n_sites * (d - 1) || n_pairs < 0 || n_single < 0 || (n_pairs > 0 && (!pair_sites || !pair_mat)) ||
        (n_single > 0 && (!single_sites || !single_diag))) {
        set_error("%s: invalid charge %d (0 .. %d) or term arrays", who, total, n_sites * (d - 1));
        return QBH_EINVAL;
    }
    QuditTerms T;
    QBH_TRY(qudit_merge_terms(who, n_sites, d, n_pairs, pair_sites, pair_mat, n_single, single_sites, single_diag, T));
    const int max_row = T.max_row;
    if (max_row > kQuditMaxRow) {
        set_error("%s: a row may hold %d entries; at most %d are supported", who, max_row, kQuditMaxRow);
        return QBH_EUNSUPP;
    }
    const int tw = total + 1;
    std::vector<uint64_t> cum, dims;
    qudit_table(n_sites, d, tw, cum, dims);
    const uint64_t dim_u = dims[(size_t)total];
    if (dim_out) *dim_out = (int64_t)std::min<uint64_t>(dim_u, (uint64_t)INT64_MAX);
    if (dim_u >= 2147483647ULL) {
        set_error("%s: dim %llu exceeds int32 columns", who, (unsigned long long)dim_u);
        return QBH_EUNSUPP;
    }
    const int64_t dim = (int64_t)dim_u;
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("%s: bad row range [%lld, %lld) of %lld", who, (long long)row_begin, (long long)row_end, (long long)dim);
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_QHIP(who, hipSetDevice(opts->device));

    HipFree pool;
    QuditDev h{};
    h.n_sites = n_sites;
    h.d = d;
    h.bits = bits_per_level(d);
    h.total = total;
    h.tw = tw;
    h.n_pairs = (int)T.pm.size();
    h.max_row = max_row;
    {
        uint64_t *c;
        int32_t *pij, *eo, *eu;
        double *pd, *sd;
        d2 *ev;
        QBH_QHIP(who, up(pool, &c, cum));
        QBH_QHIP(who, up(pool, &pij, T.pair_ij));
        QBH_QHIP(who, up(pool, &pd, T.pdiag));
        QBH_QHIP(who, up(pool, &eo, T.eoff));
        QBH_QHIP(who, up(pool, &eu, T.eout));
        QBH_QHIP(who, up(pool, &ev, T.eval));
        QBH_QHIP(who, up(pool, &sd, T.sdiag));
        h.cum = c; h.pair_ij = pij; h.pdiag = pd; h.eoff = eo; h.eout = eu; h.eval = ev; h.sdiag = sd;
    }
    const int64_t nrows = row_end - row_begin;
    const size_t tab_bytes = cum.size() * sizeof(uint64_t);
    const size_t fill_lds = tab_bytes + (size_t)kQuditFillBlock * max_row * 8;
    int32_t *d_cnt = nullptr;
    QBH_QHIP(who, qbh::dev_alloc(&d_cnt, (size_t)nrows * sizeof(int32_t)));
    pool.p.push_back(d_cnt);
    int64_t *d_ia = nullptr;
    QBH_QHIP(who, qbh::dev_alloc(&d_ia, (size_t)(nrows + 1) * sizeof(int64_t)));
    HipFree own;                                              // the CSR arrays until the handle adopts them
    own.p.push_back(d_ia);
    hipLaunchKernelGGL(k_qudit_count, dim3(blas_grid(nrows)), dim3(256), tab_bytes, 0, h, row_begin, row_end, d_cnt);
    QBH_QHIP(who, hipGetLastError());
    QBH_TRY(exclusive_scan(d_cnt, nrows, d_ia, 0));
    int64_t nnz = 0;
    QBH_QHIP(who, hipMemcpy(&nnz, d_ia + nrows, sizeof(int64_t), hipMemcpyDeviceToHost));
    int32_t *d_ja = nullptr;
    d2 *d_val = nullptr;
    QBH_QHIP(who, qbh::dev_alloc(&d_ja, (size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
    own.p.push_back(d_ja);
    QBH_QHIP(who, qbh::dev_alloc(&d_val, (size_t)std::max<int64_t>(nnz, 1) * sizeof(d2)));
    own.p.push_back(d_val);
    QBH_QHIP(who, hipFuncSetAttribute(reinterpret_cast<const void *>(k_qudit_fill), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)fill_lds));
    int64_t grid = (nrows + kQuditFillBlock - 1) / kQuditFillBlock;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(k_qudit_fill, dim3((unsigned)grid), dim3(kQuditFillBlock), fill_lds, 0, h, row_begin, row_end, d_ia, d_ja,
                       d_val);
    QBH_QHIP(who, hipGetLastError());
    QBH_QHIP(who, hipDeviceSynchronize());
    own.p.clear();                                            // ownership passes with the call (freed by it on failure)
    qbh_opts og;
    opts_generated(opts, &og);
    return qbh_csr_create_device(out, nrows, dim, row_begin, nnz, d_ia, d_ja, reinterpret_cast<qbh_z *>(d_val), 1, &og);
}

extern "C" int qbh_mf_qudit(qbh_csr **out, int n_sites, int d, int total, int n_pairs, const int32_t *pair_sites,
                            const qbh_z *pair_mat, int n_single, const int32_t *single_sites, const double *single_diag,
                            int64_t row_begin, int64_t row_end, int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    static const char *who = "qbh_mf_qudit";
    if (!out) {
        set_error("%s: out is NULL", who);
        return QBH_EINVAL;
    }
    QBH_TRY(qudit_check_shape(who, n_sites, d));
    if (total < 0 || total > n_sites * (d - 1) || n_pairs < 0 || n_single < 0 || (n_pairs > 0 && (!pair_sites || !pair_mat)) ||
        (n_single > 0 && (!single_sites || !single_diag))) {
        set_error("%s: invalid charge %d (0 .. %d) or term arrays", who, total, n_sites * (d - 1));
        return QBH_EINVAL;
    }
    QuditTerms T;
    QBH_TRY(qudit_merge_terms(who, n_sites, d, n_pairs, pair_sites, pair_mat, n_single, single_sites, single_diag, T));
    const int tw = total + 1;
    std::vector<uint64_t> cum, dims;
    qudit_table(n_sites, d, tw, cum, dims);
    const uint64_t dim_u = dims[(size_t)total];
    if (dim_out) *dim_out = (int64_t)std::min<uint64_t>(dim_u, (uint64_t)INT64_MAX);
    if (dim_u >= (1ULL << 62)) {
        set_error("%s: dim %llu exceeds 2^62", who, (unsigned long long)dim_u);
        return QBH_EUNSUPP;
    }
    const int64_t dim = (int64_t)dim_u;
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("%s: bad row range [%lld, %lld) of %lld", who, (long long)row_begin, (long long)row_end, (long long)dim);
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_QHIP(who, hipSetDevice(opts->device));

    // classes: the distinct merged pair matrices (compared bit for bit), each with its tables once
    const int d2n = d * d, np = (int)T.pm.size();
    std::map<std::string, int> cls_of;
    std::vector<int> cls(np), rep, maxk, base;                   // per pair | per class: first pair, longest row, entry base
    {
        int p = 0;
        for (const auto &kv : T.pm) {
            const std::string key(reinterpret_cast<const char *>(kv.second.data()), kv.second.size() * sizeof(kv.second[0]));
            const auto it = cls_of.emplace(key, (int)rep.size());
            if (it.second) rep.push_back(p);
            cls[p++] = it.first->second;
        }
    }
    const int n_cls = (int)rep.size();
    std::vector<int32_t> nrow((size_t)n_cls * d2n), eout((size_t)d2n, 0);
    std::vector<double> pdiag((size_t)n_cls * d2n);
    std::vector<d2> eval((size_t)d2n, d2{0.0, 0.0});             // entries [0, d^2): the zero block of the padding slots
    bool values_real = true;
    for (int c = 0; c < n_cls; ++c) {
        const int p = rep[(size_t)c];
        int mk = 0;
        for (int in = 0; in < d2n; ++in) {
            nrow[(size_t)c * d2n + in] = T.eoff[(size_t)p * d2n + in + 1] - T.eoff[(size_t)p * d2n + in];
            pdiag[(size_t)c * d2n + in] = T.pdiag[(size_t)p * d2n + in];
            mk = std::max(mk, (int)nrow[(size_t)c * d2n + in]);
        }
        maxk.push_back(mk);
        base.push_back((int)eval.size());
        eout.resize(eval.size() + (size_t)mk * d2n, 0);
        eval.resize(eval.size() + (size_t)mk * d2n, d2{0.0, 0.0});
        for (int in = 0; in < d2n; ++in)
            for (int k = 0; k < nrow[(size_t)c * d2n + in]; ++k) {
                const int e = T.eoff[(size_t)p * d2n + in] + k;
                eout[(size_t)base[(size_t)c] + (size_t)k * d2n + in] = T.eout[(size_t)e] >> 8;
                eval[(size_t)base[(size_t)c] + (size_t)k * d2n + in] = T.eval[(size_t)e];
                if (T.eval[(size_t)e].y != 0.0) values_real = false;
            }
    }
    std::vector<int32_t> pairs((size_t)np), slot;
    for (int p = 0; p < np; ++p) {
        const int c = cls[(size_t)p];
        pairs[(size_t)p] = T.pair_ij[(size_t)p] | (c << 16);
        for (int k = 0; k < std::max(1, maxk[(size_t)c]); ++k) {
            slot.push_back(pairs[(size_t)p] | (k == 0 ? 1 << 30 : 0));
            slot.push_back(maxk[(size_t)c] == 0 ? 0 : base[(size_t)c] + k * d2n);
        }
    }
    while (slot.size() % 16) slot.push_back(0);

    MfQudit t;
    t.n_sites = n_sites;
    t.d = d;
    t.bits = bits_per_level(d);
    t.total = total;
    t.tw = tw;
    t.n_pairs = np;
    t.n_cls = n_cls;
    t.n_ent = (int)eval.size();
    t.n_slots = (int)(slot.size() / 2);
    for (double v : T.sdiag)
        if (v != 0.0) t.has_single = 1;
    t.tables_lds = mf_qudit_lds_bytes(t, true) <= kMfQuditLdsCap ? 1 : 0;
    const int64_t bytes = (int64_t)(cum.size() * 8 + pairs.size() * 4 + nrow.size() * 4 + slot.size() * 4 + T.sdiag.size() * 8 + pdiag.size() * 8 +
                        eout.size() * 4 + eval.size() * 16);
    HipFree pool;
    QBH_QHIP(who, up(pool, &t.cum, cum));
    QBH_QHIP(who, up(pool, &t.pairs, pairs));
    QBH_QHIP(who, up(pool, &t.nrow, nrow));
    QBH_QHIP(who, up(pool, &t.slot, slot));
    QBH_QHIP(who, up(pool, &t.sdiag, T.sdiag));
    QBH_QHIP(who, up(pool, &t.pdiag, pdiag));
    QBH_QHIP(who, up(pool, &t.eout, eout));
    QBH_QHIP(who, up(pool, &t.eval, eval));

    const int64_t nrows = row_end - row_begin;
    const int cgrid = blas_grid(nrows);
    unsigned long long *d_part = nullptr;
    QBH_QHIP(who, qbh::dev_alloc(&d_part, (size_t)cgrid * sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_mf_qudit_count, dim3(cgrid), dim3(256), cum.size() * sizeof(uint64_t), 0, t, row_begin, row_end, d_part);
    std::vector<unsigned long long> part((size_t)cgrid);
    hipError_t ce = hipGetLastError();
    if (ce == hipSuccess) ce = hipMemcpy(part.data(), d_part, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d_part);
    QBH_QHIP(who, ce);
    int64_t nnz = 0;
    for (unsigned long long v : part) nnz += (int64_t)v;

    const int rc = adopt_mf(out, 4, &qbh_csr::mfq, t, pool.p, bytes, values_real, nrows, dim, row_begin, nnz, opts);
    if (rc == QBH_OK) pool.p.clear();                         // the handle owns the tables now
    return rc;
}

extern "C" int qbh_mopr_qudit_dev(int n_sites, int d, int total_old, int dq, const qbh_z *coef, const qbh_z *local,
                                  const qbh_z *d_vec_old, qbh_z *d_vec_new, int64_t *dim_new_out, void *stream)
{
    using namespace qbh;
    static const char *who = "qbh_mopr_qudit_dev";
    QBH_TRY(qudit_check_shape(who, n_sites, d));
    const int total_new = total_old + dq;
    if (!coef || !local || !d_vec_old || !d_vec_new || total_old < 0 || total_old > n_sites * (d - 1) || total_new < 0 ||
        total_new > n_sites * (d - 1)) {
        set_error("%s: invalid argument (charge %d -> %d of at most %d)", who, total_old, total_new, n_sites * (d - 1));
        return QBH_EINVAL;
    }
    QuditMopr cf{};
    for (int lp = 0; lp < d; ++lp)
        for (int l = 0; l < d; ++l) {
            const qbh_z z = local[lp * d + l];
            if (z.re == 0.0 && z.im == 0.0) continue;
            if (lp != l + dq) {
                set_error("%s: local[%d][%d] is nonzero but does not change the level by dq = %d", who, lp, l, dq);
                return QBH_EINVAL;
            }
            cf.la[lp] = z.re;
            cf.lb[lp] = z.im;
        }
    for (int s = 0; s < n_sites; ++s) {
        cf.ca[s] = coef[s].re;
        cf.cb[s] = coef[s].im;
    }
    const int tw = std::max(total_old, total_new) + 1;
    std::vector<uint64_t> cum, dims;
    qudit_table(n_sites, d, tw, cum, dims);
    const int64_t dim_new = (int64_t)std::min<uint64_t>(dims[(size_t)total_new], (uint64_t)INT64_MAX);
    if (dim_new_out) *dim_new_out = dim_new;
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    HipFree pool;
    uint64_t *d_cum = nullptr;
    QBH_QHIP(who, up(pool, &d_cum, cum));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_qudit_mopr, dim3(blas_grid(dim_new)), dim3(256), cum.size() * sizeof(uint64_t), s, n_sites, d,
                       bits_per_level(d), tw, total_new, dq, cf, d_cum, reinterpret_cast<const d2 *>(d_vec_old),
                       reinterpret_cast<d2 *>(d_vec_new), dim_new);
    QBH_QHIP(who, hipGetLastError());
    QBH_QHIP(who, hipStreamSynchronize(s));
    return QBH_OK;
}
