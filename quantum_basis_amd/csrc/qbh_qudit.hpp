// qbh_qudit.hpp -- what the d-level generators share: the word packing and ranking of qbh_qudit.hip (the full sector,
// qbh_gen_qudit) and of the momentum sectors in qbh_sector.hpp / qbh_sector.hip / qbh_sector_mf_qudit.hip (qbh_gen_qudit_repr,
// qbh_mf_qudit_repr), and the term merging all of them run.
//
// Site s holds a level l_s in [0, d) in bits [s b, (s+1) b), b = bits_per_level(d); words of one charge are ranked in
// ascending order of sum_s l_s d^s, which is the order of the packed words as integers.  The counting table cum[s][q] is
// described at the top of qbh_qudit.hip.
#pragma once
#include <complex>
#include <map>
#include <utility>
#include <vector>

#include "qbh_internal.hpp"

namespace qbh {

constexpr int kQuditMaxD = 8;
constexpr int kQuditMaxPairs = 1024;     // merged (unordered) site pairs

inline int bits_per_level(int d) { return d <= 2 ? 1 : d <= 4 ? 2 : 3; }

// cum[s * tw + q] for s < n_sites, q < tw; *dims = cnt[n_sites][q] (the dimension of every sector q < tw)
inline void qudit_table(int n_sites, int d, int tw, std::vector<uint64_t> &cum, std::vector<uint64_t> &dims)
{
    std::vector<uint64_t> cnt((size_t)tw, 0), nxt((size_t)tw);
    cnt[0] = 1;
    cum.assign((size_t)n_sites * tw, 0);
    for (int s = 0; s < n_sites; ++s) {
        uint64_t acc = 0;
        for (int q = 0; q < tw; ++q) cum[(size_t)s * tw + q] = (acc += cnt[q]);
        for (int q = 0; q < tw; ++q) {
            uint64_t v = 0;
            for (int l = 0; l < d && l <= q; ++l) v += cnt[q - l];
            nxt[q] = v;
        }
        cnt.swap(nxt);
    }
    dims = cnt;
}

__device__ __forceinline__ int qd_level(uint64_t w, int bits, int s)
{
    return (int)((w >> (s * bits)) & ((1ULL << bits) - 1));
}

// charge of sites 0..s
__device__ __forceinline__ int qd_charge(uint64_t w, int bits, int s)
{
    const int nb = (s + 1) * bits;
    if (nb < 64) w &= (1ULL << nb) - 1;
    if (bits == 1) return __popcll(w);
    if (bits == 2) return __popcll(w & 0x5555555555555555ULL) + 2 * __popcll(w & 0xAAAAAAAAAAAAAAAAULL);
    const uint64_t m0 = 0x9249249249249249ULL;          // bit 0 of every 3-bit field
    return __popcll(w & m0) + 2 * __popcll(w & (m0 << 1)) + 4 * __popcll(w & (m0 << 2));
}

// rank(new) - rank(old) for the move (l_i, l_j) -> (ni, nj) on sites i < j of w, Q = charge of sites 0..j (mod 2^64)
__device__ __forceinline__ uint64_t qd_move_delta(const uint64_t *cum, int tw, int bits, uint64_t w, int i, int j, int Q, int lj,
                                                 int ni, int nj)
{
    const uint64_t *cj = cum + j * tw;
    uint64_t delta = cj[Q - lj] - cj[Q - nj];
    int Qo = Q - lj, Qn = Q - nj;
    for (int t = j - 1; t > i; --t) {
        const uint64_t *ct = cum + t * tw;
        const int l = qd_level(w, bits, t);
        delta += (ct[Qn] - ct[Qn - l]) - (ct[Qo] - ct[Qo - l]);
        Qo -= l;
        Qn -= l;
    }
    (void)ni;                                              // Qn - ni == Qo - l_i: the lower halves cancel
    const uint64_t *ci = cum + i * tw;
    return delta + ci[Qn] - ci[Qo];
}

// the word of rank r among the words of charge `total` (walks from the most significant site down)
__device__ __forceinline__ uint64_t qd_unrank(const uint64_t *cum, int n_sites, int d, int bits, int tw, int total, uint64_t r)
{
    uint64_t w = 0;
    int Q = total;
    for (int s = n_sites - 1; s >= 0; --s) {
        const uint64_t *c = cum + s * tw;
        const uint64_t top = c[Q];
        int l = min(d - 1, Q);
        while (l > 0 && top - c[Q - l] > r) --l;          // largest level whose smaller siblings hold <= r words
        r -= top - c[Q - l];
        Q -= l;
        w |= (uint64_t)l << (s * bits);
    }
    return w;
}

// the rank of word w among the words of its charge, the inverse of qd_unrank: site s adds the words that agree with w above
// s and hold a smaller level at s, cum[s][Q_s] - cum[s][Q_s - l_s] with Q_s the charge of sites 0..s
__device__ __forceinline__ uint64_t qd_rank(const uint64_t *cum, int n_sites, int bits, int tw, uint64_t w)
{
    uint64_t r = 0;
    int Q = 0;
    for (int s = 0; s < n_sites; ++s) {
        const int l = qd_level(w, bits, s);
        Q += l;
        const uint64_t *c = cum + s * tw;
        r += c[Q] - c[Q - l];
    }
    return r;
}

// the next word of the same charge: the lowest site s that can take one more level while the sites below it give one up
// is raised, and the charge left below it is packed into the lowest sites (the smallest such word).  The last word of the
// sector comes back unchanged.
__device__ __forceinline__ uint64_t qd_next(uint64_t w, int n_sites, int d, int bits)
{
    int below = 0;
    for (int s = 0; s < n_sites; ++s) {
        const int l = qd_level(w, bits, s);
        if (below > 0 && l < d - 1) {
            uint64_t out = ((w >> (s * bits)) + 1ULL) << (s * bits);      // s >= 1, so the shift stays below 64
            int rest = below - 1;
            for (int t = 0; rest > 0; ++t) {
                const int v = min(d - 1, rest);
                out |= (uint64_t)v << (t * bits);
                rest -= v;
            }
            return out;
        }
        below += l;
    }
    return w;
}

// sum_s coef[s] O_s with one local d x d matrix O: la/lb[l'] = Re/Im <l'|O|l' - dq>
struct QuditMopr { double ca[64], cb[64]; double la[kQuditMaxD], lb[kQuditMaxD]; };

// The merged terms of a d-level operator and their device tables: per pair p (i < j, pair_ij = i | j << 8) and state
// `in` = l_i d + l_j of the row's word, the diagonal pdiag[p d^2 + in] and the off-diagonal nonzeros <in|M|o> of that row
// (ascending o) in eout / eval [eoff[p d^2 + in], eoff[p d^2 + in + 1]); sdiag[s d + l] the single-site diagonal.
// max_row = 1 + sum_p (most off-diagonal nonzeros in one row of pair p): the longest row the terms can produce.
struct QuditTerms {
    std::map<std::pair<int, int>, std::vector<std::complex<double>>> pm;   // d^2 x d^2, row = out, column = in
    std::vector<double> sdiag, pdiag;
    std::vector<int32_t> pair_ij, eoff, eout;
    std::vector<d2> eval;
    int max_row = 1;
};

// checks of qbh_gen_qudit on the shape: QBH_EINVAL below 1 site or 2 levels, QBH_EUNSUPP beyond 8 levels or 64 bits
int qudit_check_shape(const char *who, int n_sites, int d);
// merges and checks the terms as qbh_gen_qudit does (charge: QBH_EINVAL, Hermitian: QBH_ENOTHERM, sites: QBH_EINVAL,
// more than kQuditMaxPairs pairs: QBH_EUNSUPP) and builds the tables; the row capacity is the caller's to check
int qudit_merge_terms(const char *who, int n_sites, int d, int n_pairs, const int32_t *pair_sites, const qbh_z *pair_mat,
                      int n_single, const int32_t *single_sites, const double *single_diag, QuditTerms &T);


// what the two d-level correlation calls (qbh_corr_qudit.hip, qbh_corr_quditrepr.hip) share
// the table checks of the two d-level calls, in the order of qbh_corr_qudit_dev
int qudit_corr_check_tables(const char *who, int d, int n_diag, const double *diag, const double *string_end, const double *string_mid,
                            const double *lower, bool want_dd, bool want_str, bool want_aa);

// the diagonals of the d-level outputs (a NULL array is skipped) follow from the populations pi[l] of site i
inline void qudit_corr_put_diag(int N, int i, int d, int K, const double *pi, const double *diag, const double *string_end,
                                const double *lower, double *dd, double *str, qbh_z *aa)
{
    const size_t NN = (size_t)N * N, ii = (size_t)i * N + i;
    if (dd)
        for (int a = 0; a < K; ++a)
            for (int b = 0; b < K; ++b) {
                double v = 0.0;
                for (int l = 0; l < d; ++l) v += pi[l] * (diag[a * d + l] * diag[b * d + l]);
                dd[(size_t)(a * K + b) * NN + ii] = v;
            }
    if (str) {
        double v = 0.0;
        for (int l = 0; l < d; ++l) v += pi[l] * (string_end[l] * string_end[l]);
        str[ii] = v;
    }
    if (aa) {
        double v = 0.0;
        for (int l = 0; l + 1 < d; ++l) v += pi[l] * (lower[l + 1] * lower[l + 1]);
        aa[ii] = qbh_z{v, 0.0};
    }
}

}  // namespace qbh
