// qbh_kondo.hpp -- what the Kondo-lattice generators share: the word packing, the ranking and the terms of one row, used by
// qbh_kondo.hip (the full sector, qbh_gen_kondo and qbh_mf_kondo) and by the momentum sectors in qbh_sector.hpp / qbh_sector.hip
// (qbh_gen_kondo_repr) and qbh_sector_mf_kondo.hip (qbh_mf_kondo_repr, which also finds a word's place in the basis from kd_rank).
//
// A site carries a conduction-electron orbital and a localized spin-1/2.  A word is three n-bit fields
//     w = u | d << n | s << 2n      u, d: sites occupied by an up / down electron;  s: sites whose local spin is DOWN
// and the sector (n_elec, two_sz) holds every word with popcount(u) + popcount(d) = n_elec and
// (popcount(u) - popcount(d)) + (n - 2 popcount(s)) = two_sz.  popcount(s) = m fixes n_up(m) = nu0 + m and
// n_dn(m) = n_elec - n_up(m): the sector is the union over m in [m_lo, m_hi] of the blocks (n_up(m), n_dn(m), m).
// Basis order: ascending w.  With w(m) = C(n, n_up(m)) C(n, n_dn(m)) (0 outside [m_lo, m_hi]) the number of sector words
// whose s-field is below s is the sum, over the set bits p of s from the top with c ones above p, of
//     A[p][c] = sum_j C(p, j) w(c + j)
// (the s' that agree with s above p, hold 0 at p and j ones below it); inside one s the rank is
// rank(d) C(n, n_up) + rank(u), colexicographic ranks as in qbh_gen_hubbard.
// Fermion order as in qbh_gen_hubbard: all up operators, then all down operators, sites ascending.
#pragma once
#include <cstdint>

#include "qbh_internal.hpp"

namespace qbh {

constexpr int kKondoMaxSites = 21;        // 3 x 21 bits in one word
constexpr int kKondoTab = kKondoMaxSites + 1;
constexpr int kKondoMaxTerms = 448;       // merged directed one-body terms (i, j): at most 21 x 21
constexpr int kKondoMaxSbonds = 210;      // merged unordered local-spin bonds
constexpr int kKondoMaxRow = 160;         // entries of one row, diagonal included, counted from the merged terms

struct KondoDev {
    int n_sites, n_elec, two_sz, nu0, m_lo, m_hi, n_terms, n_sbonds;
    uint64_t total;                                        // words of the sector
    uint64_t binom[kKondoTab * kKondoTab];                 // [p * kKondoTab + k] = C(p, k)
    uint64_t A[kKondoTab * kKondoTab];                     // [p * kKondoTab + c], see above
    int8_t ti[kKondoMaxTerms], tj[kKondoMaxTerms];         // term t: amp * c^dag_{ti} c_{tj}
    double aup[kKondoMaxTerms][2], adn[kKondoMaxTerms][2];
    double U, kz[kKondoMaxSites], kxy[kKondoMaxSites];     // kz S^z_i s^z_i + kxy/2 (S^+_i s^-_i + h.c.)
    int8_t bi[kKondoMaxSbonds], bj[kKondoMaxSbonds];       // bz S^z_i S^z_j + bxy/2 (S^+_i S^-_j + h.c.), i < j
    double bz[kKondoMaxSbonds], bxy[kKondoMaxSbonds];
};

// Validates the shape and the terms, merges them into K (zeroed first) and fills its tables.  Returns the row capacity the
// merged terms need (> 0), or a code (< 0): n_sites outside
// [1, 21], n_elec outside [0, 2 n_sites], a parity of (n_elec, two_sz, n_sites) that admits no block, a term outside the
// lattice: QBH_EINVAL; merged hops not Hermitian: QBH_ENOTHERM; no block inside the range of n_up, n_dn (K.total = 0) or a
// row that may hold more than kKondoMaxRow entries: QBH_EUNSUPP.  Needs no device.  any_row_length: a row above kKondoMaxRow
// is not refused (the matrix-free form stages no row); every other check is unchanged.
int kondo_setup(const char *who, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites, const qbh_z *amp_up,
                const qbh_z *amp_dn, double U, const double *kz, const double *kxy, int n_sbonds, const int32_t *sbond_sites,
                const double *bz, const double *bxy, KondoDev &K, bool any_row_length = false);
// the shape part of kondo_setup alone (tables filled, no terms): for operators that only need the basis
int kondo_shape(const char *who, int n_sites, int n_elec, int two_sz, KondoDev &K);
// every merged term must be carried onto an equal one by every translation (QBH_EINVAL otherwise)
int kondo_invariant(const char *who, const KondoDev &K, int n_trans, const int32_t *perms);

// colexicographic rank of a pattern among those of its popcount
__device__ __forceinline__ uint64_t kd_rank_k(const uint64_t *binom, uint64_t bits)
{
    uint64_t r = 0;
    for (int k = 1; bits; ++k) {
        const int p = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        r += binom[p * kKondoTab + k];
    }
    return r;
}

__device__ __forceinline__ uint64_t kd_unrank_k(const uint64_t *binom, int n_sites, int k, uint64_t r)
{
    uint64_t bits = 0;
    int p = n_sites - 1;
    for (; k >= 1; --k) {
        while (binom[p * kKondoTab + k] > r) --p;
        bits |= 1ULL << p;
        r -= binom[p * kKondoTab + k];
        --p;
    }
    return bits;
}

// number of sector words whose s-field is below s
__device__ __forceinline__ uint64_t kd_srank(const uint64_t *A, uint64_t s)
{
    uint64_t r = 0;
    for (int c = 0; s; ++c) {
        const int p = 63 - __clzll((long long)s);
        s ^= 1ULL << p;
        r += A[p * kKondoTab + c];
    }
    return r;
}

__device__ __forceinline__ uint64_t kd_rank(const KondoDev &K, const uint64_t *A, const uint64_t *binom, uint64_t u, uint64_t d, uint64_t s)
{
    const int nu = K.nu0 + __popcll(s);
    return kd_srank(A, s) + kd_rank_k(binom, d) * binom[K.n_sites * kKondoTab + nu] + kd_rank_k(binom, u);
}

// the word of rank r < K.total as its three fields; *ru, *rd receive the ranks of u and d inside the block of s
__device__ __forceinline__ void kd_unrank(const KondoDev &K, const uint64_t *A, const uint64_t *binom, uint64_t r, uint64_t *u,
                                          uint64_t *d, uint64_t *s, uint64_t *ru, uint64_t *rd)
{
    uint64_t sb = 0;
    int c = 0;
    for (int p = K.n_sites - 1; p >= 0; --p) {
        const uint64_t a = A[p * kKondoTab + c];           // words that agree above p and hold 0 at p
        if (r >= a) {
            sb |= 1ULL << p;
            r -= a;
            ++c;
        }
    }
    const int nu = K.nu0 + c;
    const uint64_t cu = binom[K.n_sites * kKondoTab + nu];
    *s = sb;
    *rd = r / cu;
    *ru = r % cu;
    *d = kd_unrank_k(binom, K.n_sites, K.n_elec - nu, *rd);
    *u = kd_unrank_k(binom, K.n_sites, nu, *ru);
}

// The value of an off-diagonal entry from its code: kind << 12 | index << 1 | (1 if the fermion sign is -1), kind 0 = Kondo
// flip on site `index`, 1 = local-spin exchange on bond `index`, 2 / 3 = up / down hop of term `index`.
__device__ __forceinline__ d2 kd_value(const KondoDev &K, int code)
{
    const int kind = code >> 12, idx = (code >> 1) & 0x7ff;
    const double sg = (code & 1) ? -1.0 : 1.0;
    if (kind == 0) return d2{sg * 0.5 * K.kxy[idx], 0.0};
    if (kind == 1) return d2{0.5 * K.bxy[idx], 0.0};
    const double *a = kind == 2 ? K.aup[idx] : K.adn[idx];
    return d2{sg * a[0], sg * a[1]};
}

// Row (u, d, s) of the operator: emit(u', d', s', code) for every off-diagonal entry <u d s| H |u' d' s'> with a nonzero
// amplitude (each column at most once: the merged terms reach distinct words); returns the diagonal.
//   Kondo flip on site i (electron and local spin antiparallel, site singly occupied): both turn over.  With the up
//   electron on i, c^dag_{i,dn} c_{i,up} passes the up operators below i, then every other up operator and the down
//   operators below i; the reverse move has the same sign.
//   Hop of species sigma from ti to tj in the row's word: <a| c^dag_{ti} c_{tj} |b>, sign = (-1)^(sigma particles between).
template <class F>
__device__ __forceinline__ d2 kd_row_terms(const KondoDev &K, uint64_t u, uint64_t d, uint64_t s, F &&emit)
{
    d2 dg = {K.U * (double)__popcll(u & d), 0.0};
    for (int i = 0; i < K.n_sites; ++i) {
        const int iu = (int)((u >> i) & 1ULL), id = (int)((d >> i) & 1ULL), is = (int)((s >> i) & 1ULL);
        dg.x += 0.25 * K.kz[i] * (double)((iu - id) * (1 - 2 * is));
        if (iu != id && iu == is && K.kxy[i] != 0.0) {
            const uint64_t b = 1ULL << i, low = b - 1ULL;
            const int par = (__popcll(u & low) + __popcll(u & ~b) + __popcll(d & low)) & 1;
            emit(u ^ b, d ^ b, s ^ b, (i << 1) | par);
        }
    }
    for (int e = 0; e < K.n_sbonds; ++e) {
        const int i = K.bi[e], j = K.bj[e];
        if (((s >> i) ^ (s >> j)) & 1ULL) {
            dg.x -= 0.25 * K.bz[e];
            if (K.bxy[e] != 0.0) emit(u, d, s ^ (1ULL << i) ^ (1ULL << j), (1 << 12) | (e << 1));
        } else {
            dg.x += 0.25 * K.bz[e];
        }
    }
    for (int t = 0; t < K.n_terms; ++t) {
        const int ti = K.ti[t], tj = K.tj[t];
        for (int sp = 0; sp < 2; ++sp) {
            const double ar = sp ? K.adn[t][0] : K.aup[t][0], ai = sp ? K.adn[t][1] : K.aup[t][1];
            if (ar == 0.0 && ai == 0.0) continue;
            const uint64_t occ = sp ? d : u;
            if (ti == tj) {                                // number operator: diagonal
                if ((occ >> ti) & 1ULL) dg += d2{ar, ai};
                continue;
            }
            if (!((occ >> ti) & 1ULL) || ((occ >> tj) & 1ULL)) continue;
            const int lo_s = ti < tj ? ti : tj, hi_s = ti < tj ? tj : ti;
            const uint64_t between = ((1ULL << hi_s) - 1ULL) & ~((2ULL << lo_s) - 1ULL);
            const int par = __popcll(occ & between) & 1;
            const uint64_t occ2 = occ ^ (1ULL << ti) ^ (1ULL << tj);
            emit(sp ? u : occ2, sp ? occ2 : d, s, ((2 + sp) << 12) | (t << 1) | par);
        }
    }
    return dg;
}

}  // namespace qbh
