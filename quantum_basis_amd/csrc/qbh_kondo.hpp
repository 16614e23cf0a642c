// qbh_kondo.hpp -- what the Kondo-lattice generators share: the word packing, the ranking and the terms of one row, used by
// qbh_kondo.hip (the full sector, qbh_gen_kondo and qbh_mf_kondo) and by the momentum sectors in qbh_sector.hpp / qbh_sector.hip
// (qbh_gen_kondo_repr) and qbh_sector_mf_kondo.hip (qbh_mf_kondo_repr, which also finds a word's place in the basis from kd_rank),
// and by the all-pair correlation pass in qbh_corr_kondo.hip (qbh_corr_kondo_dev: kd_unrank, kd_rank, kd_rank_delta).
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

// rank(to) - rank(from) (mod 2^64) of two patterns with the same popcount that stand above k0 set bits
__device__ __forceinline__ uint64_t kd_rank_delta(const uint64_t *binom, uint64_t from, uint64_t to, int k0)
{
    uint64_t r = 0;
    for (int k = k0 + 1; to; ++k) {
        const int p2 = __ffsll((long long)to) - 1, p1 = __ffsll((long long)from) - 1;
        to &= to - 1;
        from &= from - 1;
        r += binom[p2 * kKondoTab + k] - binom[p1 * kKondoTab + k];
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

// ---- operators between sectors (qbh_kondo_mopr.hip): O = sum_s coef[s] O_s from (n_elec, two_sz) to another sector ----
//   op 0 / 1  c_{s,up} / c_{s,dn}           (n_elec - 1, two_sz -/+ 1)        op 2 / 3  c^dag_{s,up} / c^dag_{s,dn}  (n_elec + 1, two_sz +/- 1)
//   op 4      ce[s] s^+_s + cs[s] S^+_s     (n_elec, two_sz + 2)              op 5      ce[s] s^-_s + cs[s] S^-_s    (n_elec, two_sz - 2)
// with s^+_s = c^dag_{s,up} c_{s,dn}, s^-_s = c^dag_{s,dn} c_{s,up} (the product applied right to left) and S^+_s turning the
// local spin up (bit s of the s field cleared).  An electron operator carries (-1)^(operators left of it in the string "all up
// ascending, then all down ascending"): the particles of its species below s, and for the down species the whole up field.
constexpr int kKondoMoprOps = 6;

inline void kondo_mopr_target(int op, int n_elec, int two_sz, int *n_elec_new, int *two_sz_new)
{
    static const int de[kKondoMoprOps] = {-1, -1, 1, 1, 0, 0}, ds[kKondoMoprOps] = {-1, 1, 1, -1, 2, -2};
    *n_elec_new = n_elec + de[op];
    *two_sz_new = two_sz + ds[op];
}

// For the TARGET word (bu, bd, bs), site s and part (0: the electron operator, 1: the local-spin flip of ops 4 / 5) the SOURCE
// word (cu, cd, cs) and w = coef <b|O_s|c>, or false.  A row walks the sites ascending, part 0 before part 1.
struct KondoSiteOp {
    int n_sites, op;
    double ce_re[kKondoMaxSites], ce_im[kKondoMaxSites], cs_re[kKondoMaxSites], cs_im[kKondoMaxSites];
    __host__ __device__ __forceinline__ int parts() const { return op >= 4 ? 2 : 1; }
    __device__ __forceinline__ bool operator()(uint64_t bu, uint64_t bd, uint64_t bs, int s, int part, uint64_t &cu, uint64_t &cd,
                                               uint64_t &cs, d2 &w) const
    {
        const uint64_t bit = 1ULL << s, low = bit - 1ULL;
        if (part) {                           // S^+: the target's local spin is up (bit clear); S^-: down; the element is 1
            const bool down = (bs & bit) != 0;
            if ((op == 4 ? down : !down) || (cs_re[s] == 0.0 && cs_im[s] == 0.0)) return false;
            cu = bu;
            cd = bd;
            cs = bs ^ bit;
            w = d2{cs_re[s], cs_im[s]};
            return true;
        }
        if (ce_re[s] == 0.0 && ce_im[s] == 0.0) return false;
        int par;
        cs = bs;
        if (op < 4) {                         // b and c differ in the particle (s, species) alone
            const int species = op & 1, create = op >> 1;
            const uint64_t occ = species ? bd : bu;
            const bool has = (occ & bit) != 0;
            if (create ? !has : has) return false;
            par = (species ? __popcll(bu) : 0) + __popcll(occ & low);
            cu = species ? bu : bu ^ bit;
            cd = species ? bd ^ bit : bd;
        } else {                              // s^+: the target holds (s, up) alone, the source (s, dn) alone; s^-: the reverse
            const bool hu = (bu & bit) != 0, hd = (bd & bit) != 0;
            if (op == 4 ? (!hu || hd) : (hu || !hd)) return false;
            par = __popcll(bu & low) + __popcll(bu & ~bit) + __popcll(bd & low);      // as the Kondo flip of kd_row_terms
            cu = bu ^ bit;
            cd = bd ^ bit;
        }
        w = (par & 1) ? d2{-ce_re[s], -ce_im[s]} : d2{ce_re[s], ce_im[s]};
        return true;
    }
};

}  // namespace qbh
