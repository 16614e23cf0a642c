// qbh_sector.hpp -- the momentum-sector toolkit: the symmetry tables, the enumeration of orbit representatives, the row
// helpers and the four families (spin-1/2, Hubbard / t-J, d-level sites, Kondo lattice) with their row functions.  Used by
// the stored sector generators (qbh_sector.hip), the operators between sectors (qbh_sector_mopr.hip) and the matrix-free
// sectors (Hubbard: qbh_sector_mf.hip, d-level sites: qbh_sector_mf_qudit.hip, Kondo lattice: qbh_sector_mf_kondo.hip).  Internal linkage: each translation unit instantiates the kernels it uses.
#pragma once
#include "qbh_gen_util.hpp"
#include "qbh_dict.hpp"
#include "qbh_qudit.hpp"
#include "qbh_kondo.hpp"

// ------------------------------------------------- translation-symmetric sectors --
// Device counterpart of model::generate_Ham_sparse_repr (src/model.cc:687-836) for spin-1/2 Heisenberg models:
// the Hamiltonian in the basis of momentum states built on orbit representatives.  The reference reaches the
// representative of a hopped state through its sublattice (Weisse) tables; here every state is canonicalised
// directly -- all |G| translations are applied with byte-sliced lookup tables and the smallest image wins.
//   basis      the orbit representatives of the fixed-n_dn sector (see k_sector_flag for what every family's basis holds)
//   H[a][b]    sum over bond terms taking |a> to c = l.b of h * conj(chi(g*)) * sqrt(|S_b|/|S_a|), g* c = b
//              (the phase exp(2 pi i k.d/L) * sqrt(nu_i/nu_j) of src/model.cc:808-814)
namespace qbh {
namespace {

constexpr int kReprMaxTrans = 64;

// the symmetry tables of a momentum sector: checks that translation 0 is the identity and every translation a site
// permutation, fills the binomials (unless binom is null) and the characters, stores the permutations in perm8
// (perm8[g * n_sites + site]) unless it is null and builds the chunk tables tab[(g*n_chunks + c)*64 + v] = scattered bits
// of chunk c with value v under g.  A site holds `bits` bits (1, 2 or 3), so a 6-bit chunk holds 6 / bits whole sites.
// `who` prefixes error messages.
inline int sector_symmetry(int n_sites, int n_trans, const int32_t *perms, const double *chars, const char *who, uint64_t (*binom)[34],
                    double *chr, int8_t *perm8, int &n_chunks, std::vector<uint64_t> &tab, int bits = 1)
{
    for (int i = 0; i < n_sites; ++i)
        if (perms[i] != i) {
            set_error("%s: translation 0 must be the identity", who);
            return QBH_EINVAL;
        }
    for (int g = 0; g < n_trans; ++g) {
        std::vector<int> seen((size_t)n_sites, 0);
        for (int s = 0; s < n_sites; ++s) {
            const int img = perms[(size_t)g * n_sites + s];
            if (img < 0 || img >= n_sites || seen[(size_t)img]++) {
                set_error("%s: translation %d is not a site permutation", who, g);
                return QBH_EINVAL;
            }
            if (perm8) perm8[g * n_sites + s] = (int8_t)img;
        }
    }
    if (binom)
        for (int p = 0; p <= 64; ++p)
            for (int k = 0; k <= 33; ++k) binom[p][k] = binom_u64(p, k);
    for (int g = 0; g < n_trans; ++g) {
        chr[2 * g] = chars[2 * g];
        chr[2 * g + 1] = chars[2 * g + 1];
    }
    const int per = 6 / bits;                 // sites per chunk
    const uint64_t field = (1ULL << bits) - 1ULL;
    n_chunks = (n_sites + per - 1) / per;
    tab.assign((size_t)n_trans * n_chunks * 64, 0ULL);
    for (int g = 0; g < n_trans; ++g)
        for (int c = 0; c < n_chunks; ++c)
            for (int v = 0; v < 64; ++v) {
                uint64_t m = 0;
                for (int b = 0; b < per; ++b) {
                    const int site = per * c + b;
                    const uint64_t l = ((uint64_t)v >> (b * bits)) & field;
                    if (site < n_sites && l) m |= l << (perms[(size_t)g * n_sites + site] * bits);
                }
                tab[((size_t)g * n_chunks + c) * 64 + v] = m;
            }
    return QBH_OK;
}

// image of bit pattern s under translation g; tab[(g*n_chunks + c)*64 + v] = scattered bits of chunk c with value v
__device__ __forceinline__ uint64_t repr_translate(const uint64_t *tab, int n_chunks, int g, uint64_t s)
{
    uint64_t out = 0;
    const uint64_t *t = tab + (size_t)g * n_chunks * 64;
    for (int c = 0; c < n_chunks; ++c) out |= t[c * 64 + ((s >> (6 * c)) & 63ULL)];
    return out;
}

__device__ __forceinline__ uint64_t unrank_k(const uint64_t (*binom)[34], int n_sites, int k, uint64_t r)
{
    uint64_t bits = 0;
    int p = n_sites - 1;
    for (; k >= 1; --k) {
        while (binom[p][k] > r) --p;
        bits |= 1ULL << p;
        r -= binom[p][k];
        --p;
    }
    return bits;
}

// next bit pattern with the same popcount (Gosper)
__device__ __forceinline__ uint64_t next_same_popcount(uint64_t s)
{
    const uint64_t t2 = s | (s - 1ULL);
    return (t2 + 1ULL) | (((~t2 & (t2 + 1ULL)) - 1ULL) >> (__ffsll((long long)s)));
}

// ---- what a sector family is ----
// A family is a device struct Dev (n_trans, n_chunks, chr, fake_pos and its own terms) with, next to it,
//   sector_word_count(R, ctab)      host: the number of words of the sector (UINT64_MAX if that overflows); a family whose
//                                   cursor reads a counting table on the device leaves it in ctab, and
//   sector_tables(R, ctab, pool)    uploads it and points R at it (default: nothing)
//   sector_seek(R, r)               the cursor at the word of rank r (ascending words); sector_word(R, cur) the word under it,
//   sector_step(R, cur)             the step to the next word
//   sector_allowed(R, s)            whether word s is in the space at all (default: yes)
//   sector_translate(R, tab, g, s)  the image of s under translation g (default: one field of n_chunks chunks)
//   sector_parity(R, g, s)          1 if T_g |s> = -|g(s)> (default: 0, no signs)
//   sector_row(R, ...), max_row<Dev>  one row of the sector operator and its capacity
// The defaults below serve a family whose word is one field and whose cursor is the word itself; a family with more
// structure overloads them for its struct.
template <class Dev> int sector_tables(Dev &, const std::vector<uint64_t> &, std::vector<void *> &) { return QBH_OK; }
template <class Dev> __device__ __forceinline__ uint64_t sector_word(const Dev &, uint64_t cur) { return cur; }
template <class Dev> __device__ __forceinline__ bool sector_allowed(const Dev &, uint64_t) { return true; }
template <class Dev> __device__ __forceinline__ int sector_parity(const Dev &, int, uint64_t) { return 0; }
template <class Dev>
__device__ __forceinline__ uint64_t sector_translate(const Dev &R, const uint64_t *tab, int g, uint64_t s)
{
    return repr_translate(tab, R.n_chunks, g, s);
}
template <class Dev> constexpr int max_row = 0;

// ---- the row toolkit of the families: everything from the point where a term's value v and its column are known ----
// smallest image of s and the translation that produces it
template <class Dev>
__device__ __forceinline__ uint64_t sector_canonical(const Dev &R, const uint64_t *tab, uint64_t s, int *gstar)
{
    uint64_t best = s;
    int gb = 0;                           // g = 0 is the identity
    for (int g = 1; g < R.n_trans; ++g) {
        const uint64_t t = sector_translate(R, tab, g, s);
        if (t < best) {
            best = t;
            gb = g;
        }
    }
    *gstar = gb;
    return best;
}

// position of representative b in the ascending list reps[0, dim)
__device__ __forceinline__ int64_t sector_find(const uint64_t *reps, int64_t dim, uint64_t b)
{
    int64_t lo = 0, hi = dim;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (reps[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the row of a representative whose norm vanishes at this momentum: it stays in the basis, decoupled, with the fake diagonal
// fake_pos + i/dim (src/model.cc:735-740)
__device__ __forceinline__ int row_zero_norm(double fake_pos, int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    cols[0] = (int32_t)i;
    vals[0] = d2{fake_pos + (double)i / (double)dim, 0.0};
    return 1;
}

// v at column lo among the entries [first, n): added to that column if the row has it, else appended while there is room
__device__ __forceinline__ void row_merge(int32_t *cols, d2 *vals, int &n, int cap, int first, int64_t lo, d2 v)
{
    int q = first;
    while (q < n && cols[q] != (int32_t)lo) ++q;
    if (q < n) {
        vals[q] += v;
    } else if (n < cap) {
        cols[n] = (int32_t)lo;
        vals[n] = v;
        ++n;
    }
}

// v at column lo of row i, whose slot 0 is kept for the diagonal dg
__device__ __forceinline__ void row_add(int32_t *cols, d2 *vals, int &n, int cap, int64_t i, int64_t lo, d2 v, d2 &dg)
{
    if (lo == i) dg += v;
    else row_merge(cols, vals, n, cap, 1, lo, v);
}

__device__ __forceinline__ void row_sort(int32_t *cols, d2 *vals, int m)      // insertion sort by column (rows are short)
{
    for (int q = 1; q < m; ++q) {
        const int32_t c = cols[q];
        const d2 v = vals[q];
        int p = q - 1;
        while (p >= 0 && cols[p] > c) {
            cols[p + 1] = cols[p];
            vals[p + 1] = vals[p];
            --p;
        }
        cols[p + 1] = c;
        vals[p + 1] = v;
    }
}

// the diagonal into slot 0, cancelled off-diagonal entries dropped (lil_mat::add, src/sparse.cc:72-77), columns ascending;
// returns the row's length
__device__ __forceinline__ int row_finish(int32_t *cols, d2 *vals, int n, d2 dg)
{
    vals[0] = dg;
    int m = 1;
    for (int q = 1; q < n; ++q)
        if (vals[q].x * vals[q].x + vals[q].y * vals[q].y >= 1e-28) {
            cols[m] = cols[q];
            vals[m] = vals[q];
            ++m;
        }
    row_sort(cols, vals, m);
    return m;
}

// ------------------------------------ spin-1/2 family (qbh_gen_heisenberg_repr) --
constexpr int kReprMaxRow = 160;          // distinct columns in one row (unique bonds + diagonal)

struct ReprDev {
    HeisDev h;                            // binomials, bonds, amplitudes
    int n_trans, n_chunks;
    double chr[2 * kReprMaxTrans];        // characters chi(g)
    double fake_pos;
};
template <> constexpr int max_row<ReprDev> = kReprMaxRow;

inline uint64_t sector_word_count(const ReprDev &R, std::vector<uint64_t> &) { return binom_u64(R.h.n_sites, R.h.n_dn); }
__device__ __forceinline__ uint64_t sector_seek(const ReprDev &R, uint64_t r) { return heis_unrank(R.h, r); }
__device__ __forceinline__ void sector_step(const ReprDev &, uint64_t &cur) { cur = next_same_popcount(cur); }

// one row of the sector Hamiltonian into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int repr_row(const ReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                        int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double si = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    int n = 1;
    cols[0] = (int32_t)i;
    d2 dg = {0.0, 0.0};
    for (int bnd = 0; bnd < R.h.n_bonds; ++bnd) {
        const int x = R.h.sa[bnd], y = R.h.sb[bnd];
        if (((a >> x) ^ (a >> y)) & 1ULL) {
            dg.x -= R.h.diag[bnd];
            const uint64_t c = a ^ (1ULL << x) ^ (1ULL << y);
            int g = 0;
            const uint64_t b = sector_canonical(R, tab, c, &g);
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;      // zero-norm target: dropped (src/model.cc:806)
            const double f = R.h.offd[bnd] * sqrt((double)(cj & 0x7f) / si);
            const d2 v = {f * R.chr[2 * g], -f * R.chr[2 * g + 1]};          // h * conj(chi(g*)) * sqrt(|S_b|/|S_a|)
            row_add(cols, vals, n, kReprMaxRow, i, lo, v, dg);
        } else {
            dg.x += R.h.diag[bnd];
        }
    }
    return row_finish(cols, vals, n, dg);
}

__device__ __forceinline__ int sector_row(const ReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim,
                                          int64_t i, int32_t *cols, d2 *vals)
{
    return repr_row(R, tab, reps, info, dim, i, cols, vals);
}

// ------------------------------------ Hubbard family in translation-symmetric sectors --
// Device counterpart of model::enumerate_basis_repr + generate_Ham_sparse_repr (src/model.cc:687-836) for two-species
// fermions (the reference's examples/trans_symmetric/latt_square/square_Fermi_Hubbard.cc).  A basis state is the pair of
// occupation patterns (u, d) with the operator order "all up (ascending site), then all down", stored as the word
// s = u | d << n_sites (ascending words: rank = rank(d) * C(n, n_up) + rank(u)); a translation g maps c^dag_{i,sigma} to
// c^dag_{g(i),sigma}, so
//     T_g |u, d> = sgn(g, u) sgn(g, d) |g(u), g(d)>,   sgn = parity of the inversions among the images of the occupied sites,
// and the norm of a representative is the SIGNED character sum over its stabiliser.  The operator is a list of directed
// one-body terms  amp_sigma * c^dag_{i,sigma} c_{j,sigma}  plus U sum_i n_{i,up} n_{i,dn}; it must commute with the
// translations (a Hamiltonian does; a single-site operator has to be translation-averaged first, exactly as
// measure_repr_static does, src/model.cc:1874-1888).  With |a,k> = (|G||S_a|)^(-1/2) sum_g chi_k(g) T_g |a>, row a holds
//     O[a][b] = sum over terms that move a particle of a from i to j, giving c with T_{g*} |c> = sigma |b>:
//               amp * (hop sign) * sigma * conj(chi_k(g*)) * sqrt(|S_b| / |S_a|).
constexpr int kHubReprMaxTerms = 512;
constexpr int kHubReprMaxPairs = 256;
constexpr int kHubReprMaxRow = 160;       // distinct columns in one row: one move per bond and species, one exchange, the diagonal

struct HubReprDev {
    uint64_t binom[65][34];
    int n_sites, n_up, n_dn, n_terms, n_trans, n_chunks;
    int8_t ti[kHubReprMaxTerms], tj[kHubReprMaxTerms];     // term t: amp * c^dag_{ti} c_{tj}
    double aup[kHubReprMaxTerms][2], adn[kHubReprMaxTerms][2];
    int n_pairs;                                           // density-density terms v * n_{pi,s} n_{pj,s'}
    int8_t pi[kHubReprMaxPairs], pj[kHubReprMaxPairs];
    double pv[kHubReprMaxPairs][4];                        // (up,up) (up,dn) (dn,up) (dn,dn)
    int n_exch, no_double;                                 // spin-exchange terms xa * (S+_i S-_j + S-_i S+_j); t-J constraint
    int8_t xi[kHubReprMaxPairs], xj[kHubReprMaxPairs];
    double xa[kHubReprMaxPairs];
    double U, fake_pos;
    double chr[2 * kReprMaxTrans];
    int8_t perm[kReprMaxTrans * 32];                       // perm[g * n_sites + site]
};
template <> constexpr int max_row<HubReprDev> = kHubReprMaxRow;

inline uint64_t sector_word_count(const HubReprDev &R, std::vector<uint64_t> &)
{
    const uint64_t cu = binom_u64(R.n_sites, R.n_up), cd = binom_u64(R.n_sites, R.n_dn);
    return cu > UINT64_MAX / cd ? UINT64_MAX : cu * cd;
}

struct HubCursor { uint64_t u, d, ru; };                   // the two patterns and the rank of the up pattern

__device__ __forceinline__ HubCursor sector_seek(const HubReprDev &R, uint64_t r)
{
    const uint64_t cu = R.binom[R.n_sites][R.n_up];
    HubCursor c;
    c.ru = r % cu;
    c.u = unrank_k(R.binom, R.n_sites, R.n_up, c.ru);
    c.d = unrank_k(R.binom, R.n_sites, R.n_dn, r / cu);
    return c;
}
__device__ __forceinline__ uint64_t sector_word(const HubReprDev &R, const HubCursor &c) { return c.u | (c.d << R.n_sites); }
__device__ __forceinline__ void sector_step(const HubReprDev &R, HubCursor &c)
{
    if (++c.ru == R.binom[R.n_sites][R.n_up]) {            // next down pattern, up patterns start over
        c.ru = 0;
        c.u = (R.n_up > 0) ? ((1ULL << R.n_up) - 1ULL) : 0ULL;
        c.d = R.n_dn > 0 ? next_same_popcount(c.d) & ((1ULL << R.n_sites) - 1ULL) : 0ULL;
    } else {
        c.u = next_same_popcount(c.u);
    }
}
// t-J: words with a doubly occupied site are not in the space
__device__ __forceinline__ bool sector_allowed(const HubReprDev &R, uint64_t s)
{
    return !(R.no_double && (s & (s >> R.n_sites) & ((1ULL << R.n_sites) - 1ULL)));
}
__device__ __forceinline__ uint64_t sector_translate(const HubReprDev &R, const uint64_t *tab, int g, uint64_t s)
{
    const uint64_t m = (1ULL << R.n_sites) - 1ULL;
    const uint64_t u = repr_translate(tab, R.n_chunks, g, s & m), d = repr_translate(tab, R.n_chunks, g, s >> R.n_sites);
    return u | (d << R.n_sites);
}

// parity (0 / 1) of the permutation that sorts the images of the occupied sites of `occ` under the translation whose images are
// p[site] (a row of HubReprDev::perm, wherever it is kept)
__device__ __forceinline__ int hubrepr_parity(const int8_t *p, uint64_t occ)
{
    uint64_t seen = 0;
    int par = 0;
    while (occ) {
        const int i = __ffsll((long long)occ) - 1;
        occ &= occ - 1;
        const int img = p[i];
        par ^= __popcll(seen >> img) & 1;                  // images placed so far that lie above this one
        seen |= 1ULL << img;
    }
    return par;
}
__device__ __forceinline__ int hubrepr_parity(const HubReprDev &R, int g, uint64_t occ)
{
    return hubrepr_parity(R.perm + g * R.n_sites, occ);
}
__device__ __forceinline__ int sector_parity(const HubReprDev &R, int g, uint64_t s)
{
    return hubrepr_parity(R, g, s & ((1ULL << R.n_sites) - 1ULL)) ^ hubrepr_parity(R, g, s >> R.n_sites);
}

// smallest image, the translation that produces it and the sign of T_{g*}
__device__ __forceinline__ uint64_t hubrepr_canonical(const HubReprDev &R, const uint64_t *tab, uint64_t s, int *gstar, int *parity)
{
    const uint64_t best = sector_canonical(R, tab, s, gstar);
    *parity = *gstar ? sector_parity(R, *gstar, s) : 0;
    return best;
}

// one row of the sector operator into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int hubrepr_row(const HubReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                           int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double sa = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    const uint64_t mlow = (1ULL << R.n_sites) - 1ULL;
    const uint64_t au = a & mlow, ad = a >> R.n_sites;
    int n = 1;
    cols[0] = (int32_t)i;
    d2 dg = {R.U * (double)__popcll(au & ad), 0.0};
    for (int p = 0; p < R.n_pairs; ++p) {
        const int iu = (int)((au >> R.pi[p]) & 1ULL), id = (int)((ad >> R.pi[p]) & 1ULL);
        const int ju = (int)((au >> R.pj[p]) & 1ULL), jd = (int)((ad >> R.pj[p]) & 1ULL);
        dg.x += R.pv[p][0] * (iu & ju) + R.pv[p][1] * (iu & jd) + R.pv[p][2] * (id & ju) + R.pv[p][3] * (id & jd);
    }
    for (int t = 0; t < R.n_terms; ++t) {
        const int ti = R.ti[t], tj = R.tj[t];
        for (int sp = 0; sp < 2; ++sp) {
            const double ar = sp ? R.adn[t][0] : R.aup[t][0], ai = sp ? R.adn[t][1] : R.aup[t][1];
            if (ar == 0.0 && ai == 0.0) continue;
            const uint64_t occ = sp ? ad : au;
            if (ti == tj) {                                // number operator: diagonal
                if ((occ >> ti) & 1ULL) dg += d2{ar, ai};
                continue;
            }
            // row a of O = conj of O^dag |a>: the particle moves from ti to tj
            if (!((occ >> ti) & 1ULL) || ((occ >> tj) & 1ULL)) continue;
            if (R.no_double && (((sp ? au : ad) >> tj) & 1ULL)) continue;      // projected hopping
            const int lo_s = ti < tj ? ti : tj, hi_s = ti < tj ? tj : ti;
            const uint64_t between = ((1ULL << hi_s) - 1ULL) & ~((2ULL << lo_s) - 1ULL);
            int par = __popcll(occ & between) & 1;
            const uint64_t occ2 = occ ^ (1ULL << ti) ^ (1ULL << tj);
            const uint64_t c = sp ? (au | (occ2 << R.n_sites)) : (occ2 | (ad << R.n_sites));
            int g = 0, pt = 0;
            const uint64_t b = hubrepr_canonical(R, tab, c, &g, &pt);
            par ^= pt;
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;                       // zero-norm target
            const double f = (par ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
            // amp * conj(chi(g*)) * f
            const double cr = R.chr[2 * g], cim = -R.chr[2 * g + 1];
            const d2 v = {f * (ar * cr - ai * cim), f * (ar * cim + ai * cr)};
            row_add(cols, vals, n, kHubReprMaxRow, i, lo, v, dg);
        }
    }
    // spin exchange xa * (S+_i S-_j + S-_i S+_j): the up particle of one site and the down particle of the other trade
    // places.  S+_i S-_j = -(c^dag_{i,up} c_{j,up})(c^dag_{j,dn} c_{i,dn}): the product of the two hop signs, times -1.
    for (int e = 0; e < R.n_exch; ++e) {
        const int xi = R.xi[e], xj = R.xj[e];
        for (int dir = 0; dir < 2; ++dir) {
            const int su = dir ? xj : xi, sd = dir ? xi : xj;           // su carries the up particle, sd the down particle
            if (!((au >> su) & 1ULL) || ((ad >> su) & 1ULL) || !((ad >> sd) & 1ULL) || ((au >> sd) & 1ULL)) continue;
            const int lo_s = su < sd ? su : sd, hi_s = su < sd ? sd : su;
            const uint64_t between = ((1ULL << hi_s) - 1ULL) & ~((2ULL << lo_s) - 1ULL);
            int par = 1 ^ ((__popcll(au & between) + __popcll(ad & between)) & 1);
            const uint64_t u2 = au ^ (1ULL << su) ^ (1ULL << sd), d2w = ad ^ (1ULL << su) ^ (1ULL << sd);
            const uint64_t c = u2 | (d2w << R.n_sites);
            int g = 0, pt = 0;
            const uint64_t b = hubrepr_canonical(R, tab, c, &g, &pt);
            par ^= pt;
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;
            const double f = (par ? -1.0 : 1.0) * R.xa[e] * sqrt((double)(cj & 0x7f) / sa);
            const d2 v = {f * R.chr[2 * g], -f * R.chr[2 * g + 1]};
            row_add(cols, vals, n, kHubReprMaxRow, i, lo, v, dg);
        }
    }
    return row_finish(cols, vals, n, dg);
}

__device__ __forceinline__ int sector_row(const HubReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                          int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    return hubrepr_row(R, tab, reps, info, dim, i, cols, vals);
}

// ------------------------------------ d-level sites in translation-symmetric sectors (qbh_gen_qudit_repr) --
// Words packed as in qbh_gen_qudit (site s in bits [s b, (s+1) b), qbh_qudit.hpp), so the chunk tables of sector_symmetry
// with `bits` = b translate them and the integer order of the words is the generator's order.  Row a:
//     O[a][b] = sum over the pair entries <a|M|c> that move a to c, b = g* c:  <a|M|c> * conj(chi(g*)) * sqrt(|S_b|/|S_a|)
// (the Heisenberg convention above; no signs: bosons and spins).
constexpr int kQuditReprMaxRow = 160;     // entries of one row before merging, counted from the merged terms

struct QuditReprDev {
    int n_sites, d, bits, total, tw, n_pairs, n_trans, n_chunks;
    double chr[2 * kReprMaxTrans];
    double fake_pos;
    const uint64_t *cum;                  // [n_sites * tw], qudit_table
    const int32_t *pair_ij, *eoff, *eout; // the term tables of QuditTerms
    const double *pdiag, *sdiag;
    const d2 *eval;
};
template <> constexpr int max_row<QuditReprDev> = kQuditReprMaxRow;

inline uint64_t sector_word_count(const QuditReprDev &R, std::vector<uint64_t> &cum)    // cum: the counting table of qd_unrank
{
    std::vector<uint64_t> dims;
    qudit_table(R.n_sites, R.d, R.tw, cum, dims);
    return dims[(size_t)R.total];
}
inline int sector_tables(QuditReprDev &R, const std::vector<uint64_t> &cum, std::vector<void *> &pool)
{
    uint64_t *d_cum = nullptr;
    QBH_TRY(upload(cum, &d_cum, pool));
    R.cum = d_cum;
    return QBH_OK;
}
__device__ __forceinline__ uint64_t sector_seek(const QuditReprDev &R, uint64_t r)
{
    return qd_unrank(R.cum, R.n_sites, R.d, R.bits, R.tw, R.total, r);
}
__device__ __forceinline__ void sector_step(const QuditReprDev &R, uint64_t &cur) { cur = qd_next(cur, R.n_sites, R.d, R.bits); }

// the word a with the levels of sites si and sj replaced by those of the term entry o = l'_i | l'_j << 8
__device__ __forceinline__ uint64_t qrepr_target(uint64_t a, int bits, uint64_t field, int si, int sj, int o)
{
    return (a & ~((field << (si * bits)) | (field << (sj * bits)))) | ((uint64_t)(o & 0xff) << (si * bits)) |
           ((uint64_t)(o >> 8) << (sj * bits));
}

// the entry h = <a|M|c> of a row with |S_a| = sa whose target is carried to a representative with info byte cj by g:
// h * conj(chi(g)) * sqrt(|S_b|/|S_a|)
__device__ __forceinline__ d2 qrepr_value(const QuditReprDev &R, d2 h, int g, uint8_t cj, double sa)
{
    const double f = sqrt((double)(cj & 0x7f) / sa);
    const double cr = f * R.chr[2 * g], cim = -f * R.chr[2 * g + 1];
    return d2{h.x * cr - h.y * cim, h.x * cim + h.y * cr};
}

// one row of the sector operator into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int qrepr_row(const QuditReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                         int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double sa = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    const int d2n = R.d * R.d;
    const uint64_t field = (1ULL << R.bits) - 1ULL;
    int n = 1;
    cols[0] = (int32_t)i;
    d2 dg = {0.0, 0.0};
    for (int s = 0; s < R.n_sites; ++s) dg.x += R.sdiag[s * R.d + qd_level(a, R.bits, s)];
    for (int p = 0; p < R.n_pairs; ++p) {
        const int ij = R.pair_ij[p];
        const int si = ij & 0xff, sj = ij >> 8;
        const int in = qd_level(a, R.bits, si) * R.d + qd_level(a, R.bits, sj);
        dg.x += R.pdiag[p * d2n + in];
        const int e1 = R.eoff[p * d2n + in + 1];
        for (int e = R.eoff[p * d2n + in]; e < e1; ++e) {
            const int o = R.eout[e];
            const uint64_t c = qrepr_target(a, R.bits, field, si, sj, o);
            int g = 0;
            const uint64_t b = sector_canonical(R, tab, c, &g);
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;      // zero-norm target: dropped
            row_add(cols, vals, n, kQuditReprMaxRow, i, lo, qrepr_value(R, R.eval[e], g, cj, sa), dg);
        }
    }
    return row_finish(cols, vals, n, dg);
}

__device__ __forceinline__ int sector_row(const QuditReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                          int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    return qrepr_row(R, tab, reps, info, dim, i, cols, vals);
}

// ------------------------------------ Kondo lattice in translation-symmetric sectors (qbh_gen_kondo_repr) --
// Words w = u | d << n | s << 2n as in qbh_gen_kondo (qbh_kondo.hpp): a translation permutes the sites of all three fields,
// the two electron fields carry the fermion sign of hubrepr_parity, the local spins none.  The sector is a union of
// particle-number blocks, so the cursor keeps the rank and seeks again where a block of s ends.  Row a as in
// qbh_gen_hubbard_repr: O[a][b] = sum of <a|H|c> sigma(g*) conj(chi(g*)) sqrt(|S_b|/|S_a|), b = g* c.
struct KondoReprDev {
    KondoDev k;                           // shape, counting tables, terms
    int n_trans, n_chunks;
    double chr[2 * kReprMaxTrans];
    double fake_pos;
    int8_t perm[kReprMaxTrans * kKondoMaxSites];           // perm[g * n_sites + site]
};
template <> constexpr int max_row<KondoReprDev> = kKondoMaxRow;

inline uint64_t sector_word_count(const KondoReprDev &R, std::vector<uint64_t> &) { return R.k.total; }

struct KondoCursor { uint64_t u, d, s, ru, rd, r; };       // the three fields, the ranks of u and d in their block, the word's rank

__device__ __forceinline__ KondoCursor sector_seek(const KondoReprDev &R, uint64_t r)
{
    KondoCursor c;
    c.r = r;
    kd_unrank(R.k, R.k.A, R.k.binom, r, &c.u, &c.d, &c.s, &c.ru, &c.rd);
    return c;
}
__device__ __forceinline__ uint64_t sector_word(const KondoReprDev &R, const KondoCursor &c)
{
    return c.u | (c.d << R.k.n_sites) | (c.s << (2 * R.k.n_sites));
}
__device__ __forceinline__ void sector_step(const KondoReprDev &R, KondoCursor &c)
{
    if (c.r + 1 >= R.k.total) return;                      // the last word stays
    ++c.r;
    const int n = R.k.n_sites, nu = R.k.nu0 + __popcll(c.s);
    if (++c.ru < R.k.binom[n * kKondoTab + nu]) {
        c.u = next_same_popcount(c.u);
    } else if (++c.rd < R.k.binom[n * kKondoTab + R.k.n_elec - nu]) {      // next down pattern, up patterns start over
        c.ru = 0;
        c.u = (1ULL << nu) - 1ULL;
        c.d = next_same_popcount(c.d);
    } else {
        c = sector_seek(R, c.r);                           // the block of this s is done: the next s may lie in another block
    }
}
__device__ __forceinline__ uint64_t sector_translate(const KondoReprDev &R, const uint64_t *tab, int g, uint64_t w)
{
    const int n = R.k.n_sites;
    const uint64_t m = (1ULL << n) - 1ULL;
    return repr_translate(tab, R.n_chunks, g, w & m) | (repr_translate(tab, R.n_chunks, g, (w >> n) & m) << n) |
           (repr_translate(tab, R.n_chunks, g, w >> (2 * n)) << (2 * n));
}
// parity (0 / 1) of the permutation that sorts the images of the occupied sites of `occ` under translation g
__device__ __forceinline__ int kondo_parity(const KondoReprDev &R, int g, uint64_t occ)
{
    const int8_t *p = R.perm + g * R.k.n_sites;
    uint64_t seen = 0;
    int par = 0;
    while (occ) {
        const int i = __ffsll((long long)occ) - 1;
        occ &= occ - 1;
        const int img = p[i];
        par ^= __popcll(seen >> img) & 1;
        seen |= 1ULL << img;
    }
    return par;
}
__device__ __forceinline__ int sector_parity(const KondoReprDev &R, int g, uint64_t w)
{
    const uint64_t m = (1ULL << R.k.n_sites) - 1ULL;
    return kondo_parity(R, g, w & m) ^ kondo_parity(R, g, (w >> R.k.n_sites) & m);
}

// the entry of a row with |S_a| = sa from the code of kd_row_terms, when translation g with sign parity pt carries the target
// to a representative with info byte cj: <a|H|c> sigma(g*) conj(chi(g*)) sqrt(|S_b|/|S_a|).  The one expression of the stored
// rows (kondo_row) and of the matrix-free apply (qbh_sector_mf_kondo.hip).
__device__ __forceinline__ d2 kondo_repr_value(const KondoReprDev &R, int code, int g, int pt, uint8_t cj, double sa)
{
    const double f = (pt ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
    const d2 h = kd_value(R.k, code);
    const double cr = f * R.chr[2 * g], cim = -f * R.chr[2 * g + 1];
    return d2{h.x * cr - h.y * cim, h.x * cim + h.y * cr};
}

// one row of the sector operator into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int kondo_row(const KondoReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                         int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double sa = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    const int nb = R.k.n_sites;
    const uint64_t mlow = (1ULL << nb) - 1ULL;
    int n = 1;
    cols[0] = (int32_t)i;
    d2 off = {0.0, 0.0};                  // what the moves add to the diagonal (a word that comes back to its own orbit)
    const d2 dg0 = kd_row_terms(R.k, a & mlow, (a >> nb) & mlow, a >> (2 * nb), [&](uint64_t u2, uint64_t d2w, uint64_t s2, int code) {
        const uint64_t c = u2 | (d2w << nb) | (s2 << (2 * nb));
        int g = 0;
        const uint64_t b = sector_canonical(R, tab, c, &g);
        const int pt = g ? sector_parity(R, g, c) : 0;
        const int64_t lo = sector_find(reps, dim, b);
        const uint8_t cj = info[lo];
        if (cj & 0x80) return;            // zero-norm target: dropped
        row_add(cols, vals, n, kKondoMaxRow, i, lo, kondo_repr_value(R, code, g, pt, cj, sa), off);
    });
    return row_finish(cols, vals, n, dg0 + off);
}

__device__ __forceinline__ int sector_row(const KondoReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                          int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    return kondo_row(R, tab, reps, info, dim, i, cols, vals);
}

// ------------------------------------ the enumeration and the row kernels every family shares --
// The basis of a sector is ALL orbit representatives (the smallest word of each orbit) of the family's words, ascending; a
// representative whose (signed) character sum over its stabiliser vanishes has zero norm at this momentum and stays in the
// basis as a decoupled fake row (row_zero_norm).  Two passes over the words in ascending order, one workgroup per chunk of
// kSectorChunk consecutive words, a lane seeking the first of its kSectorRun words and stepping from there.  Nothing is
// kept per word besides one code byte (4x5 Hubbard at half filling has 3.4e10 words): the counts are per chunk.
constexpr int kSectorRun = 16, kSectorChunk = kSectorRun * 256;

// position of representative b in reps[0, dim) through the directory of the enumeration (sector_enumerate's chunk_pos):
// rank_of_b, the rank of b among the family's words, names its chunk of kSectorChunk words; the directory gives the
// positions of that chunk's first and last representatives, and a bisection of at most 12 steps ends among them.  b is a
// representative, so this is sector_find(reps, dim, b); the result stays below dim for any word.
static_assert(kSectorChunk == 1 << 12, "sector_dir_find shifts a rank by 12 bits to its chunk");
__device__ __forceinline__ int64_t sector_dir_find(const uint64_t *reps, const int64_t *chunk_pos, int64_t dim, uint64_t b, uint64_t rank_of_b)
{
    const uint64_t c = rank_of_b >> 12;
    int64_t lo = chunk_pos[c], hi = chunk_pos[c + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (reps[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo < dim ? lo : dim - 1;
}

// host tail of the matrix-free sector creators: launch(d_part) starts a count kernel on the null stream that leaves one sum per
// workgroup in d_part[0, cgrid) and returns its launch error; *total = the sum of them
template <class Launch>
int sector_count_entries(const char *who, int cgrid, int64_t *total, Launch launch)
{
    unsigned long long *d_part = nullptr;
    QBH_HIP_WHO(who, qbh::dev_alloc(&d_part, (size_t)cgrid * sizeof(unsigned long long)));
    hipError_t ce = launch(d_part);
    std::vector<unsigned long long> part((size_t)cgrid);
    if (ce == hipSuccess) ce = hipMemcpy(part.data(), d_part, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d_part);
    QBH_HIP_WHO(who, ce);
    *total = 0;
    for (unsigned long long v : part) *total += (int64_t)v;
    return QBH_OK;
}

// pass 1: code[r] = 0 if the word of rank r is not a representative, else |S| | (zero-norm << 7); chunk_cnt = the number of
// representatives of each chunk
template <class Dev>
__global__ __launch_bounds__(256) void k_sector_flag(const Dev *Rp, const uint64_t *tab, int64_t nstates, uint8_t *code,
                                                     int32_t *chunk_cnt, int64_t nchunks)
{
    const Dev &R = *Rp;
    __shared__ int wsum[4];
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t r0 = chunk * kSectorChunk + (int64_t)threadIdx.x * kSectorRun;
        const int64_t r1 = (r0 + kSectorRun < nstates) ? r0 + kSectorRun : nstates;
        int mine = 0;
        if (r0 < nstates) {
            auto cur = sector_seek(R, (uint64_t)r0);
            for (int64_t r = r0; r < r1; ++r) {
                const uint64_t s = sector_word(R, cur);
                bool rep = sector_allowed(R, s);
                int nstab = 1;
                double sr = R.chr[0], si = R.chr[1];
                for (int g = 1; rep && g < R.n_trans; ++g) {
                    const uint64_t t = sector_translate(R, tab, g, s);
                    if (t < s) {
                        rep = false;
                        break;
                    }
                    if (t == s) {
                        const double sg = sector_parity(R, g, s) ? -1.0 : 1.0;
                        nstab++;
                        sr += sg * R.chr[2 * g];
                        si += sg * R.chr[2 * g + 1];
                    }
                }
                code[r] = rep ? (uint8_t)(nstab | ((sr * sr + si * si < 1e-20) ? 0x80 : 0)) : 0;
                mine += rep ? 1 : 0;
                sector_step(R, cur);
            }
        }
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) chunk_cnt[chunk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// pass 2: the representatives of a chunk go to reps[chunk_pos[chunk] ...] in ascending order, their codes to info[].  Every
// lane takes every barrier of every chunk; only the walk through its own run depends on what the lane found.
template <class Dev>
__global__ __launch_bounds__(256) void k_sector_compact(const Dev *Rp, int64_t nstates, const uint8_t *code, const int64_t *chunk_pos,
                                                        int64_t nchunks, uint64_t *reps, uint8_t *info)
{
    const Dev &R = *Rp;
    __shared__ int scan[256];
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t r0 = chunk * kSectorChunk + (int64_t)threadIdx.x * kSectorRun;
        const int64_t r1 = (r0 + kSectorRun < nstates) ? r0 + kSectorRun : nstates;
        int mine = 0;
        for (int64_t r = r0; r < r1; ++r) mine += code[r] ? 1 : 0;
        __syncthreads();
        scan[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {          // inclusive Hillis-Steele scan
            const int v = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        if (mine > 0) {                                    // then r0 < nstates, and the walk ends at the lane's last one
            int64_t at = chunk_pos[chunk] + scan[threadIdx.x] - mine;
            auto cur = sector_seek(R, (uint64_t)r0);
            for (int64_t r = r0; mine > 0; ++r) {
                if (code[r]) {
                    reps[at] = sector_word(R, cur);
                    info[at] = code[r];
                    ++at;
                    --mine;
                }
                sector_step(R, cur);
            }
        }
    }
}

// row lengths of rows [r0, r1); with T.fp != nullptr the distinct values met on the way are collected for the value
// dictionary, so that the fill pass can emit 1- or 2-byte codes and the 16 B/nnz value array never exists
template <class Dev>
__global__ __launch_bounds__(128) void k_sector_count(const Dev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                      int64_t dim, int64_t r0, int64_t r1, int32_t *cnt, DictTab T)
{
    __shared__ DictCollect D;
    int32_t cols[max_row<Dev>];
    d2 vals[max_row<Dev>];
    bool collect = T.fp != nullptr;
    if (T.fp != nullptr) dict_collect_init(D);
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = r0 + (int64_t)blockIdx.x * 128 + threadIdx.x; i < r1; i += stride) {
        const int m = sector_row(*Rp, tab, reps, info, dim, i, cols, vals);
        cnt[i - r0] = m;
        for (int q = 0; collect && q < m; ++q) collect = dict_collect_insert(D, T, vals[q]);
    }
}

// ia is local to the shard (ia[0] = 0 at row r0)
template <class Dev>
__global__ __launch_bounds__(128) void k_sector_fill(const Dev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                     int64_t dim, int64_t r0, int64_t r1, const int64_t *ia, int32_t *ja, d2 *val)
{
    int32_t cols[max_row<Dev>];
    d2 vals[max_row<Dev>];
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = r0 + (int64_t)blockIdx.x * 128 + threadIdx.x; i < r1; i += stride) {
        const int m = sector_row(*Rp, tab, reps, info, dim, i, cols, vals);
        const int64_t p0 = ia[i - r0];
        for (int q = 0; q < m; ++q) {
            ja[p0 + q] = cols[q];
            val[p0 + q] = vals[q];
        }
    }
}

template <class Dev, typename CT>
__global__ __launch_bounds__(128) void k_sector_fill_coded(const Dev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                           int64_t dim, int64_t r0, int64_t r1, const int64_t *ia, int32_t *ja, CT *code,
                                                           const d2 *dict, DictTab T)
{
    __shared__ DictEncode E;
    int32_t cols[max_row<Dev>];
    d2 vals[max_row<Dev>];
    dict_encode_init(E);
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = r0 + (int64_t)blockIdx.x * 128 + threadIdx.x; i < r1; i += stride) {
        const int m = sector_row(*Rp, tab, reps, info, dim, i, cols, vals);
        const int64_t p0 = ia[i - r0];
        for (int q = 0; q < m; ++q) {
            ja[p0 + q] = cols[q];
            code[p0 + q] = (CT)dict_encode_one(E, T, dict, vals[q]);
        }
    }
}

// number of words of the sector, refused beyond what one code byte per word can enumerate; ctab as in sector_word_count
template <class Dev>
int sector_words(const Dev &R, std::vector<uint64_t> &ctab, int64_t *nstates, const char *who)
{
    const uint64_t n = sector_word_count(R, ctab);
    if (n >= (1ULL << 40)) {
        set_error("%s: sector too large to enumerate", who);
        return QBH_EUNSUPP;
    }
    *nstates = (int64_t)n;
    return QBH_OK;
}

// a sector on the device: the family's struct, the translation tables, the representatives and their info bytes
template <class Dev>
struct SectorDev {
    Dev *R = nullptr;
    uint64_t *tab = nullptr, *reps = nullptr;
    uint8_t *info = nullptr;          // |S| | zero-norm << 7
    int64_t dim = 0;
};

// enumerates the sector described by R (its term pointers already set, or unused); everything in S joins `pool`.  With
// chunk_pos_out the directory of the enumeration is kept in the pool as well: chunk_pos[c] = the position of the first
// representative among the words of ranks [c * kSectorChunk, (c + 1) * kSectorChunk), nchunks + 1 entries, the last one dim.
template <class Dev>
int sector_enumerate(const Dev &R, const std::vector<uint64_t> &tab, std::vector<void *> &pool, SectorDev<Dev> &S, const char *who,
                     int64_t **chunk_pos_out = nullptr, int64_t *nchunks_out = nullptr)
{
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));
    std::vector<Dev> rr(1, R);
    QBH_TRY(sector_tables(rr[0], ctab, pool));
    QBH_TRY(upload(rr, &S.R, pool));
    QBH_TRY(upload(tab, &S.tab, pool));
    const int64_t nchunks = (nstates + kSectorChunk - 1) / kSectorChunk;
    const int egrid = (int)std::min<int64_t>(nchunks, 256 * 32);
    DevBufs tmp;
    uint8_t *d_code = nullptr;
    int32_t *d_cnt = nullptr;
    int64_t *d_pos = nullptr;
    QBH_HIP_WHO(who, tmp.alloc(&d_code, (size_t)nstates));
    QBH_HIP_WHO(who, tmp.alloc(&d_cnt, (size_t)nchunks * sizeof(int32_t)));
    if (chunk_pos_out) {
        QBH_HIP_WHO(who, qbh::dev_alloc(&d_pos, (size_t)(nchunks + 1) * sizeof(int64_t)));
        pool.push_back(d_pos);
        *chunk_pos_out = d_pos;
        if (nchunks_out) *nchunks_out = nchunks;
    } else {
        QBH_HIP_WHO(who, tmp.alloc(&d_pos, (size_t)(nchunks + 1) * sizeof(int64_t)));
    }
    hipLaunchKernelGGL(k_sector_flag<Dev>, dim3(egrid), dim3(256), 0, 0, S.R, S.tab, nstates, d_code, d_cnt, nchunks);
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_TRY(exclusive_scan(d_cnt, nchunks, d_pos, 0));
    QBH_HIP_WHO(who, hipMemcpy(&S.dim, d_pos + nchunks, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (S.dim <= 0 || S.dim >= 2147483647LL) {         // row and column indices are int32
        set_error("%s: sector dimension %lld out of range", who, (long long)S.dim);
        return QBH_EUNSUPP;
    }
    QBH_HIP_WHO(who, qbh::dev_alloc(&S.reps, (size_t)S.dim * sizeof(uint64_t)));
    pool.push_back(S.reps);
    QBH_HIP_WHO(who, qbh::dev_alloc(&S.info, (size_t)S.dim));
    pool.push_back(S.info);
    hipLaunchKernelGGL(k_sector_compact<Dev>, dim3(egrid), dim3(256), 0, 0, S.R, nstates, d_code, d_pos, nchunks, S.reps, S.info);
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    return QBH_OK;
}

// R zeroed, then the symmetry part of the fixed-n_dn spin sector filled in (bonds and fake_pos are the caller's)
inline int repr_symmetry(ReprDev &R, std::vector<uint64_t> &tab, int n_sites, int n_dn, int n_trans, const int32_t *perms,
                  const double *chars, const char *who)
{
    memset(&R, 0, sizeof(R));
    R.h.n_sites = n_sites;
    R.h.n_dn = n_dn;
    R.n_trans = n_trans;
    return sector_symmetry(n_sites, n_trans, perms, chars, who, R.h.binom, R.chr, nullptr, R.n_chunks, tab);
}

// R zeroed, then the symmetry part of the (n_up, n_dn) sector filled in (the operator's terms are the caller's)
inline int hubrepr_symmetry(HubReprDev &R, std::vector<uint64_t> &tab, int n_sites, int n_up, int n_dn, int n_trans, const int32_t *perms,
                     const double *chars, const char *who)
{
    memset(&R, 0, sizeof(R));
    R.n_sites = n_sites;
    R.n_up = n_up;
    R.n_dn = n_dn;
    R.n_trans = n_trans;
    return sector_symmetry(n_sites, n_trans, perms, chars, who, R.binom, R.chr, R.perm, R.n_chunks, tab);
}

// one-body terms amp * c^dag_i c_j merged on the same (i, j): (up re, up im, dn re, dn im)
using TermMap = std::map<std::pair<int, int>, std::array<double, 4>>;

// merges the terms and refuses what hubrepr_row would silently truncate: a row holds at most one move per unordered site
// pair and species, one per spin-exchange term, and the diagonal
inline int merge_terms(int n_sites, int n_terms, const int32_t *term_sites, const qbh_z *amp_up, const qbh_z *amp_dn, int n_exch,
                const char *who, TermMap &tmap)
{
    for (int t = 0; t < n_terms; ++t) {
        const int i = term_sites[2 * t], j = term_sites[2 * t + 1];
        if (i < 0 || i >= n_sites || j < 0 || j >= n_sites) {
            set_error("%s: term %d acts on a site outside the lattice", who, t);
            return QBH_EINVAL;
        }
        auto &a = tmap[{i, j}];
        a[0] += amp_up[t].re;
        a[1] += amp_up[t].im;
        a[2] += amp_dn[t].re;
        a[3] += amp_dn[t].im;
    }
    std::map<std::pair<int, int>, int> pairs;
    for (const auto &kv : tmap)
        if (kv.first.first != kv.first.second) pairs[{std::min(kv.first.first, kv.first.second), std::max(kv.first.first, kv.first.second)}] = 1;
    if ((int)tmap.size() > kHubReprMaxTerms || 2 * (int)pairs.size() + n_exch + 1 > kHubReprMaxRow) {
        set_error("%s: too many distinct one-body terms (%d on %d site pairs)", who, (int)tmap.size(), (int)pairs.size());
        return QBH_EUNSUPP;
    }
    return QBH_OK;
}

// R zeroed, then the symmetry part of the d-level sector of charge `total` filled in (the terms are the caller's)
inline int qrepr_symmetry(QuditReprDev &R, std::vector<uint64_t> &tab, int n_sites, int d, int total, int n_trans, const int32_t *perms,
                   const double *chars, const char *who)
{
    memset(&R, 0, sizeof(R));
    R.n_sites = n_sites;
    R.d = d;
    R.bits = bits_per_level(d);
    R.total = total;
    R.tw = total + 1;
    R.n_trans = n_trans;
    return sector_symmetry(n_sites, n_trans, perms, chars, who, nullptr, R.chr, nullptr, R.n_chunks, tab, R.bits);
}

// the sector matrix is only right for an operator that commutes with every translation: the pair on (g(i), g(j)) must carry
// the matrix of (i, j) (transposed when g swaps the order) and the single-site diagonals of s and g(s) must agree
inline int qrepr_invariant(const QuditTerms &T, int n_sites, int d, int n_trans, const int32_t *perms, const char *who)
{
    const int d2n = d * d;
    const std::vector<std::complex<double>> zero((size_t)d2n * d2n, 0.0);
    auto close = [](std::complex<double> x, std::complex<double> y) {
        return std::abs(x - y) <= QBH_SPARSE_PRECISION * std::max(1.0, std::max(std::abs(x), std::abs(y)));
    };
    for (int g = 1; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * n_sites;
        for (const auto &kv : T.pm) {
            const int gi = pg[kv.first.first], gj = pg[kv.first.second];
            const auto it = T.pm.find({std::min(gi, gj), std::max(gi, gj)});
            const std::vector<std::complex<double>> &img = it == T.pm.end() ? zero : it->second;
            for (int r = 0; r < d2n; ++r)
                for (int c = 0; c < d2n; ++c) {
                    const int rr = gi < gj ? r : (r % d) * d + r / d, cc = gi < gj ? c : (c % d) * d + c / d;
                    if (!close(kv.second[(size_t)r * d2n + c], img[(size_t)rr * d2n + cc])) {
                        set_error("%s: the terms are not invariant under translation %d: pair (%d, %d) and its image (%d, %d) differ",
                                  who, g, kv.first.first, kv.first.second, gi, gj);
                        return QBH_EINVAL;
                    }
                }
        }
        for (int s = 0; s < n_sites; ++s)
            for (int l = 0; l < d; ++l)
                if (!close(T.sdiag[(size_t)s * d + l], T.sdiag[(size_t)pg[s] * d + l])) {
                    set_error("%s: the single-site terms are not invariant under translation %d: site %d and its image %d differ", who,
                              g, s, pg[s]);
                    return QBH_EINVAL;
                }
    }
    return QBH_OK;
}

// "the coefficients transform with a character": c_{g(s)} = eta(g) c_s in every one of the n_sets coefficient sets, with one
// eta for all of them.  eta(g) is read off the coefficient of largest magnitude (the first one on ties; eta = 1 if all
// vanish), then every set is checked on every site.  perms must be validated already (the family's *_symmetry does it).
inline int coef_character(const char *who, int n_sites, int n_trans, const int32_t *perms, const qbh_z *const *sets, int n_sets,
                          std::complex<double> *eta_out)
{
    auto at = [&](int q, int s) { return std::complex<double>(sets[q][s].re, sets[q][s].im); };
    int q0 = 0, s0 = 0;
    double best = 0.0;
    for (int q = 0; q < n_sets; ++q)
        for (int s = 0; s < n_sites; ++s)
            if (std::abs(at(q, s)) > best) {
                best = std::abs(at(q, s));
                q0 = q;
                s0 = s;
            }
    for (int g = 0; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * n_sites;
        const std::complex<double> eta = best > 0.0 ? at(q0, pg[s0]) / at(q0, s0) : 1.0;
        for (int q = 0; q < n_sets; ++q)
            for (int s = 0; s < n_sites; ++s)
                if (std::abs(at(q, pg[s]) - eta * at(q, s)) > 1e-10 * std::max(1.0, best)) {
                    set_error("%s: the coefficients do not transform with a character under translation %d (set %d, site %d)", who, g,
                              q, s);
                    return QBH_EINVAL;
                }
        if (eta_out) eta_out[g] = eta;
    }
    return QBH_OK;
}

}  // namespace
}  // namespace qbh

// ------------------------------ stored sector operators: qbh_gen_heisenberg_repr, qbh_gen_hubbard_repr --
// row range of shard `shard`: the uniform partition of qbh_comm, or the caller's cuts (nnz- or cost-balanced)
static inline int sector_row_range(const char *who, int64_t dim, int shard, int n_shards, const int64_t *row_cuts, int64_t *r0, int64_t *r1)
{
    if (row_cuts) {
        bool ok = row_cuts[0] == 0 && row_cuts[n_shards] == dim;
        for (int q = 0; q < n_shards && ok; ++q) ok = row_cuts[q + 1] >= row_cuts[q];
        if (!ok) {
            qbh::set_error("%s: row_cuts must rise from 0 to the sector dimension %lld", who, (long long)dim);
            return QBH_EINVAL;
        }
        *r0 = row_cuts[shard];
        *r1 = row_cuts[shard + 1];
    } else {
        const int64_t nblk = (dim + n_shards - 1) / n_shards;
        *r0 = std::min<int64_t>((int64_t)shard * nblk, dim);
        *r1 = std::min<int64_t>(*r0 + nblk, dim);
    }
    return QBH_OK;
}

// this shard's rows of a sector operator: lengths (+ the distinct values) -> row pointers -> coded or uncoded fill, adopted
// into *out.  `pool` holds the caller's tables and representatives; it is released before the handle takes the arrays.
template <class Dev>
static int assemble_sector_rows(const char *who, std::vector<void *> &pool, const Dev *d_R, const uint64_t *d_tab,
                                const uint64_t *d_reps, const uint8_t *d_info, int64_t dim, int shard, int n_shards,
                                const int64_t *row_cuts, const qbh_opts *opts, qbh_csr **out, int64_t *dim_out)
{
    using namespace qbh;
    if (dim >= 2147483647LL) {            // column indices are int32
        set_error("%s: sector dimension %lld out of range", who, (long long)dim);
        return QBH_EUNSUPP;
    }
    int64_t r0 = 0, r1 = 0;
    QBH_TRY(sector_row_range(who, dim, shard, n_shards, row_cuts, &r0, &r1));
    const int64_t nloc = r1 - r0;
    if (nloc <= 0) {
        set_error("%s: shard %d of %d is empty (dim %lld)", who, shard, n_shards, (long long)dim);
        return QBH_EINVAL;
    }
    DictBuild db;
    std::unique_ptr<DictBuild, void (*)(DictBuild *)> db_end(&db, dict_build_end);
    const bool want_dict = !opts || opts->value_dict;
    if (want_dict) {
        const bool rows_kernel = !opts || opts->spmv_kernel == QBH_KERNEL_AUTO || opts->spmv_kernel == QBH_KERNEL_ROWS;
        QBH_TRY(dict_build_begin(&db, (opts && opts->value_dict == 2) || !rows_kernel ? 256 : kDictMax, 0));
    }
    DevBufs csr;                          // the operator's arrays until the handle adopts them
    int64_t *d_ia = nullptr;
    int32_t *d_ja = nullptr;
    uint8_t *d_code = nullptr;
    d2 *d_val = nullptr, *d_dict = nullptr;
    const int rgrid = (int)std::min<int64_t>((nloc + 127) / 128, 256 * 16);
    int64_t nnz = 0;
    {
        DevBufs tmp;
        int32_t *d_cnt = nullptr;
        QBH_HIP_WHO(who, tmp.alloc(&d_cnt, (size_t)nloc * sizeof(int32_t)));
        QBH_HIP_WHO(who, csr.alloc(&d_ia, (size_t)(nloc + 1) * sizeof(int64_t)));
        hipLaunchKernelGGL(k_sector_count<Dev>, dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1, d_cnt, db.tab);
        QBH_HIP_WHO(who, hipGetLastError());
        QBH_TRY(exclusive_scan(d_cnt, nloc, d_ia, 0));
        QBH_HIP_WHO(who, hipMemcpy(&nnz, d_ia + nloc, sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    QBH_HIP_WHO(who, csr.alloc(&d_ja, (size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
    int n_dict = 0;
    if (want_dict) {
        QBH_TRY(dict_build_finalize(&db, &d_dict, &n_dict, 0));
        if (d_dict) csr.pool.push_back(d_dict);
    }
    if (n_dict > 0) {
        // few distinct values (amplitudes x signs x phases x square roots of stabiliser ratios): 1- or 2-byte codes are
        // emitted directly (5 or 6 B/nnz instead of 20)
        const int w = dict_code_width(n_dict);
        QBH_HIP_WHO(who, csr.alloc(&d_code, (size_t)nnz * w + 16));
        QBH_HIP_WHO(who, hipMemset(d_code + (size_t)nnz * w, 0, 16));
        if (w == 1)
            hipLaunchKernelGGL((k_sector_fill_coded<Dev, uint8_t>), dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1,
                               d_ia, d_ja, d_code, d_dict, db.tab);
        else
            hipLaunchKernelGGL((k_sector_fill_coded<Dev, uint16_t>), dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1,
                               d_ia, d_ja, reinterpret_cast<uint16_t *>(d_code), d_dict, db.tab);
        QBH_HIP_WHO(who, hipGetLastError());
        int bad = 0;
        QBH_TRY(dict_build_mismatch(&db, &bad, 0));
        if (bad) {
            set_error("%s: value dictionary mismatch between the count and fill passes", who);
            return QBH_EHIP;
        }
    } else {
        const hipError_t e = csr.alloc(&d_val, (size_t)std::max<int64_t>(nnz, 1) * sizeof(d2));
        if (e == hipErrorOutOfMemory) {
            set_error("%s: %lld nonzeros with more than 65536 distinct values do not fit this GPU uncoded (%.1f GB); shard the "
                      "sector over more GPUs", who, (long long)nnz, 20e-9 * (double)nnz);
            (void)hipGetLastError();
            return QBH_ENOMEM;
        }
        QBH_HIP_WHO(who, e);
        hipLaunchKernelGGL(k_sector_fill<Dev>, dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1, d_ia, d_ja, d_val);
        QBH_HIP_WHO(who, hipGetLastError());
    }
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    free_pool(pool);
    db_end.reset();
    csr.release();                        // ownership passes with the call: on failure the arrays have already been released
    if (dim_out) *dim_out = dim;
    if (d_code) return adopt_coded_csr(out, nloc, dim, r0, nnz, d_ia, d_ja, d_code, d_dict, n_dict, opts);
    qbh_opts og;
    opts_generated(opts, &og);
    return qbh_csr_create_device(out, nloc, dim, r0, nnz, d_ia, d_ja, reinterpret_cast<qbh_z *>(d_val), 1, &og);
}

// the symmetry part of a Kondo sector on top of R.k (shape and terms already in place)
static inline int kondo_symmetry(qbh::KondoReprDev &R, std::vector<uint64_t> &tab, int n_trans, const int32_t *perms, const double *chars,
                          const char *who)
{
    using namespace qbh;
    if (!perms || !chars || n_trans < 1) {
        set_error("%s: invalid symmetry argument", who);
        return QBH_EINVAL;
    }
    if (n_trans > kReprMaxTrans) {
        set_error("%s: %d translations; at most %d are supported", who, n_trans, kReprMaxTrans);
        return QBH_EUNSUPP;
    }
    R.n_trans = n_trans;
    return sector_symmetry(R.k.n_sites, n_trans, perms, chars, who, nullptr, R.chr, R.perm, R.n_chunks, tab);
}
