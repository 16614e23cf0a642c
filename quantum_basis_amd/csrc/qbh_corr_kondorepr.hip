// qbh_corr_kondorepr.hip -- qbh_corr_kondo_repr_dev: all-pair static correlations of a Kondo-lattice state held in a MOMENTUM
// SECTOR (basis of qbh_gen_kondo_repr / qbh_mf_kondo_repr: all orbit representatives of the words u | d << n | s << 2n,
// ascending), in one pass over the representatives.  The result is what qbh_corr_kondo_dev returns on the unfolded state.
//
// With T_g |u, d, s> = sgn(g, u) sgn(g, d) |g(u), g(d), g(s)> (no sign from the local spins), |a, k> = (|G| |S_a|)^(-1/2) sum_g
// chi(g) T_g |a>, Psi = sum_a psi_a |a, k> (representatives of zero norm left out, their entries never read), w_a = |psi_a|^2:
//   norm2          = sum_a w_a
//   site[c][i]     = sum_a w_a (1/|G|) sum_g f_c(g(i))(a),   f = n_up, n_dn, n_up n_dn, S^z (+1/2 where the bit of s is clear)
//   nn[2A+B][i][j] = sum_a w_a (1/|G|) sum_g n_{g(i),A}(a) n_{g(j),B}(a)
//   zn[B][i][j]    = sum_a w_a (1/|G|) sum_g S^z_{g(i)}(a) n_{g(j),B}(a)            zz[i][j] likewise with S^z_{g(i)} S^z_{g(j)}
//   X[i][j]        = (1/|G|) sum_a sum_{g: <a| X_{g(i) g(j)} |c> != 0} conj(psi_a) <a|X|c> v psi_b      for the gathered groups
//       v = sigma(g*) conj(chi(g*)) sqrt(|S_b| / |S_a|),  T_{g*} |c> = sigma |b>;  a target b of zero norm is skipped
//     hop[s]  c+_{i,s} c_{j,s}       a: i occupied, j empty in s; c: the particle on j;  sign (-1)^(particles of s between)
//     ee      s^+_i s^-_j            a: i up-only, j down-only; c: the two trade places;  sign -(-1)^(particles of both between)
//     ll      S^+_i S^-_j            a: local spin i up, j down; c: both turned;  no sign
//     le      S^+_i s^-_j            a: local spin i up, j down-only; c: local spin i down, j up-only -- c lies in the block
//                                    popcount(s) + 1, n_up + 1 of the sector;  sign of s^-_j as in kd_row_terms;  i = j included
// the entries of kondo_row / kondo_repr_value for the one-term operator, averaged over the group.  Nothing is divided by norm2.
//
// The sums over g only see the IMAGE of (i, j).  A row walks site pairs once and adds what it finds to the accumulators of
//   the pair's CLASS (qbh_corr_repr.hpp: an orbit of ordered pairs with its mirror image, n_u unordered pairs) for the groups that
//     are Hermitian in (i, j): nn as in qbh_corr_hubrepr.hip (UU, DD, F, B);  zz: Z = sum_a w_a (#pairs with equal local spins -
//     #pairs with unequal ones), zz = Z / (4 n_u);  hop, ee, ll: C = the term of the pair's one orientation if that orientation is
//     forward, its conjugate if not, value = C / (2 n_u) forward, its conjugate backward, real for a class that is its own mirror;
//   the pair's ORBIT OF ORDERED PAIRS (repr_ordered_orbits, the diagonal pairs (i, i) included, n_o pairs) for zn and le, which are
//     not Hermitian: ZU, ZD = sum_a w_a sum_{(p, q) in orbit} (1 - 2 s_p) n_{q,up / dn}, zn = ZU / (2 n_o);  le = L / n_o;
//   the site's orbit (n_s sites): U, D, UD = sum_a w_a popcount(u & orbit), ..., SZ = sum_a w_a (n_s - 2 popcount(s & orbit)),
//     site = U / n_s, D / n_s, UD / n_s, SZ / (2 n_s).
// The host fills the diagonals as qbh_corr_kondo_dev does: nn[i][i] = n_up, docc, docc, n_dn;  zz[i][i] = norm2 / 4;
// hop[s][i][i] = site[s][i];  ee[i][i] = n_up - docc;  ll[i][i] = norm2 / 2 + S^z.  The diagonal groups cost no gather.
//
// Gathers: one per row and unordered pair with the allowed pattern (hop per species, ee, ll), one per ordered pair (local spin up,
// down-only site) for le.  A candidate is canonicalised with the byte-sliced translation tables (three fields), the parity of
// T_{g*} comes from the permutation bytes of the two electron fields, b is ranked with the counting tables (kd_rank: all three
// fields, so a target in another block of the sector is found like any other) and located through the directory of the
// enumeration (sector_dir_find).
//
// Launches: one per kind that is asked for, a grid of (row blocks) x (passes), one lane per representative, grid-stride over a
// resident grid, kKrAcc = 16 accumulators per pass indexed by compile-time constants only:
//   DIAG  no gather; the sub-kind is uniform over the workgroup
//           SITE  3 site orbits:  [g] U, [3+g] D, [6+g] UD, [9+g] SZ, [15] norm2 (read from the first site pass)
//           NN    4 classes:  [g] UU, [4+g] DD, [8+g] F, [12+g] B
//           ZN    8 ordered orbits:  [g] ZU, [8+g] ZD
//           ZZ    16 classes:  [g] Z
//   HOP (species uniform per pass), EE, LL  8 classes:  [g] Re C, [8+g] Im C (complex vectors only)
//   LE    8 ordered orbits:  [g] Re L, [8+g] Im L
// A group that is not asked for has no passes and no launch, so the other outputs keep their bits.  Every workgroup leaves its
// sums at partials[blockIdx.x][pass][accumulator] (corr_block_partials) and k_corr_reduce adds the workgroups in a fixed order
// (corr_reduce_launch): no atomics, two calls return the same bits.
//
// Tables.  Translation tables, A, binom, characters and permutation bytes are dynamic LDS: at most 138,816 + 1024 + 1344 B =
// 141,184 B (64 translations of 21 sites) <= kCorrLdsCap, so there is no global-memory table path.  The footprint chooses between
// workgroups of 256 lanes (four or more fit a CU) and one of 1024 (repr_launch_shape).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), 0 bytes of scratch in every instance; the static LDS is
// the reduction scratch (512 B at 256 lanes, 2048 B at 1024), the tables are dynamic LDS on top of it:
//   k_corr_kondorepr<vector, kind>     VGPRs at 256 / 1024 lanes  SGPRs  wavefronts/SIMD  scratch
//   <complex, DIAG>                          94 /  94              106         5            0
//   <complex, HOP>                          108 / 108              104         4            0
//   <complex, EE>                           110 / 110               99         4            0
//   <complex, LL>                           110 / 110              103         4            0
//   <complex, LE>                           104 / 104               94         4            0
//   <real,    DIAG>                          92 /  92              106         5            0
//   <real,    HOP>                           72 /  70              101         7            0
//   <real,    EE>                            76 /  74               97         6            0
//   <real,    LL>                            76 /  74               96         6            0
//   <real,    LE>                            72 /  70               94         7            0
// At most 110 VGPRs: every instance keeps the four wavefronts per SIMD that a workgroup of 1024 lanes needs (128 at most).
#include <algorithm>
#include <vector>

#include "qbh_kondo_lds.hpp"                                 // qbh_sector.hpp, kKondoTabEntries, kMfKreprLdsMax
#include "qbh_device.hpp"
#include "qbh_corr.hpp"                                      // device helpers, launch path, pass layout and host fills
#include "qbh_corr_repr.hpp"                                 // classes and orbits of site pairs, symmetry checks

namespace qbh {
namespace {

constexpr int kKrAcc = 16;                                   // accumulators of a pass
constexpr int kKrSite = 3, kKrNN = 4, kKrZN = 8, kKrZZ = 16, kKrGat = 8;     // site orbits / classes / ordered orbits of a pass
enum { kKrDiag = 0, kKrHop = 1, kKrEE = 2, kKrLL = 3, kKrLE = 4, kKrKinds = 5 };
enum { kKrSubSite = 0, kKrSubNN = 1, kKrSubZN = 2, kKrSubZZ = 3, kKrSubs = 4 };
constexpr size_t kKrLdsMax = kMfKreprLdsMax + (2 * (size_t)kReprMaxTrans + (size_t)kReprMaxTrans * kKondoMaxSites / 8) * 8;
static_assert(kKrLdsMax == 141184 && kKrLdsMax <= kCorrLdsCap, "the tables of every admissible sector fit LDS");

// The pair words of class c are pairs[cls_start[c] .. cls_start[c + 1]), those of ordered orbit o opairs[orb_start[o] ..
// orb_start[o + 1]) (qbh_corr_repr.hpp); both start arrays are padded with the total beyond the last entry, so a pass reads the
// bounds of its whole group without a check.  Site pass sp owns the site orbits sp * kKrSite ... with the masks site_mask[..]
// (0 past the last orbit).
struct CorrKondoRepr {
    const KondoReprDev *R;                                   // counting tables, characters, permutation bytes (staged in LDS)
    const uint64_t *tab, *reps;
    const uint8_t *info;
    const int64_t *chunk_pos;
    int64_t dim;
    int n_tab, n_sites, n_trans, n_chunks;
    int sub_end[kKrSubs];                                    // DIAG: passes [sub_end[k - 1], sub_end[k]) are of sub-kind k
    int hop_passes;                                          // HOP: passes of one species (up first)
    const int32_t *cls_start, *orb_start;
    const uint32_t *pairs, *opairs;
    const uint64_t *site_mask;
    const d2 *xg;                                            // exactly one of xg / xr
    const double *xr;
    double *partials;
};

template <bool REALX, int BLOCK, int KIND>
__global__ __launch_bounds__(BLOCK) void k_corr_kondorepr(CorrKondoRepr t)
{
    constexpr int NA = kKrAcc, GH = kKrGat;
    extern __shared__ __attribute__((aligned(16))) uint64_t kr_lds[];
    __shared__ double red[NA * (BLOCK / 64)];
    const KondoReprDev &R = *t.R;
    const int tid = threadIdx.x, pass = blockIdx.y, n = t.n_sites;
    const uint64_t mlow = (1ULL << n) - 1ULL;
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    if (KIND != kKrDiag) {
        uint64_t *lds_A = kr_lds + t.n_tab;                                   // tab | A | binom | chr | perm
        uint64_t *lds_binom = lds_A + kKondoTabEntries;
        double *chr = reinterpret_cast<double *>(lds_binom + kKondoTabEntries);        // [2 * n_trans]
        int8_t *perm = reinterpret_cast<int8_t *>(chr + 2 * t.n_trans);       // [n_trans * n_sites]
        for (int k = tid; k < t.n_tab; k += BLOCK) kr_lds[k] = t.tab[k];
        for (int k = tid; k < kKondoTabEntries; k += BLOCK) {
            lds_A[k] = R.k.A[k];
            lds_binom[k] = R.k.binom[k];
        }
        for (int k = tid; k < 2 * t.n_trans; k += BLOCK) chr[k] = R.chr[k];
        for (int k = tid; k < t.n_trans * n; k += BLOCK) perm[k] = R.perm[k];
        __syncthreads();
        const uint64_t *tab = kr_lds, *A = lds_A, *binom = lds_binom;
        const bool down = KIND == kKrHop && pass >= t.hop_passes;             // the species of a HOP pass
        const int lp = KIND == kKrHop && down ? pass - t.hop_passes : pass;
        const int32_t *start = KIND == kKrLE ? t.orb_start : t.cls_start;
        const uint32_t *plist = KIND == kKrLE ? t.opairs : t.pairs;
        int k0[GH + 1];
        corr_group_bounds<GH>(start, lp * GH, k0);
        for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
            const uint8_t ci = t.info[row];
            if (ci & 0x80) continue;                                          // zero norm at this momentum: its entry is never read
            const uint64_t a = t.reps[row], au = a & mlow, ad = (a >> n) & mlow, as = a >> (2 * n);
            const double sa = (double)(ci & 0x7f);
            const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
#pragma unroll
            for (int g = 0; g < GH; ++g) {
                double sr = 0.0, si = 0.0;
#pragma unroll 1
                for (int k = k0[g]; k < k0[g + 1]; ++k) {
                    const uint32_t pr = plist[k];
                    const int p = (int)(pr & 255u), q = (int)((pr >> 8) & 255u);         // p < q, except in LE: any ordered pair
                    const uint64_t bp = 1ULL << p, bq = 1ULL << q, m = bp | bq;
                    uint64_t cu = au, cd = ad, cs = as;                       // the candidate word's three fields
                    int par = 0;
                    bool fwd = true;                                          // the orientation found is a forward one
                    if (KIND == kKrLE) {
                        // (local spin up, down-only site) = (p, q): the candidate has the local spin down and the electron up
                        if ((as & bp) || !(ad & bq) || (au & bq)) continue;
                        par = (__popcll(au & (bq - 1ULL)) + __popcll(au) + __popcll(ad & (bq - 1ULL))) & 1;
                        cu = au | bq;
                        cd = ad ^ bq;
                        cs = as | bp;
                    } else {
                        const uint64_t between = (bq - 1ULL) & ~((bp << 1) - 1ULL);
                        bool first;                                           // the orientation is (p, q); (q, p) otherwise
                        if (KIND == kKrHop) {
                            // (occupied site, empty site): the particle moves from the first to the second
                            const uint64_t occ = down ? ad : au, om = occ & m;
                            if (om == 0 || om == m) continue;
                            first = om == bp;
                            par = __popcll(occ & between) & 1;
                            if (down) cd = ad ^ m;
                            else      cu = au ^ m;
                        } else if (KIND == kKrEE) {
                            // (up-only site, down-only site): the two electrons trade places
                            const uint64_t uo = au & ~ad, dn = ad & ~au;
                            if ((uo & bp) && (dn & bq)) first = true;
                            else if ((uo & bq) && (dn & bp)) first = false;
                            else continue;
                            par = 1 ^ ((__popcll(au & between) + __popcll(ad & between)) & 1);
                            cu = au ^ m;
                            cd = ad ^ m;
                        } else {
                            // (local spin up, local spin down): both turn over
                            const uint64_t sm = as & m;
                            if (sm == 0 || sm == m) continue;
                            first = sm == bq;
                            cs = as ^ m;
                        }
                        fwd = (pr >> (first ? 16 : 17)) & 1u;
                    }
                    // the smallest image of the candidate, its translation and the sign of T_{g*}
                    uint64_t b = cu | (cd << n) | (cs << (2 * n));
                    int gs = 0;
                    for (int gg = 1; gg < t.n_trans; ++gg) {
                        const uint64_t im = repr_translate(tab, t.n_chunks, gg, cu) | (repr_translate(tab, t.n_chunks, gg, cd) << n) |
                                            (repr_translate(tab, t.n_chunks, gg, cs) << (2 * n));
                        if (im < b) {
                            b = im;
                            gs = gg;
                        }
                    }
                    if (gs) par ^= hubrepr_parity(perm + gs * n, cu) ^ hubrepr_parity(perm + gs * n, cd);
                    const uint64_t rk = kd_rank(R.k, A, binom, b & mlow, (b >> n) & mlow, b >> (2 * n));
                    const int64_t lo = sector_dir_find(t.reps, t.chunk_pos, t.dim, b, rk);
                    const uint8_t cj = t.info[lo];
                    if (cj & 0x80) continue;                                  // zero-norm target: dropped
                    const double f = (par ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
                    const double zr = f * chr[2 * gs], zi = -f * chr[2 * gs + 1];      // sign conj(chi(g*)) sqrt(|S_b|/|S_a|)
                    if (REALX) {
                        sr += x.x * (zr * t.xr[lo]);
                    } else {
                        const d2 xb = t.xg[lo];
                        const double yr = zr * xb.x - zi * xb.y, yi = zr * xb.y + zi * xb.x;
                        sr += x.x * yr + x.y * yi;                            // conj(psi_a) * y
                        const double ti = x.x * yi - x.y * yr;
                        si += fwd ? ti : -ti;
                    }
                }
                acc[g] += sr;
                if (!REALX) acc[GH + g] += si;
            }
        }
    } else {
        int sub = 0;
        while (pass >= t.sub_end[sub]) ++sub;
        const int lp = pass - (sub > 0 ? t.sub_end[sub - 1] : 0);             // the pass among those of its sub-kind
        if (sub == kKrSubSite) {
            constexpr int NS = kKrSite;
            uint64_t mk[NS];
#pragma unroll
            for (int g = 0; g < NS; ++g) mk[g] = corr_uniform(t.site_mask[lp * NS + g]);
            for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
                if (t.info[row] & 0x80) continue;
                const uint64_t a = t.reps[row], au = a & mlow, ad = (a >> n) & mlow, as = a >> (2 * n);
                const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
                const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
                for (int g = 0; g < NS; ++g) {
                    acc[g] += w * (double)__popcll(au & mk[g]);
                    acc[NS + g] += w * (double)__popcll(ad & mk[g]);
                    acc[2 * NS + g] += w * (double)__popcll(au & ad & mk[g]);
                    acc[3 * NS + g] += w * (double)((int)__popcll(mk[g]) - 2 * (int)__popcll(as & mk[g]));     // signed: __popcll is unsigned
                }
                acc[NA - 1] += w;
            }
        } else if (sub == kKrSubNN) {
            constexpr int GN = kKrNN;
            int k0[GN + 1];
            corr_group_bounds<GN>(t.cls_start, lp * GN, k0);
            for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
                if (t.info[row] & 0x80) continue;
                const uint64_t a = t.reps[row], au = a & mlow, ad = (a >> n) & mlow;
                const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
                const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
                for (int g = 0; g < GN; ++g) {
                    uint32_t uu = 0, dd = 0, f = 0, bk = 0;
#pragma unroll 1
                    for (int k = k0[g]; k < k0[g + 1]; ++k) {
                        const uint32_t pr = t.pairs[k];
                        const int p = (int)(pr & 255u), q = (int)((pr >> 8) & 255u);
                        const uint32_t up = (uint32_t)(au >> p) & 1u, uq = (uint32_t)(au >> q) & 1u;
                        const uint32_t dp = (uint32_t)(ad >> p) & 1u, dq = (uint32_t)(ad >> q) & 1u;
                        const uint32_t f1 = (pr >> 16) & 1u, f2 = (pr >> 17) & 1u;                   // (p, q) / (q, p) is forward
                        const uint32_t o1 = up & dq, o2 = uq & dp;            // orientation (up site, down site) = (p, q) / (q, p)
                        uu += up & uq;
                        dd += dp & dq;
                        f += (o1 & f1) + (o2 & f2);
                        bk += (o1 & (f1 ^ 1u)) + (o2 & (f2 ^ 1u));
                    }
                    acc[g] += w * (double)uu;
                    acc[GN + g] += w * (double)dd;
                    acc[2 * GN + g] += w * (double)f;
                    acc[3 * GN + g] += w * (double)bk;
                }
            }
        } else if (sub == kKrSubZN) {
            constexpr int GZ = kKrZN;
            int k0[GZ + 1];
            corr_group_bounds<GZ>(t.orb_start, lp * GZ, k0);
            for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
                if (t.info[row] & 0x80) continue;
                const uint64_t a = t.reps[row], au = a & mlow, ad = (a >> n) & mlow, as = a >> (2 * n);
                const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
                const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
                for (int g = 0; g < GZ; ++g) {
                    int zu = 0, zd = 0;
#pragma unroll 1
                    for (int k = k0[g]; k < k0[g + 1]; ++k) {
                        const uint32_t pr = t.opairs[k];
                        const int p = (int)(pr & 255u), q = (int)((pr >> 8) & 255u);                 // S^z on p, the electron on q
                        const int z2 = 1 - 2 * (int)((as >> p) & 1ULL);
                        zu += z2 * (int)((au >> q) & 1ULL);
                        zd += z2 * (int)((ad >> q) & 1ULL);
                    }
                    acc[g] += w * (double)zu;
                    acc[GZ + g] += w * (double)zd;
                }
            }
        } else {
            constexpr int GZ = kKrZZ;
            int k0[GZ + 1];
            corr_group_bounds<GZ>(t.cls_start, lp * GZ, k0);
            for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
                if (t.info[row] & 0x80) continue;
                const uint64_t as = t.reps[row] >> (2 * n);
                const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
                const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
                for (int g = 0; g < GZ; ++g) {
                    int z = 0;
#pragma unroll 1
                    for (int k = k0[g]; k < k0[g + 1]; ++k) {
                        const uint32_t pr = t.pairs[k];
                        z += 1 - 2 * (int)(((as >> (pr & 255u)) ^ (as >> ((pr >> 8) & 255u))) & 1ULL);
                    }
                    acc[g] += w * (double)z;
                }
            }
        }
    }
    corr_block_partials<NA, BLOCK>(acc, red, t.partials);
}

// ------------------------------------------------------------------------------------------------------ host side --
// dynamic LDS of a launch: translation tables, A, binom, characters and permutation bytes
size_t kr_lds_bytes(int n_sites, int n_trans, size_t n_tab)
{
    return (n_tab + 2 * (size_t)kKondoTabEntries + 2 * (size_t)n_trans + ((size_t)n_trans * n_sites + 7) / 8) * 8;
}

template <bool REALX, int KIND>
void (*kr_kernel(bool large))(CorrKondoRepr)
{
    return large ? k_corr_kondorepr<REALX, kReprBlockL, KIND>
                 : k_corr_kondorepr<REALX, kReprBlockS, KIND>;
}

// one launch and one two-stage reduction per kind that is asked for: comp[kind][pass * kKrAcc + accumulator]; dp: the sub-kinds
// of the DIAG launch, hp: the two species of the HOP launch
template <bool REALX>
int corr_kondorepr_run(const char *who, CorrKondoRepr t, const ReprClasses &K, const ReprOrbits &O, const bool want_sub[kKrSubs],
                       const bool want_kind[kKrKinds], std::vector<double> comp[kKrKinds], CorrPasses &dp, CorrPasses &hp, hipStream_t s,
                       std::vector<void *> &pool)
{
    constexpr int NA = kKrAcc;
    dp.add(kKrSubSite, K.n_orb, kKrSite);
    dp.add(kKrSubNN, want_sub[kKrSubNN] ? K.n_cls : 0, kKrNN);
    dp.add(kKrSubZN, want_sub[kKrSubZN] ? O.n_orb : 0, kKrZN);
    dp.add(kKrSubZZ, want_sub[kKrSubZZ] ? K.n_cls : 0, kKrZZ);
    for (int k = 0; k < kKrSubs; ++k) t.sub_end[k] = dp.first[k] + dp.count[k];
    const int n_site = dp.count[kKrSubSite], n_gat = (K.n_cls + kKrGat - 1) / kKrGat;     // passes of one Hermitian gathered group
    if (want_kind[kKrHop])
        for (int species = 0; species < 2; ++species) hp.add(species, K.n_cls, kKrGat);
    t.hop_passes = n_gat;
    const int n_passes[kKrKinds] = {dp.n_pass, want_kind[kKrHop] ? 2 * n_gat : 0, want_kind[kKrEE] ? n_gat : 0,
                                    want_kind[kKrLL] ? n_gat : 0, want_kind[kKrLE] ? (O.n_orb + kKrGat - 1) / kKrGat : 0};
    std::vector<int32_t> cls_start, orb_start;
    std::vector<uint32_t> pairs, opairs;
    repr_flatten(K.pairs, NA, cls_start, pairs);
    repr_flatten(O.pairs, NA, orb_start, opairs);
    std::vector<uint64_t> site_mask((size_t)n_site * kKrSite, 0ULL);
    std::copy(K.mask.begin(), K.mask.end(), site_mask.begin());
    int32_t *d_cstart = nullptr, *d_ostart = nullptr;
    uint32_t *d_pairs = nullptr, *d_opairs = nullptr;
    uint64_t *d_mask = nullptr;
    QBH_TRY(upload(cls_start, &d_cstart, pool));
    QBH_TRY(upload(orb_start, &d_ostart, pool));
    QBH_TRY(upload(pairs, &d_pairs, pool));
    QBH_TRY(upload(opairs, &d_opairs, pool));
    QBH_TRY(upload(site_mask, &d_mask, pool));
    t.cls_start = d_cstart;
    t.orb_start = d_ostart;
    t.pairs = d_pairs;
    t.opairs = d_opairs;
    t.site_mask = d_mask;
    const size_t lds = kr_lds_bytes(t.n_sites, t.n_trans, (size_t)t.n_tab);
    if (lds > kKrLdsMax) {
        set_error("%s: internal: %d table words", who, t.n_tab);
        return QBH_EHIP;
    }
    const ReprShape shape = repr_launch_shape(lds, t.dim);   // one shape for every kind: the DIAG launch stages nothing, but
    for (int k = 0; k < kKrKinds; ++k) {                     // its grid along x does not depend on what is asked for
        comp[k].clear();
        if (n_passes[k] == 0) continue;
        void (*kernel)(CorrKondoRepr) = k == kKrDiag ? kr_kernel<REALX, kKrDiag>(shape.large) : k == kKrHop ? kr_kernel<REALX, kKrHop>(shape.large)
                             : k == kKrEE ? kr_kernel<REALX, kKrEE>(shape.large) : k == kKrLL    ? kr_kernel<REALX, kKrLL>(shape.large)
                                                                                                : kr_kernel<REALX, kKrLE>(shape.large);
        QBH_TRY(corr_reduce_launch(who, kernel, shape.gx, n_passes[k], NA, shape.block, k == kKrDiag ? 0 : lds, s, t, nullptr, pool,
                                   comp[k]));
    }
    return QBH_OK;
}

}  // namespace
}  // namespace qbh

// Refusals, in this order, all before the device is looked for and before anything is written:
//   QBH_EINVAL   perms or chars NULL; the shape as qbh_gen_kondo checks it (n_sites outside 1 .. 21, n_elec outside 0 .. 2 n_sites,
//                a parity of (n_elec, two_sz, n_sites) that admits no block)
//   QBH_EUNSUPP  an empty sector
//   QBH_EINVAL   n_trans outside 1 .. 64; not exactly one of d_vec / d_vec_re; norm2 NULL; translation 0 not the identity; a
//                translation that is no site permutation; d_vec_re with a complex character
//   QBH_EUNSUPP  2^40 or more words in the sector
//   QBH_ENODEVICE
// and after the enumeration QBH_EUNSUPP for 2^31 - 1 representatives or more.
extern "C" int qbh_corr_kondo_repr_dev(int n_sites, int n_elec, int two_sz, int n_trans, const int32_t *perms, const double *chars,
                                       const qbh_z *d_vec, const double *d_vec_re, double *norm2, double *site, double *nn, double *zn,
                                       double *zz, qbh_z *hop, qbh_z *ee, qbh_z *ll, qbh_z *le, int64_t *dim_out, void *stream)
{
    using namespace qbh;
    const char *who = "qbh_corr_kondo_repr_dev";
    QBH_TRY(repr_check_tables(who, perms, chars));
    std::vector<KondoReprDev> rr(1);
    memset(rr.data(), 0, sizeof(KondoReprDev));
    KondoReprDev &R = rr[0];
    QBH_TRY(kondo_shape(who, n_sites, n_elec, two_sz, R.k));           // the shape (QBH_EINVAL), then an empty sector (QBH_EUNSUPP)
    QBH_TRY(repr_check_trans(who, n_trans));
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    QBH_TRY(corr_check_norm2(who, norm2));
    std::vector<uint64_t> tab;
    QBH_TRY(kondo_symmetry(R, tab, n_trans, perms, chars, who));
    if (d_vec_re != nullptr) QBH_TRY(repr_real_characters(who, R.chr, n_trans));
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));           // every refusal comes before the device is looked for
    QBH_TRY(corr_check_device());
    const int N = n_sites;
    const ReprClasses K = repr_classes(N, n_trans, perms);
    const ReprOrbits O = repr_ordered_orbits(N, n_trans, perms);
    DevBufs bufs;
    SectorDev<KondoReprDev> S;
    int64_t *d_pos = nullptr;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who, &d_pos));
    CorrKondoRepr t{};
    t.R = S.R;
    t.tab = S.tab;
    t.reps = S.reps;
    t.info = S.info;
    t.chunk_pos = d_pos;
    t.dim = S.dim;
    t.n_tab = (int)tab.size();
    t.n_sites = N;
    t.n_trans = n_trans;
    t.n_chunks = R.n_chunks;
    t.xg = reinterpret_cast<const d2 *>(d_vec);
    t.xr = d_vec_re;
    const bool rx = d_vec_re != nullptr;
    const bool want_sub[kKrSubs] = {true, nn != nullptr, zn != nullptr, zz != nullptr};
    const bool want_kind[kKrKinds] = {true, hop != nullptr, ee != nullptr, ll != nullptr, le != nullptr};
    std::vector<double> comp[kKrKinds];
    CorrPasses dp, hp;
    const CorrPasses lone;                                   // the layout of a launch of one kind: its passes begin at 0
    if (rx) QBH_TRY(corr_kondorepr_run<true>(who, t, K, O, want_sub, want_kind, comp, dp, hp, (hipStream_t)stream, bufs.pool));
    else    QBH_TRY(corr_kondorepr_run<false>(who, t, K, O, want_sub, want_kind, comp, dp, hp, (hipStream_t)stream, bufs.pool));
    constexpr int NA = kKrAcc, GH = kKrGat;
    auto diag = [&](int sub, int item, int per_pass, int slot) { return dp.at(comp[kKrDiag], sub, item, per_pass, slot, NA); };
    const double n2 = diag(kKrSubSite, 0, kKrSite, 5);
    *norm2 = n2;
    if (dim_out) *dim_out = S.dim;
    std::vector<double> nu((size_t)N), nd((size_t)N), dc((size_t)N), sz((size_t)N);
    for (int i = 0; i < N; ++i) {
        const int o = K.orb[(size_t)i];
        const double n_s = (double)K.n_s[(size_t)o];
        nu[(size_t)i] = diag(kKrSubSite, o, kKrSite, 0) / n_s;
        nd[(size_t)i] = diag(kKrSubSite, o, kKrSite, 1) / n_s;
        dc[(size_t)i] = diag(kKrSubSite, o, kKrSite, 2) / n_s;
        sz[(size_t)i] = diag(kKrSubSite, o, kKrSite, 3) / (2.0 * n_s);
    }
    if (site) {
        std::copy(nu.begin(), nu.end(), site);
        std::copy(nd.begin(), nd.end(), site + N);
        std::copy(dc.begin(), dc.end(), site + 2 * N);
        std::copy(sz.begin(), sz.end(), site + 3 * N);
    }
    const size_t NN = (size_t)N * N;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const size_t ij = (size_t)i * N + j;
            const int o = O.orb[ij];
            const double n_o = (double)O.size[(size_t)o];
            if (zn) {
                zn[ij] = diag(kKrSubZN, o, kKrZN, 0) / (2.0 * n_o);
                zn[NN + ij] = diag(kKrSubZN, o, kKrZN, 1) / (2.0 * n_o);
            }
            if (le) le[ij] = qbh_z{lone.at(comp[kKrLE], 0, o, GH, 0, NA) / n_o, rx ? 0.0 : lone.at(comp[kKrLE], 0, o, GH, 1, NA) / n_o};
            if (i == j) {
                if (nn) corr_put_nn_diag(nn, N, i, nu[(size_t)i], dc[(size_t)i], nd[(size_t)i]);
                if (zz) zz[ij] = 0.25 * n2;
                corr_put_onsite_diag(hop, ee, N, i, nu[(size_t)i], nd[(size_t)i], dc[(size_t)i]);
                if (ll) ll[ij] = qbh_z{0.5 * n2 + sz[(size_t)i], 0.0};
                continue;
            }
            const int c = K.cls[ij];
            const bool forward = K.fwd[ij] != 0, self = K.self[(size_t)c] != 0;
            const double n_u = (double)K.nu[(size_t)c];
            // a Hermitian gathered group; part: the species in the HOP launch (layout hp), 0 in a launch of one kind (layout lone)
            auto gathered = [&](const CorrPasses &lay, int kind, int part) {
                return repr_herm_value(lay.at(comp[kind], part, c, GH, 0, NA), (rx || self) ? 0.0 : lay.at(comp[kind], part, c, GH, 1, NA),
                                       2.0 * n_u, forward);
            };
            if (nn) corr_put_nn_class(nn, N, i, j, diag(kKrSubNN, c, kKrNN, 0), diag(kKrSubNN, c, kKrNN, 1), diag(kKrSubNN, c, kKrNN, 2), diag(kKrSubNN, c, kKrNN, 3), n_u, self, forward);
            if (zz) zz[ij] = diag(kKrSubZZ, c, kKrZZ, 0) / (4.0 * n_u);
            if (hop) {
                hop[ij] = gathered(hp, kKrHop, 0);
                hop[NN + ij] = gathered(hp, kKrHop, 1);
            }
            if (ee) ee[ij] = gathered(lone, kKrEE, 0);
            if (ll) ll[ij] = gathered(lone, kKrLL, 0);
        }
    return QBH_OK;
}
