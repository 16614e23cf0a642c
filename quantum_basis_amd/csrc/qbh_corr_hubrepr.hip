// qbh_corr_hubrepr.hip -- qbh_corr_hubbard_repr_dev: all-pair static correlations of a two-species fermion state held in a
// MOMENTUM SECTOR (basis of qbh_gen_hubbard_repr: all orbit representatives of the words u | d << n_sites, ascending), in one
// pass over the representatives.  The result is what qbh_corr_hubbard_dev returns on the unfolded full-space state.
//
// With T_g |u, d> = sgn(g, u) sgn(g, d) |g(u), g(d)>, |a, k> = (|G| |S_a|)^(-1/2) sum_g chi(g) T_g |a> and Psi = sum_a psi_a |a, k>
// (representatives of zero norm left out, their entries never read), and w_a = |psi_a|^2:
//   norm2          = sum_a w_a
//   dens[s][i]     = sum_a w_a (1/|G|) sum_g n_{g(i),s}(a)
//   nn[2A+B][i][j] = sum_a w_a (1/|G|) sum_g n_{g(i),A}(a) n_{g(j),B}(a)                                  (i = j included)
//   hop[s][i][j]   = (1/|G|) sum_a sum_{g: a has g(i) occupied and g(j) empty in species s} conj(psi_a) v psi_b
//   flip[i][j]     = (1/|G|) sum_a sum_{g: a has only an up particle at g(i) and only a down particle at g(j)} conj(psi_a) v psi_b
//       v = (operator sign) sigma(g*) conj(chi(g*)) sqrt(|S_b| / |S_a|),  c = a with the particle(s) moved,  T_{g*} |c> = sigma |b>,
// the entries of hubrepr_row for the one-term operators c+_{i,s} c_{j,s} and S+_i S-_j = -(c+_{i,up} c_{j,up})(c+_{j,dn} c_{i,dn}),
// averaged over the group: hop sign = the parity of the species' particles between the two sites, the exchange's sign = minus
// the product of the two hop signs.  A target b of zero norm is skipped, and with no_double a hop onto a site that the other
// species occupies.  Nothing is divided by norm2.
//
// The sums over g only see the IMAGE of (i, j): a row walks the unordered site pairs {p, q} once and adds what it finds to the
// accumulators of the pair's CLASS (qbh_corr_repr.hpp: an orbit of ordered pairs together with its mirror image; one of the two
// orbits is called forward).  With n_u unordered pairs in the class, per class
//   UU, DD    sum_a w_a #{pairs with both sites occupied in the species}                            nn_uu = UU / n_u
//   F, B      sum_a w_a #{orientations (p, q) with p up and q down that are forward / backward}     nn_ud[i][j] = F / n_u for (i, j)
//             forward, B / n_u backward; a class that is its own mirror has only forward pairs: F / (2 n_u);  nn_du[i][j] = nn_ud[j][i]
//   C (hop of a species, flip)   the term of the pair's one orientation -- (occupied site, empty site) for a hop, (up-only site,
//             down-only site) for the flip -- if that orientation is forward, its conjugate if not (Hermiticity):
//             value[i][j] = C / (2 n_u) for (i, j) forward, its conjugate otherwise; real for a class that is its own mirror
// and per orbit of sites  U, D, UD = sum_a w_a popcount(u & orbit), (d & orbit), (u & d & orbit):  dens = U / n_s, D / n_s, the
// double occupancy UD / n_s.  The host fills the diagonals: nn_uu[i][i] = hop[0][i][i] = dens[0][i], nn_ud[i][i] = docc,
// flip[i][i] = dens[0][i] - docc[i].  The diagonal groups cost no gather: w_a times a small integer.
//
// Gathers: one per row, species and unordered pair of unequally occupied sites (hop), one per pair of an up-only and a down-only
// site (flip).  A candidate is canonicalised with the byte-sliced translation tables, the parity of T_{g*} comes from the
// permutation bytes, b is ranked with the binomials (rank(d) C(n, n_up) + rank(u)) and found through the directory of the
// enumeration (sector_dir_find).
//
// Launch: (row blocks) x (passes), one lane per representative, grid-stride over a resident grid.  Pass kinds as in
// k_corr_hubbard, kHrAcc = 16 accumulators each, indexed by compile-time constants only:
//   NN    4 classes:  [g] UU, [4+g] DD, [8+g] F, [12+g] B                                 no gather
//   HOPU / HOPD / FLIP  8 classes:  [g] Re C, [8+g] Im C (complex vectors only)           gathers
//   SITE  5 site orbits:  [g] U, [5+g] D, [10+g] UD, [15] norm2 (read from the first site pass)
// A group that is not asked for has no passes; it changes neither the grid along x nor any other accumulator, so the other
// outputs keep their bits.  Every workgroup leaves its sums at partials[blockIdx.x][pass][accumulator] (corr_block_partials) and
// k_corr_reduce adds the workgroups in a fixed order (corr_reduce_launch): no atomics, two calls return the same bits.
//
// Tables.  The binomials, the characters and the permutation bytes are always staged in LDS (at most 12 KB).  The translation
// tables join them when everything fits kCorrLdsCap (150 KB); 62 group elements x 6 chunks (the dihedral group of a ring of 31)
// are 186 KB and are read from global memory instead, so no shape that qbh_gen_hubbard_repr accepts is refused here.  The LDS
// footprint chooses between workgroups of 256 lanes (four or more fit a CU) and one of 1024, as in qbh_corr_repr.hip.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), 0 bytes of scratch in every instance; the static LDS is
// the reduction scratch, the tables are dynamic LDS on top of it:
//   k_corr_hubrepr<vector, lanes, tables>     VGPRs  SGPRs  wavefronts/SIMD  static LDS  scratch
//   <complex,  256, LDS>                        116    106        4            512 B       0
//   <complex, 1024, LDS>                        116    106        4           2048 B       0
//   <complex,  256, global>                     116    106        4            512 B       0
//   <real,     256, LDS>                         93    106        5            512 B       0
//   <real,    1024, LDS>                         93    106        5           2048 B       0
//   <real,     256, global>                      93    106        5            512 B       0
// 116 VGPRs keep four wavefronts per SIMD, which is what a workgroup of 1024 lanes needs (128 at most); 32 accumulators instead
// of 16 would not.
#include <algorithm>
#include <vector>

#include "qbh_sector.hpp"
#include "qbh_device.hpp"
#include "qbh_corr.hpp"                                      // device helpers, launch path, pass layout and host fills
#include "qbh_corr_repr.hpp"                                 // classes and orbits of site pairs, symmetry checks

namespace qbh {
namespace {

constexpr int kHrAcc = 16;                                   // accumulators of a pass
constexpr int kHrNN = kHrAcc / 4, kHrGat = kHrAcc / 2, kHrSite = (kHrAcc - 1) / 3;      // classes / classes / site orbits of a pass
enum { kHrKindNN = 0, kHrKindHopU = 1, kHrKindHopD = 2, kHrKindFlip = 3, kHrKindSite = 4 };
constexpr int kHrBinomRow = 34;                              // HubReprDev::binom[p][0 .. 33]

// The pair words of class c are pairs[cls_start[c] .. cls_start[c + 1]) (qbh_corr_repr.hpp); cls_start is padded with the total
// beyond the last class, so a pass reads its kHrNN + 1 or kHrGat + 1 entries without a bound check.  Site pass sp owns the site
// orbits sp * kHrSite ... with the masks site_mask[..] (0 past the last orbit).
struct CorrHubRepr {
    const HubReprDev *R;                                     // binomials, characters, permutation bytes (staged in LDS)
    const uint64_t *tab, *reps;
    const uint8_t *info;
    const int64_t *chunk_pos;
    int64_t dim;
    int n_tab, n_sites, n_up, n_trans, n_chunks, no_double;
    int pass_end[5];                                         // passes [pass_end[k - 1], pass_end[k]) are of kind k
    const int32_t *cls_start;
    const uint32_t *pairs;
    const uint64_t *site_mask;
    const d2 *xg;                                            // exactly one of xg / xr
    const double *xr;
    double *partials;
};

// rank of the pattern `bits` among the patterns of its popcount, from the staged binomials
__device__ __forceinline__ uint64_t hr_rank(const uint64_t *binom, uint64_t bits)
{
    uint64_t rk = 0;
    for (int kk = 1; bits; ++kk) {
        rk += binom[(__ffsll((long long)bits) - 1) * kHrBinomRow + kk];
        bits &= bits - 1;
    }
    return rk;
}

template <bool REALX, int BLOCK, bool TABLDS>
__global__ __launch_bounds__(BLOCK) void k_corr_hubrepr(CorrHubRepr t)
{
    constexpr int NA = kHrAcc, GN = kHrNN, GH = kHrGat, NS = kHrSite;
    extern __shared__ __attribute__((aligned(16))) uint64_t hr_lds[];
    __shared__ double red[NA * (BLOCK / 64)];
    const HubReprDev &R = *t.R;
    const int tid = threadIdx.x, pass = blockIdx.y, n = t.n_sites;
    const int n_binom = (n + 1) * kHrBinomRow, n_perm = t.n_trans * n;
    uint64_t *binom = hr_lds + (TABLDS ? t.n_tab : 0);                    // [(n_sites + 1) * 34]
    double *chr = reinterpret_cast<double *>(binom + n_binom);            // [2 * n_trans]
    int8_t *perm = reinterpret_cast<int8_t *>(chr + 2 * t.n_trans);       // [n_trans * n_sites]
    int kind = 0;
    while (pass >= t.pass_end[kind]) ++kind;
    const int lp = pass - (kind > 0 ? t.pass_end[kind - 1] : 0);          // the pass among those of its kind
    const bool gathers = kind == kHrKindHopU || kind == kHrKindHopD || kind == kHrKindFlip;
    if (gathers) {
        if (TABLDS)
            for (int k = tid; k < t.n_tab; k += BLOCK) hr_lds[k] = t.tab[k];
        for (int k = tid; k < n_binom; k += BLOCK) binom[k] = (&R.binom[0][0])[k];
        for (int k = tid; k < 2 * t.n_trans; k += BLOCK) chr[k] = R.chr[k];
        for (int k = tid; k < n_perm; k += BLOCK) perm[k] = R.perm[k];
    }
    __syncthreads();
    const uint64_t *tab = TABLDS ? hr_lds : t.tab;
    const uint64_t mlow = (1ULL << n) - 1ULL;
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    if (gathers) {
        const bool no_double = t.no_double != 0;
        const uint64_t cu_count = binom[n * kHrBinomRow + t.n_up];
        int k0[GH + 1];
        corr_group_bounds<GH>(t.cls_start, lp * GH, k0);
        for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
            const uint8_t ci = t.info[row];
            if (ci & 0x80) continue;                                      // zero norm at this momentum: its entry is never read
            const uint64_t a = t.reps[row], au = a & mlow, ad = a >> n;
            const double sa = (double)(ci & 0x7f);
            const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
#pragma unroll
            for (int g = 0; g < GH; ++g) {
                double sr = 0.0, si = 0.0;
#pragma unroll 1
                for (int k = k0[g]; k < k0[g + 1]; ++k) {
                    const uint32_t pr = t.pairs[k];
                    const int p = (int)(pr & 255u), q = (int)((pr >> 8) & 255u);                 // p < q
                    const uint64_t bp = 1ULL << p, bq = 1ULL << q, m = bp | bq;
                    const uint64_t between = (bq - 1ULL) & ~((bp << 1) - 1ULL);
                    uint64_t cu, cd;                                      // the candidate word's two patterns
                    int par;
                    bool first;                                           // the orientation is (p, q); (q, p) otherwise
                    if (kind == kHrKindFlip) {
                        // orientation (up-only site, down-only site): the two particles trade places
                        const uint64_t uo = au & ~ad, dn = ad & ~au;
                        if ((uo & bp) && (dn & bq)) first = true;
                        else if ((uo & bq) && (dn & bp)) first = false;
                        else continue;
                        par = 1 ^ ((__popcll(au & between) + __popcll(ad & between)) & 1);
                        cu = au ^ m;
                        cd = ad ^ m;
                    } else {
                        // orientation (occupied site, empty site): the particle moves from the first to the second
                        const bool down = kind == kHrKindHopD;
                        const uint64_t occ = down ? ad : au, other = down ? au : ad, om = occ & m;
                        if (om == 0 || om == m) continue;                 // equally occupied: nothing to move
                        first = om == bp;
                        if (no_double && (other & (first ? bq : bp))) continue;                  // projected hopping
                        par = __popcll(occ & between) & 1;
                        cu = down ? au : occ ^ m;
                        cd = down ? occ ^ m : ad;
                    }
                    const bool fwd = (pr >> (first ? 16 : 17)) & 1u;
                    // hubrepr_canonical on the staged tables: the smallest image, its translation and the sign of T_{g*}
                    uint64_t b = cu | (cd << n);
                    int gs = 0;
                    for (int gg = 1; gg < t.n_trans; ++gg) {
                        const uint64_t im = repr_translate(tab, t.n_chunks, gg, cu) | (repr_translate(tab, t.n_chunks, gg, cd) << n);
                        if (im < b) {
                            b = im;
                            gs = gg;
                        }
                    }
                    if (gs) par ^= hubrepr_parity(perm + gs * n, cu) ^ hubrepr_parity(perm + gs * n, cd);
                    const uint64_t rk = hr_rank(binom, b >> n) * cu_count + hr_rank(binom, b & mlow);
                    const int64_t lo = sector_dir_find(t.reps, t.chunk_pos, t.dim, b, rk);
                    const uint8_t cj = t.info[lo];
                    if (cj & 0x80) continue;                              // zero-norm target: dropped
                    const double f = (par ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
                    const double zr = f * chr[2 * gs], zi = -f * chr[2 * gs + 1];      // sign conj(chi(g*)) sqrt(|S_b|/|S_a|)
                    if (REALX) {
                        sr += x.x * (zr * t.xr[lo]);
                    } else {
                        const d2 xb = t.xg[lo];
                        const double yr = zr * xb.x - zi * xb.y, yi = zr * xb.y + zi * xb.x;
                        sr += x.x * yr + x.y * yi;                        // conj(psi_a) * y
                        const double ti = x.x * yi - x.y * yr;
                        si += fwd ? ti : -ti;
                    }
                }
                acc[g] += sr;
                if (!REALX) acc[GH + g] += si;
            }
        }
    } else if (kind == kHrKindNN) {
        int k0[GN + 1];
        corr_group_bounds<GN>(t.cls_start, lp * GN, k0);
        for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
            if (t.info[row] & 0x80) continue;
            const uint64_t a = t.reps[row], au = a & mlow, ad = a >> n;
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
    } else {
        uint64_t mk[NS];
#pragma unroll
        for (int g = 0; g < NS; ++g) mk[g] = corr_uniform(t.site_mask[lp * NS + g]);
        for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
            if (t.info[row] & 0x80) continue;
            const uint64_t a = t.reps[row], au = a & mlow, ad = a >> n;
            const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
            const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
            for (int g = 0; g < NS; ++g) {
                acc[g] += w * (double)__popcll(au & mk[g]);
                acc[NS + g] += w * (double)__popcll(ad & mk[g]);
                acc[2 * NS + g] += w * (double)__popcll(au & ad & mk[g]);
            }
            acc[3 * NS] += w;
        }
    }
    corr_block_partials<NA, BLOCK>(acc, red, t.partials);
}

// ------------------------------------------------------------------------------------------------------ host side --
// dynamic LDS of a launch: binomials, characters and permutation bytes, and the translation tables when all of it fits the budget
size_t hr_lds_small(int n_sites, int n_trans)
{
    return ((size_t)(n_sites + 1) * kHrBinomRow + 2 * (size_t)n_trans + ((size_t)n_trans * n_sites + 7) / 8) * 8;
}
bool hr_tab_lds(int n_sites, int n_trans, size_t n_tab) { return hr_lds_small(n_sites, n_trans) + n_tab * 8 <= kCorrLdsCap; }

// the passes of the wanted groups, the launch and the two-stage reduction: comp[pass * kHrAcc + accumulator]
template <bool REALX>
int corr_hubrepr_run(const char *who, CorrHubRepr t, const ReprClasses &K, size_t n_tab, bool want_nn, bool want_hop, bool want_flip,
                     std::vector<double> &comp, CorrPasses &hp, hipStream_t s, std::vector<void *> &pool)
{
    constexpr int NA = kHrAcc;
    hp.add(kHrKindNN, want_nn ? K.n_cls : 0, kHrNN);
    hp.add(kHrKindHopU, want_hop ? K.n_cls : 0, kHrGat);
    hp.add(kHrKindHopD, want_hop ? K.n_cls : 0, kHrGat);
    hp.add(kHrKindFlip, want_flip ? K.n_cls : 0, kHrGat);
    hp.add(kHrKindSite, K.n_orb, kHrSite);
    for (int k = 0; k < 5; ++k) t.pass_end[k] = hp.first[k] + hp.count[k];
    const int n_site = hp.count[kHrKindSite];
    std::vector<int32_t> cls_start;
    std::vector<uint32_t> pairs;
    repr_flatten(K.pairs, NA, cls_start, pairs);
    std::vector<uint64_t> site_mask((size_t)n_site * kHrSite, 0ULL);
    std::copy(K.mask.begin(), K.mask.end(), site_mask.begin());
    int32_t *d_start = nullptr;
    uint32_t *d_pairs = nullptr;
    uint64_t *d_mask = nullptr;
    QBH_TRY(upload(cls_start, &d_start, pool));
    QBH_TRY(upload(pairs, &d_pairs, pool));
    QBH_TRY(upload(site_mask, &d_mask, pool));
    t.cls_start = d_start;
    t.pairs = d_pairs;
    t.site_mask = d_mask;
    const bool tab_lds = hr_tab_lds(t.n_sites, t.n_trans, n_tab);
    const size_t lds = hr_lds_small(t.n_sites, t.n_trans) + (tab_lds ? n_tab * 8 : 0);
    const ReprShape shape = repr_launch_shape(lds, t.dim);
    const bool large = tab_lds && shape.large;                            // then one workgroup of 1024 lanes per CU
    void (*kernel)(CorrHubRepr) = !tab_lds ? k_corr_hubrepr<REALX, kReprBlockS, false>
                         : large  ? k_corr_hubrepr<REALX, kReprBlockL, true>
                                  : k_corr_hubrepr<REALX, kReprBlockS, true>;
    return corr_reduce_launch(who, kernel, shape.gx, hp.n_pass, NA, large ? kReprBlockL : kReprBlockS, lds, s, t, nullptr, pool,
                              comp);
}

}  // namespace
}  // namespace qbh

// Refusals, in this order, all before the device is looked for and before anything is written:
//   QBH_EINVAL   perms or chars NULL; n_sites outside 1 .. 31; n_up or n_dn outside 0 .. n_sites; n_trans outside 1 .. 64; no_double
//                not 0 or 1; not exactly one of d_vec / d_vec_re; translation 0 not the identity; a translation that is no site
//                permutation; d_vec_re with a complex character; no_double with more particles than sites
//   QBH_EUNSUPP  2^40 or more words in the (n_up, n_dn) space
//   QBH_ENODEVICE
extern "C" int qbh_corr_hubbard_repr_dev(int n_sites, int n_up, int n_dn, int no_double, int n_trans, const int32_t *perms,
                                         const double *chars, const qbh_z *d_vec, const double *d_vec_re, double *norm2, double *dens,
                                         double *nn, qbh_z *hop, qbh_z *flip, int64_t *dim_out, void *stream)
{
    using namespace qbh;
    const char *who = "qbh_corr_hubbard_repr_dev";
    QBH_TRY(repr_check_tables(who, perms, chars));
    if (n_sites < 1 || n_sites > 31) {
        set_error("%s: n_sites = %d (1 .. 31 allowed)", who, n_sites);
        return QBH_EINVAL;
    }
    if (n_up < 0 || n_up > n_sites || n_dn < 0 || n_dn > n_sites) {
        set_error("%s: (n_up, n_dn) = (%d, %d) (0 .. n_sites allowed)", who, n_up, n_dn);
        return QBH_EINVAL;
    }
    QBH_TRY(repr_check_trans(who, n_trans));
    if (no_double != 0 && no_double != 1) {
        set_error("%s: no_double = %d (0 or 1 allowed)", who, no_double);
        return QBH_EINVAL;
    }
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    std::vector<HubReprDev> rr(1);
    HubReprDev &R = rr[0];
    std::vector<uint64_t> tab;
    QBH_TRY(hubrepr_symmetry(R, tab, n_sites, n_up, n_dn, n_trans, perms, chars, who));
    R.no_double = no_double;
    if (d_vec_re != nullptr) QBH_TRY(repr_real_characters(who, R.chr, n_trans));
    if (no_double && n_up + n_dn > n_sites) {
        set_error("%s: no_double with n_up + n_dn = %d particles on %d sites: the space is empty", who, n_up + n_dn, n_sites);
        return QBH_EINVAL;
    }
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));           // every refusal comes before the device is looked for
    QBH_TRY(corr_check_device());
    const int N = n_sites;
    const ReprClasses K = repr_classes(N, n_trans, perms);
    DevBufs bufs;
    SectorDev<HubReprDev> S;
    int64_t *d_pos = nullptr;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who, &d_pos));
    CorrHubRepr t{};
    t.R = S.R;
    t.tab = S.tab;
    t.reps = S.reps;
    t.info = S.info;
    t.chunk_pos = d_pos;
    t.dim = S.dim;
    t.n_tab = (int)tab.size();
    t.n_sites = N;
    t.n_up = n_up;
    t.n_trans = n_trans;
    t.n_chunks = R.n_chunks;
    t.no_double = no_double;
    t.xg = reinterpret_cast<const d2 *>(d_vec);
    t.xr = d_vec_re;
    const bool rx = d_vec_re != nullptr;
    std::vector<double> comp;
    CorrPasses hp;
    if (rx) QBH_TRY(corr_hubrepr_run<true>(who, t, K, tab.size(), nn != nullptr, hop != nullptr, flip != nullptr, comp, hp, (hipStream_t)stream, bufs.pool));
    else    QBH_TRY(corr_hubrepr_run<false>(who, t, K, tab.size(), nn != nullptr, hop != nullptr, flip != nullptr, comp, hp, (hipStream_t)stream, bufs.pool));
    constexpr int NA = kHrAcc, GN = kHrNN, GH = kHrGat, NS = kHrSite;
    auto at = [&](int kind, int item, int per_pass, int slot) { return hp.at(comp, kind, item, per_pass, slot, NA); };
    if (norm2) *norm2 = at(kHrKindSite, 0, NS, 3);
    if (dim_out) *dim_out = S.dim;
    std::vector<double> du((size_t)N), dd((size_t)N), dc((size_t)N);
    for (int i = 0; i < N; ++i) {
        const int o = K.orb[(size_t)i];
        const double n_s = (double)K.n_s[(size_t)o];
        du[(size_t)i] = at(kHrKindSite, o, NS, 0) / n_s;
        dd[(size_t)i] = at(kHrKindSite, o, NS, 1) / n_s;
        dc[(size_t)i] = at(kHrKindSite, o, NS, 2) / n_s;
    }
    if (dens) {
        std::copy(du.begin(), du.end(), dens);
        std::copy(dd.begin(), dd.end(), dens + N);
    }
    const size_t NN = (size_t)N * N;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const size_t ij = (size_t)i * N + j;
            if (i == j) {
                if (nn) corr_put_nn_diag(nn, N, i, du[(size_t)i], dc[(size_t)i], dd[(size_t)i]);
                corr_put_onsite_diag(hop, flip, N, i, du[(size_t)i], dd[(size_t)i], dc[(size_t)i]);
                continue;
            }
            const int c = K.cls[ij];
            const bool forward = K.fwd[ij] != 0, self = K.self[(size_t)c] != 0;
            const double n_u = (double)K.nu[(size_t)c];
            auto gathered = [&](int kind) {
                return repr_herm_value(at(kind, c, GH, 0), (rx || self) ? 0.0 : at(kind, c, GH, 1), 2.0 * n_u, forward);
            };
            if (nn) corr_put_nn_class(nn, N, i, j, at(kHrKindNN, c, GN, 0), at(kHrKindNN, c, GN, 1), at(kHrKindNN, c, GN, 2), at(kHrKindNN, c, GN, 3), n_u, self, forward);
            if (hop) {
                hop[ij] = gathered(kHrKindHopU);
                hop[NN + ij] = gathered(kHrKindHopD);
            }
            if (flip) flip[ij] = gathered(kHrKindFlip);
        }
    return QBH_OK;
}
