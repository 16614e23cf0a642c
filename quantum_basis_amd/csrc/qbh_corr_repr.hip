// qbh_corr_repr.hip -- qbh_corr_spin_repr_dev: all-pair static correlations of a spin-1/2 state held in a MOMENTUM SECTOR
// (basis of qbh_gen_heisenberg_repr: all orbit representatives, ascending), in one pass over the representatives.
//
// With |a, k> = (|G| |S_a|)^(-1/2) sum_g chi(g) T_g |a> and Psi = sum_a psi_a |a, k> the bilinear forms of the unfolded state are
//   norm2    = sum_a |psi_a|^2                                                            (nonzero-norm representatives only)
//   sz[i]    = sum_a |psi_a|^2 (1/|G|) sum_g s_{g(i)}(a),            s_p(a) = +1/2 (bit p clear) or -1/2 (bit set = down)
//   zz[i][j] = sum_a |psi_a|^2 (1/|G|) sum_g s_{g(i)}(a) s_{g(j)}(a)
//   pm[i][j] = (1/|G|) sum_a sum_{g: a has g(i) up, g(j) down} conj(psi_a) conj(chi(g*)) sqrt(|S_b|/|S_a|) psi_b,
//              c = a ^ bit g(i) ^ bit g(j),  b = g* c the representative of c (skipped when b has zero norm)
// -- the row formula of repr_row with the matrix element of S^+_i S^-_j in place of a bond's.  The sums over g only ever see
// the IMAGE of the pair (i, j), so a row does not loop over translations: it walks the unordered site pairs {p, q} once and adds
// what it finds to the accumulator of the pair's CLASS, and the host divides by the size of the class.
//
// Classes.  Two ordered pairs are in one orbit when a translation carries one to the other; a class is an orbit O together
// with its mirror image (q, p): zz is the same on both, pm on the mirror is the conjugate (Hermiticity).  One orbit of every
// class is called forward.  A row whose bits p and q differ has exactly one of the two orientations (up site, down site); it
// canonicalises the flipped word once, gathers psi_b once and adds the term t to the class if that orientation is forward, its
// conjugate if it is not: n_dn (N - n_dn) gathers per row, none for a pair of equal bits.  With n_u unordered pairs in the class
//   pm[i][j] = C / (2 n_u)  for (i, j) forward, its conjugate otherwise  (a class that is its own mirror has only forward pairs
//                            and a real value: |O| = 2 n_u there, |O| = n_u and both orbits summed otherwise)
//   zz[i][j] = Z / n_u,     Z = sum_a |psi_a|^2 (n_u - 2 u_a) / 4,  u_a = the pairs of the class whose bits differ in a
//   sz[i]    = S / n_s,     S = sum_a |psi_a|^2 (n_s / 2 - popcount(a & orbit of i)),  n_s = the sites in the orbit of i
// For a free action there are N^2 / |G| ordered classes, half of that after mirroring: 19 for 36 sites and 36 translations.
//
// The launch is a grid of (row blocks) x (passes) as in qbh_corr.hip: a pair pass owns kReprGroup classes and their list of
// site pairs, a site pass a group of site orbits (and norm2).  Accumulators are indexed by compile-time constants only, every
// workgroup leaves its sums at partials[blockIdx.x][pass][accumulator] (the pattern of mf_block_partials) and k_corr_reduce
// adds the workgroups in a fixed order: no atomics, two calls return the same bits, and a group that is not asked for changes
// neither the grid nor any other accumulator.  One lane per representative, grid-stride over a resident grid.  The flipped
// word is canonicalised with the byte-sliced translation tables (repr_translate), b is ranked with the binomials and found
// through the directory of the enumeration (sector_dir_find: at most 12 bisection steps).
//
// Tables.  The binomials and the characters are always staged in LDS (at most 18 KB).  The translation tables join them when
// everything fits the 150 KB budget of the other sector kernels (kCorrLdsCap); 64 translations x 11 chunks are 360 KB and are
// read from global memory instead, as k_sector_fill does, so no shape that qbh_gen_heisenberg_repr accepts is refused here.
// As in qbh_kondo_lds.hpp the LDS footprint chooses between workgroups of 256 lanes (four or more fit a CU) and one of 1024.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): 0 bytes of scratch in every instance; 123 VGPRs for the
// complex and 104 for the packed-real vector in all three shapes (256 lanes / 1024 lanes with the tables in LDS, 256 lanes with
// the tables in global memory), four wavefronts per SIMD; the table is in DESIGN 4.5e.
#include <algorithm>
#include <vector>

#include "qbh_sector.hpp"
#include "qbh_device.hpp"
#include "qbh_corr.hpp"                                      // device helpers, launch path, pass layout and host fills
#include "qbh_corr_repr.hpp"                                 // classes and orbits of site pairs, symmetry checks

namespace qbh {
namespace {

constexpr int kReprGroup = 8;                                // classes of a pair pass
constexpr int kBinomRow = 34;                               // HeisDev::binom[p][0 .. 33]

template <bool REALX>
constexpr int repr_acc() { return (REALX ? 2 : 3) * kReprGroup; }

// Pair pass `pass`, slot g = class pass * G + g: its pairs are pairs[slot_start[slot] .. slot_start[slot + 1]), one word
// p | q << 8 | fwd(p, q) << 16 | fwd(q, p) << 17 with p < q, and slot_nu[slot] = their number.  Accumulators of a pair pass:
//   [g] Z,  [G + g] Re C,  [2G + g] Im C (complex vectors only).
// Site pass sp (passes n_pair_pass ...), NA - 1 site orbits each: [g] S of orbit sp * (NA - 1) + g with the site mask
// site_mask[..] (0 past the last orbit),  [NA - 1] norm2 (read from the first site pass).
struct CorrRepr {
    const ReprDev *R;                                        // binomials and characters (staged in LDS)
    const uint64_t *tab, *reps;
    const uint8_t *info;
    const int64_t *chunk_pos;
    int64_t dim;
    int n_tab, n_sites, n_trans, n_chunks, n_pair_pass, want_pm, want_zz;
    const int32_t *slot_start, *slot_nu;
    const uint32_t *pairs;
    const uint64_t *site_mask;
    const d2 *xg;                                            // exactly one of xg / xr
    const double *xr;
    double *partials;
};

template <bool REALX, int BLOCK, bool TABLDS>
__global__ __launch_bounds__(BLOCK) void k_corr_repr(CorrRepr t)
{
    constexpr int G = kReprGroup, NA = repr_acc<REALX>();
    extern __shared__ __attribute__((aligned(16))) uint64_t cr_lds[];
    __shared__ double red[NA * (BLOCK / 64)];
    const ReprDev &R = *t.R;
    const int tid = threadIdx.x, pass = blockIdx.y;
    const int n_binom = (t.n_sites + 1) * kBinomRow;
    uint64_t *binom = cr_lds + (TABLDS ? t.n_tab : 0);                    // [(n_sites + 1) * 34]
    double *chr = reinterpret_cast<double *>(binom + n_binom);            // [2 * n_trans]
    if (TABLDS)
        for (int k = tid; k < t.n_tab; k += BLOCK) cr_lds[k] = t.tab[k];
    for (int k = tid; k < n_binom; k += BLOCK) binom[k] = (&R.h.binom[0][0])[k];
    for (int k = tid; k < 2 * t.n_trans; k += BLOCK) chr[k] = R.chr[k];
    __syncthreads();
    const uint64_t *tab = TABLDS ? cr_lds : t.tab;
    const bool want_pm = t.want_pm != 0, want_zz = t.want_zz != 0;
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    if (pass < t.n_pair_pass) {
        int k0[G + 1], nu[G];
        corr_group_bounds<G>(t.slot_start, pass * G, k0);
#pragma unroll
        for (int g = 0; g < G; ++g) nu[g] = (int)corr_uniform((uint32_t)t.slot_nu[pass * G + g]);
        for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
            const uint8_t ci = t.info[row];
            if (ci & 0x80) continue;                                      // zero norm at this momentum: its entry is never read
            const uint64_t a = t.reps[row];
            const double sa = (double)(ci & 0x7f);
            const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
            const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                int u = 0;
                double sr = 0.0, si = 0.0;
#pragma unroll 1
                for (int k = k0[g]; k < k0[g + 1]; ++k) {
                    const uint32_t pr = t.pairs[k];
                    const int p = (int)(pr & 255u), q = (int)((pr >> 8) & 255u);
                    const uint64_t m = (1ULL << p) | (1ULL << q), am = a & m;
                    if (am == 0 || am == m) continue;                     // equal bits: nothing to flip
                    ++u;
                    if (!want_pm) continue;
                    // the up site is the one whose bit is clear: orientation (p, q) when that is p, (q, p) otherwise
                    const bool fwd = (pr >> (((am >> p) & 1ULL) ? 17 : 16)) & 1u;
                    const uint64_t c = a ^ m;
                    uint64_t b = c;
                    int gs = 0;
                    for (int gg = 1; gg < t.n_trans; ++gg) {
                        const uint64_t im = repr_translate(tab, t.n_chunks, gg, c);
                        if (im < b) {
                            b = im;
                            gs = gg;
                        }
                    }
                    uint64_t rk = 0, bb = b;                              // heis_rank from the staged binomials
                    for (int kk = 1; bb; ++kk) {
                        rk += binom[(__ffsll((long long)bb) - 1) * kBinomRow + kk];
                        bb &= bb - 1;
                    }
                    const int64_t lo = sector_dir_find(t.reps, t.chunk_pos, t.dim, b, rk);
                    const uint8_t cj = t.info[lo];
                    if (cj & 0x80) continue;                              // zero-norm target: dropped
                    const double f = sqrt((double)(cj & 0x7f) / sa);
                    const double zr = f * chr[2 * gs], zi = -f * chr[2 * gs + 1];      // conj(chi(g*)) sqrt(|S_b|/|S_a|)
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
                if (want_zz) acc[g] += w * (0.25 * (double)(nu[g] - 2 * u));
                acc[G + g] += sr;
                if (!REALX) acc[(REALX ? 1 : 2) * G + g] += si;
            }
        }
    } else {
        constexpr int NS = NA - 1;
        const int sp = pass - t.n_pair_pass;
        uint64_t mk[NS];
#pragma unroll
        for (int g = 0; g < NS; ++g) mk[g] = corr_uniform(t.site_mask[sp * NS + g]);
        for (int64_t row = (int64_t)blockIdx.x * BLOCK + tid; row < t.dim; row += stride) {
            if (t.info[row] & 0x80) continue;
            const uint64_t a = t.reps[row];
            const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
            const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
            for (int g = 0; g < NS; ++g) acc[g] += w * (0.5 * (double)__popcll(mk[g]) - (double)__popcll(a & mk[g]));
            acc[NS] += w;
        }
    }
    corr_block_partials<NA, BLOCK>(acc, red, t.partials);
}

// ------------------------------------------------------------------------------------------------------ host side --
// dynamic LDS of a launch: binomials and characters, and the translation tables when all of it fits the budget
size_t repr_lds_small(int n_sites, int n_trans) { return ((size_t)(n_sites + 1) * kBinomRow + 2 * (size_t)n_trans) * 8; }
bool repr_tab_lds(int n_sites, int n_trans, size_t n_tab) { return repr_lds_small(n_sites, n_trans) + n_tab * 8 <= kCorrLdsCap; }

enum { kReprPair = 0, kReprSite = 1 };

template <bool REALX>
int corr_repr_run(const char *who, CorrRepr t, const ReprClasses &K, size_t n_tab, bool want_pairs, std::vector<double> &comp,
                  CorrPasses &rp, hipStream_t s, std::vector<void *> &pool)
{
    constexpr int G = kReprGroup, NA = repr_acc<REALX>(), NS = NA - 1;
    rp.add(kReprPair, want_pairs ? K.n_cls : 0, G);
    rp.add(kReprSite, K.n_orb, NS);
    const int n_pair_pass = rp.count[kReprPair], n_site_pass = rp.count[kReprSite];
    std::vector<int32_t> slot_start((size_t)n_pair_pass * G + 1, 0), slot_nu((size_t)n_pair_pass * G + 1, 0);
    std::vector<uint32_t> pairs;
    for (int c = 0; c < n_pair_pass * G; ++c) {
        slot_start[(size_t)c] = (int32_t)pairs.size();
        if (c < K.n_cls) {
            slot_nu[(size_t)c] = K.nu[(size_t)c];
            pairs.insert(pairs.end(), K.pairs[(size_t)c].begin(), K.pairs[(size_t)c].end());
        }
    }
    slot_start[(size_t)n_pair_pass * G] = (int32_t)pairs.size();
    std::vector<uint64_t> site_mask((size_t)n_site_pass * NS, 0ULL);
    std::copy(K.mask.begin(), K.mask.end(), site_mask.begin());
    int32_t *d_start = nullptr, *d_nu = nullptr;
    uint32_t *d_pairs = nullptr;
    uint64_t *d_mask = nullptr;
    QBH_TRY(upload(slot_start, &d_start, pool));
    QBH_TRY(upload(slot_nu, &d_nu, pool));
    QBH_TRY(upload(pairs, &d_pairs, pool));
    QBH_TRY(upload(site_mask, &d_mask, pool));
    t.n_pair_pass = n_pair_pass;
    t.slot_start = d_start;
    t.slot_nu = d_nu;
    t.pairs = d_pairs;
    t.site_mask = d_mask;
    const bool tab_lds = repr_tab_lds(t.n_sites, t.n_trans, n_tab);
    const size_t lds = repr_lds_small(t.n_sites, t.n_trans) + (tab_lds ? n_tab * 8 : 0);
    const ReprShape shape = repr_launch_shape(lds, t.dim);
    const bool large = tab_lds && shape.large;                            // then one workgroup of 1024 lanes per CU
    void (*kernel)(CorrRepr) = !tab_lds ? k_corr_repr<REALX, kReprBlockS, false>
                         : large  ? k_corr_repr<REALX, kReprBlockL, true>
                                  : k_corr_repr<REALX, kReprBlockS, true>;
    return corr_reduce_launch(who, kernel, shape.gx, rp.n_pass, NA, large ? kReprBlockL : kReprBlockS, lds, s, t, nullptr, pool,
                              comp);
}

}  // namespace
}  // namespace qbh

extern "C" int qbh_corr_spin_repr_dev(int n_sites, int n_dn, int n_trans, const int32_t *perms, const double *chars,
                                      const qbh_z *d_vec, const double *d_vec_re, double *norm2, double *sz, double *zz, qbh_z *pm,
                                      int64_t *dim_out, void *stream)
{
    using namespace qbh;
    const char *who = "qbh_corr_spin_repr_dev";
    if (!perms || !chars || n_sites <= 0 || n_sites > 62 || n_dn < 0 || n_dn > n_sites || n_dn > 33 || n_trans < 1 ||
        n_trans > kReprMaxTrans) {
        set_error("%s: invalid argument (1 .. 62 sites, n_dn in 0 .. min(n_sites, 33), 1 .. %d translations)", who, kReprMaxTrans);
        return QBH_EINVAL;
    }
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    std::vector<ReprDev> rr(1);
    ReprDev &R = rr[0];
    std::vector<uint64_t> tab;
    QBH_TRY(repr_symmetry(R, tab, n_sites, n_dn, n_trans, perms, chars, who));
    if (d_vec_re != nullptr) QBH_TRY(repr_real_characters(who, R.chr, n_trans));
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));           // every refusal comes before the device is looked for
    QBH_TRY(corr_check_device());
    const int N = n_sites;
    const ReprClasses K = repr_classes(N, n_trans, perms);
    DevBufs bufs;
    SectorDev<ReprDev> S;
    int64_t *d_pos = nullptr;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who, &d_pos));
    CorrRepr t{};
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
    t.want_pm = pm ? 1 : 0;
    t.want_zz = zz ? 1 : 0;
    t.xg = reinterpret_cast<const d2 *>(d_vec);
    t.xr = d_vec_re;
    const bool rx = d_vec_re != nullptr, want_pairs = zz != nullptr || pm != nullptr;
    std::vector<double> comp;
    CorrPasses rp;
    if (rx) QBH_TRY(corr_repr_run<true>(who, t, K, tab.size(), want_pairs, comp, rp, (hipStream_t)stream, bufs.pool));
    else    QBH_TRY(corr_repr_run<false>(who, t, K, tab.size(), want_pairs, comp, rp, (hipStream_t)stream, bufs.pool));
    const int G = kReprGroup, NA = rx ? repr_acc<true>() : repr_acc<false>(), NS = NA - 1;
    const double n2 = rp.at(comp, kReprSite, 0, NS, 1, NA);
    if (norm2) *norm2 = n2;
    if (dim_out) *dim_out = S.dim;
    std::vector<double> szv((size_t)N);
    for (int i = 0; i < N; ++i) {
        const int o = K.orb[(size_t)i];
        szv[(size_t)i] = rp.at(comp, kReprSite, o, NS, 0, NA) / (double)K.n_s[(size_t)o];
    }
    if (sz) std::copy(szv.begin(), szv.end(), sz);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const size_t ij = (size_t)i * N + j;
            if (i == j) {
                if (zz) zz[ij] = 0.25 * n2;
                if (pm) pm[ij] = qbh_z{0.5 * n2 + szv[(size_t)i], 0.0};
                continue;
            }
            const int c = K.cls[ij];
            const double n_u = (double)K.nu[(size_t)c];
            if (zz) zz[ij] = rp.at(comp, kReprPair, c, G, 0, NA) / n_u;
            if (pm)
                pm[ij] = repr_herm_value(rp.at(comp, kReprPair, c, G, 1, NA), (rx || K.self[(size_t)c]) ? 0.0 : rp.at(comp, kReprPair, c, G, 2, NA),
                                         2.0 * n_u, K.fwd[ij] != 0);
        }
    return QBH_OK;
}
