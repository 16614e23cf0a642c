// qbh_corr_quditrepr.hip -- qbh_corr_qudit_repr_dev: all-pair static correlations and string order of a state of d-level sites
// held in a MOMENTUM SECTOR (basis of qbh_gen_qudit_repr / qbh_mf_qudit_repr: all orbit representatives of the words of charge
// `total`, ascending), in one pass over the representatives.  The result is what qbh_corr_qudit_dev returns on the unfolded state.
//
// With T_g |w> = |g(w)> (the level of site s goes to site perms[g][s]), |a, k> = (|G| |S_a|)^(-1/2) sum_g chi(g) T_g |a>,
// Psi = sum_a psi_a |a, k> (representatives of zero norm left out, their entries never read) and w_a = |psi_a|^2, an observable
// that is diagonal in the words is sum_a w_a (1/|G|) sum_g D(g a), and g a carries at site i the level a has at g^-1(i): the sum
// over g only sees the IMAGES of the sites the observable names, evaluated on the representative word itself.
//   norm2            = sum_a w_a
//   pop[s][l]        = sum_a w_a (1/n_s) #{sites p in the orbit of s with l_p = l}
//   dd[a][b][i][j]   = sum_a w_a (1/|O|) sum_{(p, q) in O(i, j)} f_a(l_p) f_b(l_q),   O(i, j) the orbit of the ORDERED pair
//   str[i][j], i < j = sum_a w_a (1/|orbit(m)|) sum_{m' in orbit(m)} h(l_e1') h(l_e2') prod_{k in M'} g(l_k)
//                      m = ({i, j}, {k: i < k < j}) a DECORATED STRING (two end sites and the set of middle sites), the group
//                      acting on it site by site; the images of an index interval need not be intervals (wrapped strings of a
//                      ring, reflections, tori), which is why M travels as a set
//   aa[i][j]         = <A_i A+_j> = (1/|O|) sum_a sum_{(p, q) in O(i, j), l_p >= 1, l_q <= d - 2}
//                      lower[l_p] lower[l_q + 1] sqrt(|S_b| / |S_a|) chi(g*) conj(psi_b) psi_a,
//                      c = a with l_p - 1 and l_q + 1,  b = g* c its representative (skipped when b has zero norm)
// aa is the column form of the row entry of qrepr_value: <b, k| A_p A+_q |a, k> = <c|A_p A+_q|a> chi(g*) sqrt(|S_b|/|S_a|), whose
// conjugate transpose is the row convention of qbh_gen_qudit_repr.  Nothing is divided by norm2.
//
// Classes.  Site pairs: qbh_corr_repr.hpp (an orbit of ordered pairs and its mirror image; one of the two orbits is forward).  The
// kernel sums over the FORWARD orbit only: a pair word p < q carries one bit per orientation, (p, q) and (q, p), that says whether
// it is forward.  A class that is not its own mirror has exactly one forward orientation per unordered pair -- one gather per
// unordered pair at most -- and the mirror orientation gets dd[b][a] resp. the conjugate of aa on the host.  A class that is its
// own mirror holds both orientations of every pair in ONE orbit, so both are summed (half an orbit is not invariant under the
// group); its aa is real.  Strings: union-find over the decorated strings reached from the N (N - 1) / 2 seeds; a member record
// is two site bytes and the 64-bit set M, stored with bit s * bits for site s (the layout of the packed word), so that
// popcount(level mask & M) needs no bit compaction.
//
// Launch: (row blocks) x (passes), one lane per representative, grid-stride over a resident grid.  kQrAcc = 16 accumulators per
// pass, indexed by compile-time constants only:
//   DD    16 / KP^2 classes x the KP^2 table pairs (KP = 1, 2 or 4 >= n_diag, zero tables added):  [g KP^2 + a KP + b]   no gather
//   STR   16 string classes:  [g]; per row the level masks lm[l] (bit s * bits set when l_s = l) are built once, a member costs two
//         table reads for its ends and, per level, a popcount and gpow[l][popcount(lm[l] & M)] = g(l)^n from LDS         no gather
//   PAIR  8 pair classes:  [g] Re, [8 + g] Im (complex vectors only); a hit canonicalises c with the byte-sliced translation tables,
//         ranks b with the counting table (qd_rank) and finds it through the directory of the enumeration (sector_dir_find)
//   SITE  15 / LV site orbits x LV levels (LV = 3, 5 or 8 >= d):  [g LV + l] = sum w_a popcount(lm[l] & orbit), [15] norm2 (read
//         from the first site pass)
// A group that is not asked for has no passes; it changes neither the grid along x nor any other accumulator, so the other outputs
// keep their bits.  Every workgroup leaves its sums at partials[blockIdx.x][pass][accumulator] (corr_block_partials) and
// k_corr_reduce adds the workgroups in a fixed order (corr_reduce_launch): no atomics, two calls return the same bits.
//
// Tables.  The counting table cum (at most 33 KB), the characters, the operator tables (512 B) and gpow (4160 B) are staged in LDS
// by the passes that read them.  The translation tables join them when everything fits kCorrLdsCap (150 KB); 64 translations x 11
// chunks are 360 KB and are read from global memory instead (second instance), so no shape that qbh_gen_qudit_repr accepts is
// refused here.  The LDS footprint chooses between workgroups of 256 lanes and one of 1024 (repr_launch_shape).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), 0 bytes of scratch in every instance; the static LDS is
// the reduction scratch, the tables are dynamic LDS on top of it:
//   k_corr_quditrepr<vector, lanes, tables>   VGPRs  SGPRs  wavefronts/SIMD  static LDS  scratch
//   <complex,  256, LDS>                        126    106        4            512 B       0
//   <complex, 1024, LDS>                        104    106        4           2048 B       0
//   <complex,  256, global>                     126    106        4            512 B       0
//   <real,     256, LDS>                        124    106        4            512 B       0
//   <real,    1024, LDS>                         96    106        5           2048 B       0
//   <real,     256, global>                     124    106        4            512 B       0
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "qbh_sector.hpp"
#include "qbh_device.hpp"
#include "qbh_corr.hpp"                                      // device helpers, launch path, pass layout and host fills
#include "qbh_corr_repr.hpp"                                 // classes and orbits of site pairs, symmetry checks

namespace qbh {
namespace {

constexpr int kQrAcc = 16;                                   // accumulators of a pass
constexpr int kQrStr = kQrAcc, kQrGat = kQrAcc / 2;          // string classes / pair classes of a pass
enum { kQrKindDD = 0, kQrKindStr = 1, kQrKindPair = 2, kQrKindSite = 3 };
constexpr int kQrTabStride = 8;                              // entries per operator table (d <= 8)
enum { kQrEnd = 0, kQrLow = 1, kQrUp = 2, kQrDiag = 3, kQrTables = 7 };          // optab[T * 8 + l]
constexpr int kQrPow = 65;                                   // gpow[l][0 .. 64]
constexpr int kQrOps = kQrTables * kQrTabStride + kQuditMaxD * kQrPow;          // operator tables | gpow, doubles

// The pair words of class c are pairs[cls_start[c] .. cls_start[c + 1]) (qbh_corr_repr.hpp), the members of string class c are
// str_mask / str_ends[str_start[c] .. str_start[c + 1]) (ends = e1 | e2 << 8); both start arrays are padded with the total beyond
// the last class, so a pass reads the bounds of its whole group without a check.  Site pass sp owns the site orbits sp * (15 / LV)
// ... with the masks site_mask[..] in the layout of the packed word (0 past the last orbit).
struct CorrQuditRepr {
    const QuditReprDev *R;                                   // the characters
    const uint64_t *tab, *cum, *reps;                        // translation tables, counting table [n_sites * tw], representatives
    const uint8_t *info;
    const int64_t *chunk_pos;
    const double *ops;                                       // [kQrOps]
    int64_t dim;
    uint64_t fields;                                         // bit s * bits of every site s
    int n_tab, n_cum, n_sites, d, bits, tw, n_trans, n_chunks, kp, lv;
    int pass_end[4];                                         // passes [pass_end[k - 1], pass_end[k]) are of kind k
    const int32_t *cls_start, *str_start;
    const uint32_t *pairs, *str_ends;
    const uint64_t *str_mask, *site_mask;
    const d2 *xg;                                            // exactly one of xg / xr
    const double *xr;
    double *partials;
};

// lm[l] = the sites of word a at level l, bit s * bits for site s (F = that bit of every site).  Codes a field cannot hold for
// this d (and levels >= d, which no word of the sector has) give 0.
__device__ __forceinline__ void qr_level_masks(uint64_t a, int bits, uint64_t F, uint64_t (&lm)[kQuditMaxD])
{
    const uint64_t b0 = a & F, b1 = bits >= 2 ? (a >> 1) & F : 0ULL, b2 = bits >= 3 ? (a >> 2) & F : 0ULL;
#pragma unroll
    for (int l = 0; l < kQuditMaxD; ++l)
        lm[l] = ((l & 1) ? b0 : F & ~b0) & ((l & 2) ? b1 : F & ~b1) & ((l & 4) ? b2 : F & ~b2);
}

// DD pass lp: 16 / KP^2 classes, s[a KP + b] = sum over the forward orientations (P, Q) of the class of f_a(l_P) f_b(l_Q)
template <bool REALX, int KP>
__device__ __forceinline__ void qr_dd_pass(const CorrQuditRepr &t, const double *optab, int lp, int64_t row0, int64_t stride,
                                           double (&acc)[kQrAcc])
{
    constexpr int KK = KP * KP, GC = kQrAcc / KK;
    const int bits = t.bits;
    const uint32_t field = (1u << bits) - 1u;
    int k0[GC + 1];
    corr_group_bounds<GC>(t.cls_start, lp * GC, k0);
    for (int64_t row = row0; row < t.dim; row += stride) {
        if (t.info[row] & 0x80) continue;
        const uint64_t a = t.reps[row];
        const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
        const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
        for (int g = 0; g < GC; ++g) {
            double s[KK];
#pragma unroll
            for (int e = 0; e < KK; ++e) s[e] = 0.0;
#pragma unroll 1
            for (int k = k0[g]; k < k0[g + 1]; ++k) {
                const uint32_t pr = corr_uniform(t.pairs[k]);
                const int p = (int)(pr & 255u), q = (int)((pr >> 8) & 255u);
                const double *fp = optab + kQrDiag * kQrTabStride + ((uint32_t)(a >> (p * bits)) & field);
                const double *fq = optab + kQrDiag * kQrTabStride + ((uint32_t)(a >> (q * bits)) & field);
                double vp[KP], vq[KP];
#pragma unroll
                for (int e = 0; e < KP; ++e) {
                    vp[e] = fp[e * kQrTabStride];
                    vq[e] = fq[e * kQrTabStride];
                }
                if (pr & (1u << 16)) {                                    // (p, q) is forward
#pragma unroll
                    for (int e = 0; e < KK; ++e) s[e] = fma(vp[e / KP], vq[e % KP], s[e]);
                }
                if (pr & (1u << 17)) {                                    // (q, p) is forward
#pragma unroll
                    for (int e = 0; e < KK; ++e) s[e] = fma(vq[e / KP], vp[e % KP], s[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < KK; ++e) acc[g * KK + e] = fma(w, s[e], acc[g * KK + e]);
        }
    }
}

// SITE pass lp: 15 / LV site orbits x LV levels, and norm2
template <bool REALX, int LV>
__device__ __forceinline__ void qr_site_pass(const CorrQuditRepr &t, int lp, int64_t row0, int64_t stride, double (&acc)[kQrAcc])
{
    constexpr int NO = (kQrAcc - 1) / LV;
    uint64_t mk[NO];
#pragma unroll
    for (int g = 0; g < NO; ++g) mk[g] = corr_uniform(t.site_mask[lp * NO + g]);
    for (int64_t row = row0; row < t.dim; row += stride) {
        if (t.info[row] & 0x80) continue;
        const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
        const double w = fma(x.x, x.x, x.y * x.y);
        uint64_t lm[kQuditMaxD];
        qr_level_masks(t.reps[row], t.bits, t.fields, lm);
#pragma unroll
        for (int g = 0; g < NO; ++g) {
#pragma unroll
            for (int l = 0; l < LV; ++l) acc[g * LV + l] += w * (double)__popcll(lm[l] & mk[g]);
        }
        acc[kQrAcc - 1] += w;
    }
}

template <bool REALX, int BLOCK, bool TABLDS>
__global__ __launch_bounds__(BLOCK) void k_corr_quditrepr(CorrQuditRepr t)
{
    constexpr int NA = kQrAcc, GS = kQrStr, GH = kQrGat;
    extern __shared__ __attribute__((aligned(16))) uint64_t qr_lds[];
    __shared__ double red[NA * (BLOCK / 64)];
    const QuditReprDev &R = *t.R;
    const int tid = threadIdx.x, pass = blockIdx.y, n = t.n_sites, d = t.d, bits = t.bits;
    uint64_t *cum = qr_lds + (TABLDS ? t.n_tab : 0);                      // [n_sites * tw]
    double *chr = reinterpret_cast<double *>(cum + t.n_cum);              // [2 * n_trans]
    double *optab = chr + 2 * t.n_trans;                                  // [kQrTables * 8]
    double *gpow = optab + kQrTables * kQrTabStride;                      // [8 * 65]
    int kind = 0;
    while (pass >= t.pass_end[kind]) ++kind;
    const int lp = pass - (kind > 0 ? t.pass_end[kind - 1] : 0);          // the pass among those of its kind
    if (kind == kQrKindPair) {
        if (TABLDS)
            for (int k = tid; k < t.n_tab; k += BLOCK) qr_lds[k] = t.tab[k];
        for (int k = tid; k < t.n_cum; k += BLOCK) cum[k] = t.cum[k];
        for (int k = tid; k < 2 * t.n_trans; k += BLOCK) chr[k] = R.chr[k];
    }
    if (kind != kQrKindSite)
        for (int k = tid; k < kQrOps; k += BLOCK) optab[k] = t.ops[k];
    __syncthreads();
    const uint64_t *tab = TABLDS ? qr_lds : t.tab;
    const uint32_t field = (1u << bits) - 1u;
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * BLOCK, row0 = (int64_t)blockIdx.x * BLOCK + tid;
    if (kind == kQrKindPair) {
        int k0[GH + 1];
        corr_group_bounds<GH>(t.cls_start, lp * GH, k0);
        for (int64_t row = row0; row < t.dim; row += stride) {
            const uint8_t ci = t.info[row];
            if (ci & 0x80) continue;                                      // zero norm at this momentum: its entry is never read
            const uint64_t a = t.reps[row];
            const double sa = (double)(ci & 0x7f);
            const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
#pragma unroll
            for (int g = 0; g < GH; ++g) {
                double sr = 0.0, si = 0.0;
#pragma unroll 1
                for (int k = k0[g]; k < k0[g + 1]; ++k) {
                    const uint32_t pr = corr_uniform(t.pairs[k]);
#pragma unroll 1
                    for (int o = 0; o < 2; ++o) {                         // the orientations (p, q) and (q, p) of the pair word
                        if (!((pr >> (16 + o)) & 1u)) continue;           // not forward: the host takes it from the mirror
                        const int P = (int)((pr >> (o ? 8 : 0)) & 255u), Q = (int)((pr >> (o ? 0 : 8)) & 255u);
                        const int lP = (int)((uint32_t)(a >> (P * bits)) & field), lQ = (int)((uint32_t)(a >> (Q * bits)) & field);
                        if (lP < 1 || lQ > d - 2) continue;               // A_P A+_Q gives nothing on this word
                        const uint64_t c = a - (1ULL << (P * bits)) + (1ULL << (Q * bits));
                        uint64_t b = c;                                   // sector_canonical on the staged tables
                        int gs = 0;
                        for (int gg = 1; gg < t.n_trans; ++gg) {
                            const uint64_t im = repr_translate(tab, t.n_chunks, gg, c);
                            if (im < b) {
                                b = im;
                                gs = gg;
                            }
                        }
                        const int64_t lo = sector_dir_find(t.reps, t.chunk_pos, t.dim, b, qd_rank(cum, n, bits, t.tw, b));
                        const uint8_t cj = t.info[lo];
                        if (cj & 0x80) continue;                          // zero-norm target: dropped
                        const double cf = (optab[kQrLow * kQrTabStride + lP] * optab[kQrUp * kQrTabStride + lQ]) *
                                          sqrt((double)(cj & 0x7f) / sa);
                        const double zr = cf * chr[2 * gs], zi = cf * chr[2 * gs + 1];      // lower lower sqrt(|S_b|/|S_a|) chi(g*)
                        if (REALX) {
                            sr += zr * (t.xr[lo] * x.x);
                        } else {
                            const d2 xb = t.xg[lo];
                            const double ur = xb.x * x.x + xb.y * x.y, ui = xb.x * x.y - xb.y * x.x;      // conj(psi_b) psi_a
                            sr += zr * ur - zi * ui;
                            si += zr * ui + zi * ur;
                        }
                    }
                }
                acc[g] += sr;
                if (!REALX) acc[GH + g] += si;
            }
        }
    } else if (kind == kQrKindStr) {
        int k0[GS + 1];
        corr_group_bounds<GS>(t.str_start, lp * GS, k0);
        for (int64_t row = row0; row < t.dim; row += stride) {
            if (t.info[row] & 0x80) continue;
            const uint64_t a = t.reps[row];
            const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
            const double w = fma(x.x, x.x, x.y * x.y);
            uint64_t lm[kQuditMaxD];
            qr_level_masks(a, bits, t.fields, lm);
#pragma unroll
            for (int g = 0; g < GS; ++g) {
                double s = 0.0;
#pragma unroll 1
                for (int k = k0[g]; k < k0[g + 1]; ++k) {
                    const uint64_t M = corr_uniform(t.str_mask[k]);
                    const uint32_t ends = corr_uniform(t.str_ends[k]);
                    const int e1 = (int)(ends & 255u), e2 = (int)((ends >> 8) & 255u);
                    double v = optab[kQrEnd * kQrTabStride + ((uint32_t)(a >> (e1 * bits)) & field)] *
                               optab[kQrEnd * kQrTabStride + ((uint32_t)(a >> (e2 * bits)) & field)];
#pragma unroll
                    for (int l = 0; l < kQuditMaxD; ++l)
                        if (l < d) v *= gpow[l * kQrPow + __popcll(lm[l] & M)];
                    s += v;
                }
                acc[g] = fma(w, s, acc[g]);
            }
        }
    } else if (kind == kQrKindDD) {
        if (t.kp == 1)      qr_dd_pass<REALX, 1>(t, optab, lp, row0, stride, acc);
        else if (t.kp == 2) qr_dd_pass<REALX, 2>(t, optab, lp, row0, stride, acc);
        else                qr_dd_pass<REALX, 4>(t, optab, lp, row0, stride, acc);
    } else {
        if (t.lv == 3)      qr_site_pass<REALX, 3>(t, lp, row0, stride, acc);
        else if (t.lv == 5) qr_site_pass<REALX, 5>(t, lp, row0, stride, acc);
        else                qr_site_pass<REALX, 8>(t, lp, row0, stride, acc);
    }
    corr_block_partials<NA, BLOCK>(acc, red, t.partials);
}

// ------------------------------------------------------------------------------------------------------ host side --
// The classes of decorated strings: every seed ({i, j}, {k: i < k < j}) and everything the group makes of it, site by site.
// Union-find over the strings reached; a class keeps its distinct members.  Strings are keyed by (ends, set of middle sites), the
// ends unordered.
struct QrStrings {
    int n_cls = 0;
    std::vector<int> cls;                                    // [N * N]: class of the seed (i, j), i < j (-1 elsewhere)
    std::vector<std::vector<std::pair<uint32_t, uint64_t>>> members;      // [n_cls]: (e1 | e2 << 8, middle set by site index)
};

QrStrings qr_string_classes(int N, int n_trans, const int32_t *perms)
{
    // image of a site set under g, one table read per byte of the set
    std::vector<uint64_t> img((size_t)n_trans * 8 * 256, 0ULL);
    for (int g = 0; g < n_trans; ++g)
        for (int by = 0; by < 8; ++by)
            for (int v = 0; v < 256; ++v) {
                uint64_t m = 0;
                for (int b = 0; b < 8; ++b)
                    if (((v >> b) & 1) && by * 8 + b < N) m |= 1ULL << perms[(size_t)g * N + by * 8 + b];
                img[((size_t)g * 8 + by) * 256 + v] = m;
            }
    using Key = std::pair<uint32_t, uint64_t>;
    std::map<Key, int> id;
    std::vector<Key> node;
    std::vector<int> par;
    auto intern = [&](int e1, int e2, uint64_t M) {
        const Key k{(uint32_t)std::min(e1, e2) | ((uint32_t)std::max(e1, e2) << 8), M};
        const auto it = id.find(k);
        if (it != id.end()) return it->second;
        const int v = (int)node.size();
        id.emplace(k, v);
        node.push_back(k);
        par.push_back(v);
        return v;
    };
    std::vector<int> seed((size_t)N * N, -1);
    for (int i = 0; i < N; ++i)
        for (int j = i + 1; j < N; ++j) {
            const uint64_t upto_j = (1ULL << j) - 1ULL, upto_i = (2ULL << i) - 1ULL;      // sites below j / up to i
            seed[(size_t)i * N + j] = intern(i, j, upto_j & ~upto_i);
        }
    for (size_t v = 0; v < node.size(); ++v) {               // the list grows while new strings are reached
        const Key k = node[v];
        const int e1 = (int)(k.first & 255u), e2 = (int)(k.first >> 8);
        for (int g = 1; g < n_trans; ++g) {
            uint64_t M = 0;
            for (int by = 0; by < 8; ++by) M |= img[((size_t)g * 8 + by) * 256 + ((k.second >> (8 * by)) & 255ULL)];
            const int u = intern(perms[(size_t)g * N + e1], perms[(size_t)g * N + e2], M);
            par[(size_t)uf_find(par, (int)v)] = uf_find(par, u);
        }
    }
    QrStrings S;
    S.cls.assign((size_t)N * N, -1);
    std::vector<int> cid(node.size(), -1);
    for (int i = 0; i < N; ++i)
        for (int j = i + 1; j < N; ++j) {
            const int r = uf_find(par, seed[(size_t)i * N + j]);
            if (cid[(size_t)r] < 0) {
                cid[(size_t)r] = S.n_cls++;
                S.members.emplace_back();
            }
            S.cls[(size_t)i * N + j] = cid[(size_t)r];
        }
    for (size_t v = 0; v < node.size(); ++v) S.members[(size_t)cid[(size_t)uf_find(par, (int)v)]].push_back(node[v]);
    return S;
}

// dynamic LDS of a launch: counting table, characters, operator tables and gpow, and the translation tables when all of it fits
size_t qr_lds_small(int n_cum, int n_trans) { return ((size_t)n_cum + 2 * (size_t)n_trans + kQrOps) * 8; }

// the passes of the wanted groups, the launch and the two-stage reduction: comp[pass * kQrAcc + accumulator]
template <bool REALX>
int corr_quditrepr_run(const char *who, CorrQuditRepr t, const ReprClasses &K, const QrStrings &S, size_t n_tab, bool want_dd,
                       bool want_str, bool want_aa, CorrPasses &qp, std::vector<double> &comp, hipStream_t s, std::vector<void *> &pool)
{
    constexpr int NA = kQrAcc;
    const int no = (NA - 1) / t.lv;                          // site orbits of a site pass
    qp.add(kQrKindDD, want_dd ? K.n_cls : 0, NA / (t.kp * t.kp));
    qp.add(kQrKindStr, want_str ? S.n_cls : 0, kQrStr);
    qp.add(kQrKindPair, want_aa ? K.n_cls : 0, kQrGat);
    qp.add(kQrKindSite, K.n_orb, no);
    for (int k = 0; k < 4; ++k) t.pass_end[k] = qp.first[k] + qp.count[k];
    std::vector<int32_t> cls_start, str_start((size_t)S.n_cls + NA + 1, 0);
    std::vector<uint32_t> pairs, str_ends;
    std::vector<uint64_t> str_mask;
    repr_flatten(K.pairs, NA, cls_start, pairs);
    for (int c = 0; c < S.n_cls; ++c) {
        str_start[(size_t)c] = (int32_t)str_ends.size();
        for (const auto &m : S.members[(size_t)c]) {
            uint64_t spread = 0;                             // the middle set in the layout of the packed word
            for (int k = 0; k < t.n_sites; ++k)
                if ((m.second >> k) & 1ULL) spread |= 1ULL << (k * t.bits);
            str_ends.push_back(m.first);
            str_mask.push_back(spread);
        }
    }
    for (size_t c = (size_t)S.n_cls; c < str_start.size(); ++c) str_start[c] = (int32_t)str_ends.size();
    if (str_ends.empty()) {                                  // one site: no strings, and nothing reads these words
        str_ends.push_back(0u);
        str_mask.push_back(0ULL);
    }
    std::vector<uint64_t> site_mask((size_t)qp.count[kQrKindSite] * no, 0ULL);
    for (int o = 0; o < K.n_orb; ++o)
        for (int k = 0; k < t.n_sites; ++k)
            if ((K.mask[(size_t)o] >> k) & 1ULL) site_mask[(size_t)o] |= 1ULL << (k * t.bits);
    int32_t *d_cs = nullptr, *d_ss = nullptr;
    uint32_t *d_pairs = nullptr, *d_ends = nullptr;
    uint64_t *d_smask = nullptr, *d_mask = nullptr;
    QBH_TRY(upload(cls_start, &d_cs, pool));
    QBH_TRY(upload(str_start, &d_ss, pool));
    QBH_TRY(upload(pairs, &d_pairs, pool));
    QBH_TRY(upload(str_ends, &d_ends, pool));
    QBH_TRY(upload(str_mask, &d_smask, pool));
    QBH_TRY(upload(site_mask, &d_mask, pool));
    t.cls_start = d_cs;
    t.str_start = d_ss;
    t.pairs = d_pairs;
    t.str_ends = d_ends;
    t.str_mask = d_smask;
    t.site_mask = d_mask;
    const size_t small = qr_lds_small(t.n_cum, t.n_trans);
    const bool tab_lds = small + n_tab * 8 <= kCorrLdsCap;
    const size_t lds = small + (tab_lds ? n_tab * 8 : 0);
    const ReprShape shape = repr_launch_shape(lds, t.dim);
    const bool large = tab_lds && shape.large;               // then one workgroup of 1024 lanes per CU
    void (*kernel)(CorrQuditRepr) = !tab_lds ? k_corr_quditrepr<REALX, kReprBlockS, false>
                         : large  ? k_corr_quditrepr<REALX, kReprBlockL, true>
                                  : k_corr_quditrepr<REALX, kReprBlockS, true>;
    return corr_reduce_launch(who, kernel, shape.gx, qp.n_pass, NA, large ? kReprBlockL : kReprBlockS, lds, s, t, nullptr, pool,
                              comp);
}

}  // namespace
}  // namespace qbh

// Refusals, in this order, all before the device is looked for and before anything is written:
//   QBH_EINVAL   perms or chars NULL
//   the shape as qbh_gen_qudit_repr checks it: QBH_EINVAL below 1 site or 2 levels, QBH_EUNSUPP beyond 8 levels or 64 bits,
//                QBH_EINVAL for total outside 0 .. n_sites (d - 1)
//   QBH_EINVAL   n_trans outside 1 .. 64; not exactly one of d_vec / d_vec_re; the table checks of qbh_corr_qudit_dev in its order
//                (n_diag outside 0 .. 4, diag NULL with n_diag > 0, one string table only, dd / str / aa wanted without their
//                tables, a table value that is not finite); translation 0 not the identity; a translation that is no site
//                permutation; d_vec_re with a complex character
//   QBH_EUNSUPP  2^40 or more words in the sector `total`
//   QBH_ENODEVICE
// and after the enumeration QBH_EUNSUPP for 2^31 representatives or more.
extern "C" int qbh_corr_qudit_repr_dev(int n_sites, int d, int total, int n_trans, const int32_t *perms, const double *chars,
                                       const qbh_z *d_vec, const double *d_vec_re, int n_diag, const double *diag,
                                       const double *string_end, const double *string_mid, const double *lower, double *norm2,
                                       double *pop, double *dd, double *str, qbh_z *aa, int64_t *dim_out, void *stream)
{
    using namespace qbh;
    const char *who = "qbh_corr_qudit_repr_dev";
    QBH_TRY(repr_check_tables(who, perms, chars));
    QBH_TRY(qudit_check_shape(who, n_sites, d));
    if (total < 0 || total > n_sites * (d - 1)) {
        set_error("%s: total = %d (0 .. %d allowed)", who, total, n_sites * (d - 1));
        return QBH_EINVAL;
    }
    QBH_TRY(repr_check_trans(who, n_trans));
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    QBH_TRY(qudit_corr_check_tables(who, d, n_diag, diag, string_end, string_mid, lower, dd != nullptr, str != nullptr, aa != nullptr));
    std::vector<QuditReprDev> rr(1);
    QuditReprDev &R = rr[0];
    std::vector<uint64_t> tab;
    QBH_TRY(qrepr_symmetry(R, tab, n_sites, d, total, n_trans, perms, chars, who));
    if (d_vec_re != nullptr) QBH_TRY(repr_real_characters(who, R.chr, n_trans));
    int64_t nstates = 0;
    std::vector<uint64_t> cum;
    QBH_TRY(sector_words(R, cum, &nstates, who));            // every refusal comes before the device is looked for
    QBH_TRY(corr_check_device());
    const int N = n_sites, K = n_diag, bits = R.bits;
    const ReprClasses C = repr_classes(N, n_trans, perms);
    const QrStrings S = str ? qr_string_classes(N, n_trans, perms) : QrStrings{};
    // operator tables: h, lower[l] (the site that goes down), lower[l + 1] (the site that goes up), the diagonal tables; then
    // gpow[l][n] = g(l)^n, rounded once from long double (0^0 = 1)
    std::vector<double> ops((size_t)kQrOps, 0.0);
    for (int l = 0; l < d; ++l) {
        if (string_end) ops[(size_t)kQrEnd * kQrTabStride + l] = string_end[l];
        if (lower && l >= 1) ops[(size_t)kQrLow * kQrTabStride + l] = lower[l];
        if (lower && l + 1 < d) ops[(size_t)kQrUp * kQrTabStride + l] = lower[l + 1];
        for (int a = 0; a < K; ++a) ops[(size_t)(kQrDiag + a) * kQrTabStride + l] = diag[a * d + l];
    }
    for (int l = 0; l < kQuditMaxD; ++l) {
        long double p = 1.0L;
        for (int k = 0; k < kQrPow; ++k) {
            ops[(size_t)kQrTables * kQrTabStride + (size_t)l * kQrPow + k] = (double)p;
            p *= (string_mid && l < d) ? (long double)string_mid[l] : 1.0L;
        }
    }
    DevBufs bufs;
    SectorDev<QuditReprDev> Sec;
    int64_t *d_pos = nullptr;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, Sec, who, &d_pos));
    uint64_t *d_cum = nullptr;
    double *d_ops = nullptr;
    QBH_TRY(upload(cum, &d_cum, bufs.pool));
    QBH_TRY(upload(ops, &d_ops, bufs.pool));
    CorrQuditRepr t{};
    t.R = Sec.R;
    t.tab = Sec.tab;
    t.cum = d_cum;
    t.reps = Sec.reps;
    t.info = Sec.info;
    t.chunk_pos = d_pos;
    t.ops = d_ops;
    t.dim = Sec.dim;
    for (int k = 0; k < N; ++k) t.fields |= 1ULL << (k * bits);
    t.n_tab = (int)tab.size();
    t.n_cum = N * R.tw;
    t.n_sites = N;
    t.d = d;
    t.bits = bits;
    t.tw = R.tw;
    t.n_trans = n_trans;
    t.n_chunks = R.n_chunks;
    t.kp = K <= 1 ? 1 : K == 2 ? 2 : 4;
    t.lv = d <= 3 ? 3 : d <= 5 ? 5 : 8;
    t.xg = reinterpret_cast<const d2 *>(d_vec);
    t.xr = d_vec_re;
    const bool rx = d_vec_re != nullptr;
    std::vector<double> comp;
    CorrPasses qp;
    if (rx) QBH_TRY(corr_quditrepr_run<true>(who, t, C, S, tab.size(), dd != nullptr, str != nullptr, aa != nullptr, qp, comp, (hipStream_t)stream, bufs.pool));
    else    QBH_TRY(corr_quditrepr_run<false>(who, t, C, S, tab.size(), dd != nullptr, str != nullptr, aa != nullptr, qp, comp, (hipStream_t)stream, bufs.pool));
    constexpr int NA = kQrAcc, GH = kQrGat;
    const int KK = t.kp * t.kp, gc = NA / KK, no = (NA - 1) / t.lv;      // classes of a DD pass, site orbits of a site pass
    const size_t NN = (size_t)N * N;
    if (norm2) *norm2 = qp.at_item(comp, kQrKindSite, 0, no, t.lv, NA - 1, NA);
    if (dim_out) *dim_out = Sec.dim;
    std::vector<double> popv((size_t)N * d);
    for (int i = 0; i < N; ++i) {
        const int o = C.orb[(size_t)i];
        for (int l = 0; l < d; ++l) popv[(size_t)i * d + l] = qp.at_item(comp, kQrKindSite, o, no, t.lv, l, NA) / (double)C.n_s[(size_t)o];
    }
    if (pop) std::copy(popv.begin(), popv.end(), pop);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const size_t ij = (size_t)i * N + j;
            if (i == j) {                                    // the diagonals follow from pop, as in qbh_corr_qudit_dev
                qudit_corr_put_diag(N, i, d, K, popv.data() + (size_t)i * d, diag, string_end, lower, dd, str, aa);
                continue;
            }
            const int c = C.cls[ij];
            const bool forward = C.fwd[ij] != 0, self = C.self[(size_t)c] != 0;
            const double n_o = (self ? 2.0 : 1.0) * (double)C.nu[(size_t)c];      // the size of the forward orbit
            if (dd)
                for (int a = 0; a < K; ++a)
                    for (int b = 0; b < K; ++b) {
                        // the mirror orientation: <f_a(i) f_b(j)> = <f_b(j) f_a(i)>, (j, i) forward.  A class that is its own mirror
                        // has summed the same terms into [a][b] and [b][a] in another order: one of the two serves both, so that
                        // dd[a][b][i][j] and dd[b][a][j][i] carry the same bits there as everywhere else
                        const bool direct = self ? a <= b : forward;
                        dd[(size_t)(a * K + b) * NN + ij] = qp.at_item(comp, kQrKindDD, c, gc, KK, direct ? a * t.kp + b : b * t.kp + a, NA) / n_o;
                    }
            if (str) {
                const int sc = S.cls[(size_t)std::min(i, j) * N + std::max(i, j)];
                str[ij] = qp.at(comp, kQrKindStr, sc, kQrStr, 0, NA) / (double)S.members[(size_t)sc].size();
            }
            if (aa) aa[ij] = repr_herm_value(qp.at(comp, kQrKindPair, c, GH, 0, NA), (rx || self) ? 0.0 : qp.at(comp, kQrKindPair, c, GH, 1, NA), n_o, forward);
        }
    return QBH_OK;
}
