// qbh_corr_repr.hpp -- what the momentum-sector correlation calls share (qbh_corr_repr.hip: spin-1/2; qbh_corr_hubrepr.hip:
// two-species fermions; qbh_corr_quditrepr.hip: d-level sites; qbh_corr_kondorepr.hip: the Kondo lattice): the classes of site
// pairs, the orbits of ordered site pairs and the orbits of sites under the group (host), the block reduction of a workgroup of
// any size into partials[blockIdx.x][pass][accumulator], the shape of a launch from its LDS footprint and the check of the
// characters of a packed-real vector.  Internal linkage, like qbh_sector.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "qbh_device.hpp"

namespace qbh {
namespace {

// acc summed over the workgroup into partials[(blockIdx.x * gridDim.y + blockIdx.y) * NA ..]: every wavefront, then lane c
// adds the wavefronts of accumulator c in order (corr_block_partials for a workgroup of BLOCK lanes)
template <int NA, int BLOCK>
__device__ __forceinline__ void repr_block_partials(double (&acc)[NA], double *red, double *partials)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NA; ++c) red[c * (BLOCK / 64) + wave] = acc[c];
    }
    __syncthreads();
    if (tid < NA) {
        double s = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) s += red[tid * (BLOCK / 64) + w];
        partials[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * NA + tid] = s;
    }
}

// Two ordered site pairs are in one orbit when a group element carries one to the other; a class is an orbit together with its
// mirror image (q, p).  One orbit of every class is called forward.  The orbits are found by union-find, so groups with
// reflections and subgroups whose action on the sites is not transitive are classified like any other.
struct ReprClasses {
    int n_cls = 0, n_orb = 0;
    std::vector<int> cls, fwd;                   // [N * N]: class of (i, j) (-1 on the diagonal) and whether (i, j) is forward
    std::vector<int> nu, self;                   // [n_cls]: unordered pairs in the class; the class is its own mirror
    std::vector<std::vector<uint32_t>> pairs;    // [n_cls]: pair words p | q << 8 | fwd(p, q) << 16 | fwd(q, p) << 17, p < q
    std::vector<int> orb, n_s;                   // [N]: orbit of a site; [n_orb]: its size
    std::vector<uint64_t> mask;                  // [n_orb]
};

inline int uf_find(std::vector<int> &par, int v)
{
    while (par[(size_t)v] != v) v = par[(size_t)v] = par[(size_t)par[(size_t)v]];
    return v;
}

// every set is named by its smallest member: rep[v]
inline std::vector<int> uf_smallest(std::vector<int> &par)
{
    const int n = (int)par.size();
    std::vector<int> low((size_t)n, n), rep((size_t)n);
    for (int v = 0; v < n; ++v) {
        const int r = uf_find(par, v);
        low[(size_t)r] = std::min(low[(size_t)r], v);
    }
    for (int v = 0; v < n; ++v) rep[(size_t)v] = low[(size_t)uf_find(par, v)];
    return rep;
}

inline ReprClasses repr_classes(int N, int n_trans, const int32_t *perms)
{
    ReprClasses K;
    std::vector<int> pp((size_t)N * N), ps((size_t)N);
    std::iota(pp.begin(), pp.end(), 0);
    std::iota(ps.begin(), ps.end(), 0);
    for (int g = 1; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * N;
        for (int i = 0; i < N; ++i) {
            ps[(size_t)uf_find(ps, i)] = uf_find(ps, pg[i]);
            for (int j = 0; j < N; ++j) pp[(size_t)uf_find(pp, i * N + j)] = uf_find(pp, pg[i] * N + pg[j]);
        }
    }
    const std::vector<int> orep = uf_smallest(pp), srep = uf_smallest(ps);
    K.cls.assign((size_t)N * N, -1);
    K.fwd.assign((size_t)N * N, 0);
    std::vector<int> id((size_t)N * N, -1);                               // class of a key (the smaller of the two orbit names)
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            if (i == j) continue;
            const int o = orep[(size_t)i * N + j], om = orep[(size_t)j * N + i], key = std::min(o, om);
            if (id[(size_t)key] < 0) {
                id[(size_t)key] = K.n_cls++;
                K.nu.push_back(0);
                K.self.push_back(o == om ? 1 : 0);
                K.pairs.emplace_back();
            }
            K.cls[(size_t)i * N + j] = id[(size_t)key];
            K.fwd[(size_t)i * N + j] = o == key ? 1 : 0;
        }
    for (int p = 0; p < N; ++p)
        for (int q = p + 1; q < N; ++q) {
            const int c = K.cls[(size_t)p * N + q];
            ++K.nu[(size_t)c];
            K.pairs[(size_t)c].push_back((uint32_t)p | ((uint32_t)q << 8) | ((uint32_t)K.fwd[(size_t)p * N + q] << 16) |
                                         ((uint32_t)K.fwd[(size_t)q * N + p] << 17));
        }
    K.orb.assign((size_t)N, -1);
    std::vector<int> sid((size_t)N, -1);
    for (int i = 0; i < N; ++i) {
        const int r = srep[(size_t)i];
        if (sid[(size_t)r] < 0) {
            sid[(size_t)r] = K.n_orb++;
            K.n_s.push_back(0);
            K.mask.push_back(0ULL);
        }
        K.orb[(size_t)i] = sid[(size_t)r];
        ++K.n_s[(size_t)sid[(size_t)r]];
        K.mask[(size_t)sid[(size_t)r]] |= 1ULL << i;
    }
    return K;
}

// the pair words of all classes in class order: those of class c are pairs[cls_start[c] .. cls_start[c + 1]); cls_start is padded
// with the total for `pad` entries beyond the last class, so a pass reads the bounds of its whole group without a check
inline void repr_flatten_classes(const ReprClasses &K, int pad, std::vector<int32_t> &cls_start, std::vector<uint32_t> &pairs)
{
    cls_start.assign((size_t)K.n_cls + pad + 1, 0);
    pairs.clear();
    for (int c = 0; c < K.n_cls; ++c) {
        cls_start[(size_t)c] = (int32_t)pairs.size();
        pairs.insert(pairs.end(), K.pairs[(size_t)c].begin(), K.pairs[(size_t)c].end());
    }
    for (size_t c = (size_t)K.n_cls; c < cls_start.size(); ++c) cls_start[c] = (int32_t)pairs.size();
    if (pairs.empty()) pairs.push_back(0u);                               // one site: no pairs, and nothing reads this word
}

// The orbits of ORDERED site pairs, the diagonal pairs (i, i) included (they form orbits of their own), for correlations that are
// not Hermitian in (i, j) (qbh_corr_kondorepr.hip: <S^z_i n_j>, <S^+_i s^-_j>): value[i][j] = (sum over the pairs of the orbit of
// (i, j)) / size.
struct ReprOrbits {
    int n_orb = 0;
    std::vector<int> orb;                        // [N * N]: orbit of (i, j)
    std::vector<int> size;                       // [n_orb]: ordered pairs in the orbit
    std::vector<std::vector<uint32_t>> pairs;    // [n_orb]: pair words p | q << 8
};

inline ReprOrbits repr_ordered_orbits(int N, int n_trans, const int32_t *perms)
{
    ReprOrbits O;
    std::vector<int> pp((size_t)N * N);
    std::iota(pp.begin(), pp.end(), 0);
    for (int g = 1; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * N;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) pp[(size_t)uf_find(pp, i * N + j)] = uf_find(pp, pg[i] * N + pg[j]);
    }
    const std::vector<int> orep = uf_smallest(pp);
    O.orb.assign((size_t)N * N, -1);
    std::vector<int> id((size_t)N * N, -1);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const int r = orep[(size_t)i * N + j];
            if (id[(size_t)r] < 0) {
                id[(size_t)r] = O.n_orb++;
                O.size.push_back(0);
                O.pairs.emplace_back();
            }
            const int o = id[(size_t)r];
            O.orb[(size_t)i * N + j] = o;
            ++O.size[(size_t)o];
            O.pairs[(size_t)o].push_back((uint32_t)i | ((uint32_t)j << 8));
        }
    return O;
}

// as repr_flatten_classes, for the ordered orbits
inline void repr_flatten_orbits(const ReprOrbits &O, int pad, std::vector<int32_t> &orb_start, std::vector<uint32_t> &pairs)
{
    orb_start.assign((size_t)O.n_orb + pad + 1, 0);
    pairs.clear();
    for (int o = 0; o < O.n_orb; ++o) {
        orb_start[(size_t)o] = (int32_t)pairs.size();
        pairs.insert(pairs.end(), O.pairs[(size_t)o].begin(), O.pairs[(size_t)o].end());
    }
    for (size_t o = (size_t)O.n_orb; o < orb_start.size(); ++o) orb_start[o] = (int32_t)pairs.size();
}

// The shape of a launch from the dynamic LDS of a workgroup: workgroups of 256 lanes while four or more fit a CU (at most four
// are used), one of 1024 lanes otherwise; gx = the resident grid along x, at most one workgroup per piece of `block` rows.
constexpr int kReprBlockS = 256, kReprBlockL = 1024;
constexpr int kReprPerCuS = 4;                               // workgroups of 256 lanes per CU at most
constexpr size_t kReprLdsCu = (size_t)160 * 1024;
constexpr size_t kReprLdsStatic = 4096;                      // the reduction scratch of a workgroup and allocation granules

struct ReprShape {
    bool large;
    int block, gx;
};

inline ReprShape repr_launch_shape(size_t lds, int64_t dim)
{
    const int fit = (int)(kReprLdsCu / (lds + kReprLdsStatic));
    ReprShape s;
    s.large = fit < 4;
    s.block = s.large ? kReprBlockL : kReprBlockS;
    const int per_cu = s.large ? 1 : std::min(kReprPerCuS, fit);
    const int64_t nblk = (dim + s.block - 1) / s.block;
    s.gx = (int)std::max<int64_t>(1, std::min<int64_t>(nblk, (int64_t)device_cu_count() * per_cu));
    return s;
}

// A packed-real vector needs real characters.  A character computed as exp(-i k.t) at k = pi carries sin(pi t): an imaginary
// part below 1e-13 is that rounding (qbh_mf_kondo_repr) and is dropped, anything larger is a complex character.
inline int repr_real_characters(const char *who, double *chr, int n_trans)
{
    for (int g = 0; g < n_trans; ++g) {
        if (std::fabs(chr[2 * g + 1]) > 1e-13) {
            set_error("%s: d_vec_re needs real characters, and the character of translation %d is complex", who, g);
            return QBH_EINVAL;
        }
        chr[2 * g + 1] = 0.0;
    }
    return QBH_OK;
}

}  // namespace
}  // namespace qbh
