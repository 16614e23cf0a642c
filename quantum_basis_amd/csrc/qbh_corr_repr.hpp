// qbh_corr_repr.hpp -- what the momentum-sector correlation calls share on top of qbh_corr.hpp (qbh_corr_repr.hip: spin-1/2;
// qbh_corr_hubrepr.hip: two-species fermions; qbh_corr_quditrepr.hip: d-level sites; qbh_corr_kondorepr.hip: the Kondo lattice):
// the classes of site pairs, the orbits of ordered site pairs and the orbits of sites under the group, and the checks of the
// symmetry arguments; all of it host code.  Internal linkage, like qbh_sector.hpp, which comes first.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "qbh_device.hpp"

namespace qbh {
namespace {

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

// the orbits of the ordered site pairs under the group: [i * N + j] = the smallest member of the orbit of (i, j)
inline std::vector<int> repr_pair_orbits(int N, int n_trans, const int32_t *perms)
{
    std::vector<int> pp((size_t)N * N);
    std::iota(pp.begin(), pp.end(), 0);
    for (int g = 1; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * N;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) pp[(size_t)uf_find(pp, i * N + j)] = uf_find(pp, pg[i] * N + pg[j]);
    }
    return uf_smallest(pp);
}

inline ReprClasses repr_classes(int N, int n_trans, const int32_t *perms)
{
    ReprClasses K;
    const std::vector<int> orep = repr_pair_orbits(N, n_trans, perms);
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
        const int r = orep[(size_t)i * N + i] / (N + 1);                  // the orbit of (i, i) is that of site i: its smallest site
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

// the pair words of all classes (or ordered orbits) in order: those of list c are words[start[c] .. start[c + 1]); start is padded
// with the total for `pad` entries beyond the last list, so a pass reads the bounds of its whole group without a check
inline void repr_flatten(const std::vector<std::vector<uint32_t>> &lists, int pad, std::vector<int32_t> &start, std::vector<uint32_t> &words)
{
    start.assign(lists.size() + pad + 1, 0);
    words.clear();
    for (size_t c = 0; c < lists.size(); ++c) {
        start[c] = (int32_t)words.size();
        words.insert(words.end(), lists[c].begin(), lists[c].end());
    }
    for (size_t c = lists.size(); c < start.size(); ++c) start[c] = (int32_t)words.size();
    if (words.empty()) words.push_back(0u);                               // one site has no classes, and nothing reads this word
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
    const std::vector<int> orep = repr_pair_orbits(N, n_trans, perms);
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

// A Hermitian gathered group of a class: value[i][j] = C / div for (i, j) forward, its conjugate otherwise (the caller passes
// im = 0 for a packed-real vector and for a class that is its own mirror)
inline qbh_z repr_herm_value(double re, double im, double div, bool forward)
{
    const double v = im / div;
    return qbh_z{re / div, forward ? v : -v};
}

// the refusals of the symmetry arguments (QBH_EINVAL); qbh_corr_spin_repr_dev has one message of its own for all its arguments
inline int repr_check_tables(const char *who, const int32_t *perms, const double *chars)
{
    if (perms && chars) return QBH_OK;
    set_error("%s: perms and chars must be given", who);
    return QBH_EINVAL;
}

inline int repr_check_trans(const char *who, int n_trans)
{
    if (n_trans >= 1 && n_trans <= kReprMaxTrans) return QBH_OK;
    set_error("%s: n_trans = %d (1 .. %d allowed)", who, n_trans, kReprMaxTrans);
    return QBH_EINVAL;
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
