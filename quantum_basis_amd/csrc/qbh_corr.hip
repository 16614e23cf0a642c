// qbh_corr.hip -- all-pair static correlations of a resident state in one pass over it (no temporary vector):
//   qbh_corr_spin_dev      spin-1/2 fixed-n_dn sector (basis of qbh_gen_heisenberg):  <psi|psi>, <S^z_i>, <S^z_i S^z_j>, <S^+_i S^-_j>
//   qbh_corr_hubbard_dev   two-species fermions (basis of qbh_gen_hubbard):           <n_{i,s}>, <n_{i,a} n_{j,b}>, <c+_{i,s} c_{j,s}>,
//                                                                                     <S^+_i S^-_j>
// The kernels are the matrix-free apply kernels (qbh_mf.hip) turned round: one lane per row, the row's pattern from the
// binomials (spin) or the configuration lists (fermions), a moved pattern re-ranked through 6-bit chunk tables in LDS, and the
// gathered element REDUCED into a register accumulator instead of written to a vector.  A launch is a grid of (row blocks) x
// (passes); a pass owns a group of site pairs (or of sites) and kCorrAcc accumulators per lane, every workgroup leaves its sums
// at partials[blockIdx.x][pass][accumulator], and k_corr_reduce adds the workgroups in a fixed order, one lane per component: no
// atomics, two calls on the same input return the same bits.
// The host side of what all seven correlation calls share (qbh_corr.hpp) is defined here as well.
#include <algorithm>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_device.hpp"
#include "qbh_gen_util.hpp"
#include "qbh_corr.hpp"

namespace qbh {
namespace {

// Second stage: out[c] = sum of partials[i][c] over the workgroups i.  One lane per component (a launch has hundreds of them, and
// k_reduce_partials would walk them one after another); the 16 wavefronts of a workgroup take every 16th partial and are added in
// order, so the sum does not depend on the run.
constexpr int kCorrRedWaves = 16;

__global__ __launch_bounds__(64 * kCorrRedWaves) void k_corr_reduce(const double *partials, int nparts, int ncomp, double *out)
{
    __shared__ double sm[kCorrRedWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    double v = 0.0;
    if (c < ncomp) {
#pragma unroll 4
        for (int i = wave; i < nparts; i += kCorrRedWaves) v += partials[(size_t)i * ncomp + c];
    }
    sm[wave][lane] = v;
    __syncthreads();
    if (wave == 0 && c < ncomp) {
        double s = 0.0;
        for (int w = 0; w < kCorrRedWaves; ++w) s += sm[w][lane];
        out[c] = s;
    }
}

// ------------------------------------------------------------------------------------------------------- spin-1/2 --
// Passes 0 .. n_pair_pass - 1 own kSpinGroup pairs i < j each (mask = bit i | bit j; the list is padded with mask 0, which no row
// matches and a whole wavefront skips); the passes after them own kSpinGroup sites each.  Accumulators of a pair pass, pair g:
//   [g]                   D_ij    = sum_s |psi_s|^2 [bit i != bit j]                   (zz = (norm2 - 2 D) / 4, no gather)
//   [G + g], [2G + g]     pm_ij   = sum_{s: i down, j up} conj(psi(s ^ mask)) psi(s)   (re, im; REALX has no imaginary part)
// of a site pass:  [g] = sum_s |psi_s|^2 (1/2 - bit_site),  [G] = sum_s |psi_s|^2 (read from the first site pass).
// (One site pass over 31 sites instead of two over 16 was measured: the unrolled loop takes 186 VGPRs instead of 155, two
// wavefronts per SIMD instead of three, and the whole launch 113 ms instead of 83 at 30 sites.)
// Rows come in tiles of kCorrBlock * R (the scheme is described in qbh_corr.hpp): unranking every row in every pass would cost
// a third of the time of a pass of 16 pairs.
// W: the word of a pattern, of a rank and of the table entries -- 32 bits up to 32 sites (C(32, 16) < 2^32), 64 bits beyond.
constexpr int kSpinGroup = 16;

struct CorrSpin {
    int n_sites, n_dn, n_chunks, n_pair_pass, want_pm, want_zz;
    int64_t dim;
    const void *binom, *chunk;                   // W [(n_sites+1) * (n_dn+1)], W [n_chunks * (n_dn+1) * 64]
    const uint64_t *mask;                        // [n_pair_pass * kSpinGroup]
    const d2 *xg;                                // exactly one of xg / xr
    const double *xr;
    double *partials;
};

template <bool REALX>
constexpr int spin_acc() { return (REALX ? 2 : 3) * kSpinGroup; }

template <typename W>
constexpr int spin_rows() { return 32 / (int)sizeof(W); }        // R: rows per lane and tile (9 - 10 KB of patterns per workgroup)

__device__ __forceinline__ int corr_popc(uint32_t v) { return __popc(v); }
__device__ __forceinline__ int corr_popc(uint64_t v) { return __popcll(v); }
__device__ __forceinline__ int corr_ctz(uint32_t v) { return v ? __ffs((int)v) - 1 : 0; }
__device__ __forceinline__ int corr_ctz(uint64_t v) { return v ? __ffsll((long long)v) - 1 : 0; }

template <bool REALX, typename W, int NCH>
__global__ __launch_bounds__(kCorrBlock) void k_corr_spin(CorrSpin t)
{
    constexpr int G = kSpinGroup, NA = spin_acc<REALX>(), R = spin_rows<W>();
    extern __shared__ unsigned long long lds_u64[];
    __shared__ double red[NA * (kCorrBlock / 64)];
    const int nk = t.n_dn + 1;
    W *binom = reinterpret_cast<W *>(lds_u64);                            // [(n_sites+1) * nk]
    W *chunk = binom + (size_t)(t.n_sites + 1) * nk;                      // [n_chunks * nk * 64]
    W *stage = chunk + (size_t)t.n_chunks * nk * 64;                      // [kCorrBlock * (R + 1)]: the tile's patterns
    const int tid = threadIdx.x, pass = blockIdx.y;
    const bool pair_pass = pass < t.n_pair_pass;
    const bool want_pm = t.want_pm != 0, want_zz = t.want_zz != 0;
    for (int i = tid; i < (t.n_sites + 1) * nk; i += kCorrBlock) binom[i] = static_cast<const W *>(t.binom)[i];
    W mk[G];                                                              // this pass's pairs
#pragma unroll
    for (int g = 0; g < G; ++g) mk[g] = 0;
    if (pair_pass) {
        if (want_pm)
            for (int i = tid; i < t.n_chunks * nk * 64; i += kCorrBlock) chunk[i] = static_cast<const W *>(t.chunk)[i];
#pragma unroll
        for (int g = 0; g < G; ++g) mk[g] = corr_uniform((W)t.mask[pass * G + g]);
    }
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int site0 = (pass - t.n_pair_pass) * G;
    const int64_t tile_rows = (int64_t)kCorrBlock * R, n_tiles = (t.dim + tile_rows - 1) / tile_rows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int64_t base = tile * tile_rows;
      __syncthreads();                               // the tables are in place; the last tile's patterns have been read
      if (base + (int64_t)tid * R < t.dim) {
          // unrank (colexicographic): largest p with C(p, k) <= r, for k = n_dn .. 1
          W c = 0, r = (W)(base + (int64_t)tid * R);
          int p = t.n_sites - 1;
          for (int k = t.n_dn; k >= 1; --k) {
              while (binom[p * nk + k] > r) --p;
              c |= (W)1 << p;
              r -= binom[p * nk + k];
              --p;
          }
#pragma unroll
          for (int q = 0; q < R; ++q) {
              stage[tid * (R + 1) + q] = c;
              const W u = c | (c - 1);                                    // the next larger word with as many bits (past the last row: unused)
              c = (u + 1) | ((((~u & (u + 1)) - 1) >> corr_ctz(c)) >> 1);
          }
      }
      __syncthreads();
#pragma unroll 1
      for (int q = 0; q < R; ++q) {
        const int local = q * kCorrBlock + tid;                           // made by lane local / R at its step local % R
        const int64_t row = base + local;
        if (row >= t.dim) break;
        const W s = stage[(local / R) * (R + 1) + local % R];
        const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
        const double w = fma(x.x, x.x, x.y * x.y);
        if (!pair_pass) {
#pragma unroll
            for (int g = 0; g < G; ++g)             // sites past the last: dropped on the host
                acc[g] += ((s >> ((site0 + g) & (8 * (int)sizeof(W) - 1))) & 1) ? -0.5 * w : 0.5 * w;
            acc[G] += w;
            continue;
        }
#pragma unroll
        for (int g0 = 0; g0 < G; g0 += 8) {
            W idx[8];
            bool hits[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const W m = mk[g0 + j], sm = s & m;
                // w * (1.0 or 0.0): the two numbers differ in the high word only, one select instead of two
                if (want_zz) acc[g0 + j] = fma(w, __hiloint2double(corr_popc(sm) == 1 ? 0x3FF00000 : 0, 0), acc[g0 + j]);
                // exactly the lower site (i) of the pair is down (a padding pair has mask 0: skipped by the whole wavefront)
                const bool hit = want_pm && m != 0 && sm == (m & ((W)0 - m));
                W rk = 0;                              // read under `hit` only
                if (hit) {
                    const W f = s ^ m;
                    if (NCH > 0) {
                        const uint32_t flo = (uint32_t)f, fhi = (uint32_t)((uint64_t)f >> 30);      // chunks 0-4 | chunks 5-9
                        int below64 = 0;                                               // 64 * (particles below)
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            const int bits = (int)(((c < 5 ? flo >> (6 * c) : fhi >> (6 * (c - 5)))) & 63u);
                            rk += chunk[c * nk * 64 + below64 + bits];
                            below64 += __popc(bits) << 6;
                        }
                    } else {
                        int below = 0;
                        for (int c = 0; c < t.n_chunks; ++c) {
                            const int bits = (int)((f >> (6 * c)) & 63);
                            rk += chunk[((size_t)c * nk + below) * 64 + bits];
                            below += __popc(bits);
                        }
                    }
                }
                idx[j] = rk;
                hits[j] = hit;
            }
            // Only the lanes with a hit load and accumulate (the gathers are issued under the hit mask, eight in flight, and waited
            // for in the second loop): no select of an index or of a weight, and no line fetched for a lane that adds nothing.
            if (want_pm) {
                if (REALX) {
                    double xv[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (hits[j]) xv[j] = t.xr[idx[j]];          // xv[j] is written and read under hits[j] only
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (hits[j]) acc[G + g0 + j] = fma(xv[j], x.x, acc[G + g0 + j]);
                } else {
                    d2 xv[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (hits[j]) xv[j] = t.xg[idx[j]];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (hits[j]) {
                            acc[G + g0 + j] += fma(xv[j].x, x.x, xv[j].y * x.y);
                            acc[2 * G + g0 + j] += xv[j].x * x.y - xv[j].y * x.x;
                        }
                }
            }
        }
      }
    }
    corr_block_partials<NA>(acc, red, t.partials);
}

// ------------------------------------------------------------------------------------------- two-species fermions --
// row = ru * Nd + rd; the patterns come from the configuration lists (two loads per row), a moved pattern is re-ranked through
// one chunk table per species in LDS (32-bit entries: a species has fewer than 2^31 configurations at 31 sites).  Pass kinds,
// kHubAcc accumulators each:
//   NN    8 pairs i < j:   [g] uu, [8+g] dd, [16+g] n_{i,up} n_{j,dn}, [24+g] n_{i,dn} n_{j,up}                       no gather
//   HOPU / HOPD / FLIP  16 pairs i < j:  [g] re, [16+g] im of  sum_w conj(psi(w')) sign psi(w)                        one gather
//         HOP*: w has j occupied and i empty in the species, w' = w with the particle moved j -> i, sign = parity of the occupied
//               orbitals between the two;  FLIP: c+_{i,up} c_{i,dn} c+_{j,dn} c_{j,up}: up j -> i and down i -> j, the sign of the
//               four factors in the order of qbh_mopr_terms_dev family 1 (orbital = site + species * n_sites, ascending)
//   SITE  8 sites: [g] n_up, [8+g] n_dn, [16+g] n_up n_dn, [24] |psi|^2 (the first site pass only)                      no gather
constexpr int kHubAcc = 32;
enum { kHubNN = 0, kHubHopU = 1, kHubHopD = 2, kHubFlip = 3, kHubSite = 4 };

struct CorrHub {
    int n_sites, n_up, n_dn, n_chunks;
    int pass_end[5];                             // passes [pass_end[k-1], pass_end[k]) are of kind k
    int64_t Nu, Nd;
    const uint32_t *cfg_u, *cfg_d, *chunk_u, *chunk_d;   // chunk_s: [n_chunks * (n_s+1) * 64]
    const uint32_t *pair;                        // [n_pairs padded to 16]: i | j << 8; padding 0 (i == j: no row matches)
    const d2 *xg;
    const double *xr;
    double *partials;
};

__device__ __forceinline__ uint32_t hub_rank(const uint32_t *chunk, int n_chunks, int nk, uint32_t c)
{
    uint32_t rk = 0;
    int below = 0;
    for (int q = 0; q < n_chunks; ++q) {
        const int bits = (int)((c >> (6 * q)) & 63u);
        rk += chunk[(q * nk + below) * 64 + bits];
        below += __popc(bits);
    }
    return rk;
}

// occupied orbitals of c strictly between sites lo < hi
__device__ __forceinline__ int hub_between(uint32_t c, int lo, int hi)
{
    return __popc(c & ((1u << hi) - 1u) & ~((2u << lo) - 1u));
}

template <bool REALX>
__global__ __launch_bounds__(kCorrBlock) void k_corr_hubbard(CorrHub t)
{
    constexpr int NA = kHubAcc;
    extern __shared__ uint32_t lds_u32[];
    __shared__ double red[NA * (kCorrBlock / 64)];
    __shared__ uint32_t pair[16];
    const int nku = t.n_up + 1, nkd = t.n_dn + 1;
    uint32_t *chunk_u = lds_u32;                                          // [n_chunks * nku * 64]
    uint32_t *chunk_d = chunk_u + (size_t)t.n_chunks * nku * 64;          // [n_chunks * nkd * 64]
    const int tid = threadIdx.x, pass = blockIdx.y;
    int kind = 0;
    while (pass >= t.pass_end[kind]) ++kind;
    const int first = (pass - (kind > 0 ? t.pass_end[kind - 1] : 0)) * (kind == kHubNN || kind == kHubSite ? 8 : 16);
    if (kind == kHubHopU || kind == kHubFlip)
        for (int i = tid; i < t.n_chunks * nku * 64; i += kCorrBlock) chunk_u[i] = t.chunk_u[i];
    if (kind == kHubHopD || kind == kHubFlip)
        for (int i = tid; i < t.n_chunks * nkd * 64; i += kCorrBlock) chunk_d[i] = t.chunk_d[i];
    if (kind != kHubSite && tid < (kind == kHubNN ? 8 : 16)) pair[tid] = t.pair[first + tid];
    __syncthreads();
    double acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = 0.0;
    const int64_t dim = t.Nu * t.Nd, stride = (int64_t)gridDim.x * kCorrBlock;
    for (int64_t row = (int64_t)blockIdx.x * kCorrBlock + tid; row < dim; row += stride) {
        const int64_t ru = row / t.Nd, rd = row - ru * t.Nd;
        const uint32_t u = t.cfg_u[ru], d = t.cfg_d[rd];
        const d2 x = corr_load_x<REALX>(t.xg, t.xr, row);
        if (kind == kHubSite) {
            const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const uint32_t bu = (u >> ((first + g) & 31)) & 1u, bd = (d >> ((first + g) & 31)) & 1u;
                acc[g] += bu ? w : 0.0;
                acc[8 + g] += bd ? w : 0.0;
                acc[16 + g] += (bu & bd) ? w : 0.0;
            }
            acc[24] += w;
        } else if (kind == kHubNN) {
            const double w = fma(x.x, x.x, x.y * x.y);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const int i = (int)(pair[g] & 255u), j = (int)(pair[g] >> 8);
                const uint32_t ui = (u >> i) & 1u, uj = (u >> j) & 1u, di = (d >> i) & 1u, dj = (d >> j) & 1u;
                const bool real_pair = i != j;
                acc[g] += (real_pair && (ui & uj)) ? w : 0.0;
                acc[8 + g] += (real_pair && (di & dj)) ? w : 0.0;
                acc[16 + g] += (real_pair && (ui & dj)) ? w : 0.0;
                acc[24 + g] += (real_pair && (di & uj)) ? w : 0.0;
            }
        } else {
#pragma unroll
            for (int g0 = 0; g0 < 16; g0 += 8) {
                long long idx[8];
                double sg[8];                          // +-1, 0 without a hit: such a lane reads its own row and adds 0 (a hit mask
                                                       // here takes 175 VGPRs instead of 162 and the third wavefront per SIMD)
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const int i = (int)(pair[g0 + g] & 255u), j = (int)(pair[g0 + g] >> 8);       // i < j, or i == j == 0 (padding)
                    const uint32_t bi = 1u << i, bj = 1u << j;
                    long long q = row;
                    double sign = 0.0;
                    if (kind == kHubHopU) {
                        if (i != j && (u & bj) && !(u & bi)) {
                            sign = (hub_between(u, i, j) & 1) ? -1.0 : 1.0;
                            q = (long long)hub_rank(chunk_u, t.n_chunks, nku, u ^ bi ^ bj) * t.Nd + rd;
                        }
                    } else if (kind == kHubHopD) {
                        if (i != j && (d & bj) && !(d & bi)) {
                            sign = (hub_between(d, i, j) & 1) ? -1.0 : 1.0;
                            q = ru * t.Nd + (long long)hub_rank(chunk_d, t.n_chunks, nkd, d ^ bi ^ bj);
                        }
                    } else {
                        // c_{j,up}: j up occupied; c+_{j,dn}: j down empty; c_{i,dn}: i down occupied; c+_{i,up}: i up empty
                        if (i != j && (u & bj) && !(d & bj) && (d & bi) && !(u & bi)) {
                            const uint32_t u1 = u ^ bj, d1 = d | bj;
                            // occupied orbitals below each factor's orbital; the n_up - 1 up orbitals below both down factors cancel
                            const int par = __popc(u & (bj - 1u)) + __popc(d & (bj - 1u)) + __popc(d1 & (bi - 1u)) + __popc(u1 & (bi - 1u));
                            sign = (par & 1) ? -1.0 : 1.0;
                            q = (long long)hub_rank(chunk_u, t.n_chunks, nku, u1 | bi) * t.Nd +
                                (long long)hub_rank(chunk_d, t.n_chunks, nkd, d1 ^ bi);
                        }
                    }
                    idx[g] = q;
                    sg[g] = sign;
                }
                if (REALX) {
                    double xv[8];
#pragma unroll
                    for (int g = 0; g < 8; ++g) xv[g] = t.xr[idx[g]];
#pragma unroll
                    for (int g = 0; g < 8; ++g) acc[g0 + g] += sg[g] * (xv[g] * x.x);
                } else {
                    d2 xv[8];
#pragma unroll
                    for (int g = 0; g < 8; ++g) xv[g] = t.xg[idx[g]];
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        acc[g0 + g] += sg[g] * fma(xv[g].x, x.x, xv[g].y * x.y);
                        acc[16 + g0 + g] += sg[g] * (xv[g].x * x.y - xv[g].y * x.x);
                    }
                }
            }
        }
    }
    corr_block_partials<NA>(acc, red, t.partials);
}

// ------------------------------------------------------------------------------------------------------ host side --
}  // namespace

int corr_check_vectors(const char *who, const void *d_vec, const void *d_vec_re)
{
    if ((d_vec != nullptr) != (d_vec_re != nullptr)) return QBH_OK;
    set_error("%s: exactly one of d_vec and d_vec_re must be given", who);
    return QBH_EINVAL;
}

int corr_check_norm2(const char *who, const double *norm2)
{
    if (norm2 != nullptr) return QBH_OK;
    set_error("%s: norm2 is NULL", who);
    return QBH_EINVAL;
}

int corr_check_device()
{
    if (qbh_device_count() > 0) return QBH_OK;
    set_error("no HIP device visible");
    return QBH_ENODEVICE;
}

int corr_grid(int64_t dim, size_t lds, int rows_per_block)
{
    const int ncu = device_cu_count();
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, ((size_t)158 * 1024) / (lds + 2048)));
    const int64_t nblk = (dim + rows_per_block - 1) / rows_per_block;
    return (int)std::max<int64_t>(1, std::min<int64_t>(nblk, (int64_t)ncu * per_cu));
}

hipError_t corr_launch(const void *kernel, int gx, int n_pass, int block, size_t lds, hipStream_t s, const void *arg)
{
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    void *args[] = {const_cast<void *>(arg)};
    (void)hipLaunchKernel(kernel, dim3(gx, n_pass), dim3(block), args, lds, s);
    return hipGetLastError();
}

size_t corr_reduce_doubles(int gx, int n_pass, int na) { return ((size_t)gx + 1) * n_pass * na; }

int corr_reduce_launch_any(const char *who, const void *kernel, int gx, int n_pass, int na, int block, size_t lds, hipStream_t s,
                       const void *arg, double **partials, std::vector<void *> &pool, std::vector<double> &out)
{
    const int ncomp = n_pass * na;
    if (*partials == nullptr) {
        QBH_HIP_WHO(who, qbh::dev_alloc(partials, corr_reduce_doubles(gx, n_pass, na) * sizeof(double)));
        pool.push_back(*partials);
    }
    QBH_HIP_WHO(who, corr_launch(kernel, gx, n_pass, block, lds, s, arg));
    // second stage + download: out[ncomp] = sum over the gx workgroups, in the order of k_corr_reduce
    double *d_out = *partials + (size_t)gx * ncomp;
    QBH_TRY(launch_kernel(k_corr_reduce, (ncomp + 63) / 64, 64 * kCorrRedWaves, s, (const double *)*partials, gx, ncomp, d_out));
    out.resize((size_t)ncomp);
    QBH_HIP(hipMemcpyAsync(out.data(), d_out, (size_t)ncomp * sizeof(double), hipMemcpyDeviceToHost, s));
    QBH_HIP(hipStreamSynchronize(s));
    return QBH_OK;
}

namespace {

size_t corr_spin_lds(int n_sites, int n_dn)
{
    const size_t nk = (size_t)n_dn + 1, n_chunks = (size_t)(n_sites + 5) / 6, word = n_sites <= 32 ? 4 : 8;
    return ((size_t)(n_sites + 1) * nk + n_chunks * nk * 64) * word + (size_t)kCorrBlock * (32 + word);      // tables + one tile of patterns
}

// binom[p * (n + 1) + k] = C(p, k), p = 0 .. n_sites, k = 0 .. n
std::vector<uint64_t> corr_binom_table(int n_sites, int n)
{
    const int nk = n + 1;
    std::vector<uint64_t> binom((size_t)(n_sites + 1) * nk);
    for (int p = 0; p <= n_sites; ++p)
        for (int k = 0; k < nk; ++k) binom[(size_t)p * nk + k] = binom_u64(p, k);
    return binom;
}

// chunk[c][j][bits]: the t-th set bit of `bits` (site 6c + b) is the (j + t + 1)-th particle of the pattern (as qbh_mf_heisenberg);
// a combination that no pattern of n particles on n_sites sites holds is 0.  Looked up in `binom` (corr_binom_table(n_sites, n)).
template <typename W>
std::vector<W> corr_chunk_table(int n_sites, int n, const std::vector<uint64_t> &binom)
{
    const int nk = n + 1, n_chunks = (n_sites + 5) / 6;
    std::vector<W> chunk((size_t)n_chunks * nk * 64, (W)0);
    for (int c = 0; c < n_chunks; ++c)
        for (int j = 0; j < nk; ++j)
            for (int bits = 0; bits < 64; ++bits) {
                uint64_t r = 0;
                int k = j;
                bool ok = true;
                for (int b = 0; b < 6; ++b)
                    if ((bits >> b) & 1) {
                        const int site = 6 * c + b;
                        ++k;
                        if (site >= n_sites || k > n) {
                            ok = false;
                            break;
                        }
                        r += binom[(size_t)site * nk + k];
                    }
                chunk[((size_t)c * nk + j) * 64 + bits] = ok ? (W)r : (W)0;
            }
    return chunk;
}

// the spin kernel's tables in one buffer (one allocation, one copy): binomials | chunk table, in words of W, then the 64-bit masks
template <typename W>
void corr_spin_tables(int n_sites, int n_dn, const std::vector<uint64_t> &mask, std::vector<uint64_t> &buf, size_t *chunk_at,
                      size_t *mask_at)
{
    const std::vector<uint64_t> binom = corr_binom_table(n_sites, n_dn);
    const std::vector<W> chunk = corr_chunk_table<W>(n_sites, n_dn, binom);
    const size_t words = (binom.size() + chunk.size()) * sizeof(W) / 8 + 1;
    buf.assign(words + mask.size(), 0ULL);
    W *w = reinterpret_cast<W *>(buf.data());
    for (size_t i = 0; i < binom.size(); ++i) w[i] = (W)binom[i];
    std::copy(chunk.begin(), chunk.end(), w + binom.size());
    std::copy(mask.begin(), mask.end(), buf.begin() + words);
    *chunk_at = binom.size() * sizeof(W);
    *mask_at = words * 8;
}

size_t corr_hub_lds(int n_sites, int n_up, int n_dn)
{
    const size_t n_chunks = (size_t)(n_sites + 5) / 6;
    return n_chunks * 64 * ((size_t)n_up + 1 + (size_t)n_dn + 1) * 4;
}

enum { kSpinPair = 0, kSpinSite = 1 };

template <typename W, int NC>
void (*spin_kernel(bool rx))(CorrSpin)
{
    return rx ? k_corr_spin<true, W, NC> : k_corr_spin<false, W, NC>;
}

int corr_spin_run(const char *who, int n_sites, int n_dn, const d2 *xg, const double *xr, bool want_zz, bool want_pm,
                  std::vector<double> &comp, CorrPasses &sp, hipStream_t s, std::vector<void *> &pool)
{
    const int n_chunks = (n_sites + 5) / 6, G = kSpinGroup;
    const int n_pairs = (want_zz || want_pm) ? n_sites * (n_sites - 1) / 2 : 0;
    const int NA = xr ? spin_acc<true>() : spin_acc<false>();
    sp.add(kSpinPair, n_pairs, G);
    sp.add(kSpinSite, n_sites, G);
    std::vector<uint64_t> mask((size_t)sp.count[kSpinPair] * G, 0ULL);  // padding: mask 0, which no row matches
    if (n_pairs > 0) {
        size_t q = 0;
        for (int i = 0; i < n_sites; ++i)
            for (int j = i + 1; j < n_sites; ++j) mask[q++] = (1ULL << i) | (1ULL << j);
    }
    const bool w32 = n_sites <= 32;                                     // patterns, ranks and table entries in 32 bits
    CorrSpin t{};
    t.n_sites = n_sites;
    t.n_dn = n_dn;
    t.n_chunks = n_chunks;
    t.n_pair_pass = sp.count[kSpinPair];
    t.want_pm = want_pm ? 1 : 0;
    t.want_zz = want_zz ? 1 : 0;
    t.dim = (int64_t)binom_u64(n_sites, n_dn);
    t.xg = xg;
    t.xr = xr;
    std::vector<uint64_t> tables;
    size_t chunk_at = 0, mask_at = 0;                                   // byte offsets in `tables`
    if (w32) corr_spin_tables<uint32_t>(n_sites, n_dn, mask, tables, &chunk_at, &mask_at);
    else     corr_spin_tables<uint64_t>(n_sites, n_dn, mask, tables, &chunk_at, &mask_at);
    const size_t lds = corr_spin_lds(n_sites, n_dn);
    const int gx = corr_grid(t.dim, lds, kCorrBlock * (w32 ? spin_rows<uint32_t>() : spin_rows<uint64_t>()));
    // this call alone brings its own allocation: the partials and their sums | the tables, so that they cost one allocation and
    // one copy
    const size_t n_red = corr_reduce_doubles(gx, sp.n_pass, NA);
    QBH_HIP_WHO(who, qbh::dev_alloc(&t.partials, (n_red + tables.size()) * 8));
    pool.push_back(t.partials);
    const char *d_tables = reinterpret_cast<const char *>(t.partials + n_red);
    QBH_HIP_WHO(who, hipMemcpy(t.partials + n_red, tables.data(), tables.size() * 8, hipMemcpyHostToDevice));
    t.binom = d_tables;
    t.chunk = d_tables + chunk_at;
    t.mask = reinterpret_cast<const uint64_t *>(d_tables + mask_at);
    void (*kernel)(CorrSpin);
    if (w32) {                                              // 19 .. 32 sites: the re-ranking loop unrolled
        switch (n_chunks) {
        case 4: kernel = spin_kernel<uint32_t, 4>(xr != nullptr); break;
        case 5: kernel = spin_kernel<uint32_t, 5>(xr != nullptr); break;
        case 6: kernel = spin_kernel<uint32_t, 6>(xr != nullptr); break;
        default: kernel = spin_kernel<uint32_t, 0>(xr != nullptr); break;
        }
    } else {                                                // 33 .. 36 sites unrolled
        kernel = n_chunks == 6 ? spin_kernel<uint64_t, 6>(xr != nullptr) : spin_kernel<uint64_t, 0>(xr != nullptr);
    }
    return corr_reduce_launch(who, kernel, gx, sp.n_pass, NA, kCorrBlock, lds, s, t, t.partials, pool, comp);
}

int corr_hub_run(const char *who, int n_sites, int n_up, int n_dn, const d2 *xg, const double *xr, bool want_nn, bool want_hop,
                 bool want_flip, std::vector<double> &comp, CorrPasses &hp, hipStream_t s, std::vector<void *> &pool)
{
    const int n_chunks = (n_sites + 5) / 6;
    std::vector<uint32_t> cu, cd;
    enumerate_configs(n_sites, n_up, cu);
    enumerate_configs(n_sites, n_dn, cd);
    auto chunk_table = [&](int n) { return corr_chunk_table<uint32_t>(n_sites, n, corr_binom_table(n_sites, n)); };
    const int n_pairs = n_sites * (n_sites - 1) / 2;
    std::vector<uint32_t> pair((size_t)((n_pairs + 15) / 16) * 16 + 16, 0u);
    {
        size_t q = 0;
        for (int i = 0; i < n_sites; ++i)
            for (int j = i + 1; j < n_sites; ++j) pair[q++] = (uint32_t)i | ((uint32_t)j << 8);
    }
    hp.add(kHubNN, want_nn ? n_pairs : 0, 8);
    hp.add(kHubHopU, want_hop ? n_pairs : 0, 16);
    hp.add(kHubHopD, want_hop ? n_pairs : 0, 16);
    hp.add(kHubFlip, want_flip ? n_pairs : 0, 16);
    hp.add(kHubSite, n_sites, 8);
    CorrHub t{};
    for (int k = 0; k < 5; ++k) t.pass_end[k] = hp.first[k] + hp.count[k];
    t.n_sites = n_sites;
    t.n_up = n_up;
    t.n_dn = n_dn;
    t.n_chunks = n_chunks;
    t.Nu = (int64_t)cu.size();
    t.Nd = (int64_t)cd.size();
    t.xg = xg;
    t.xr = xr;
    uint32_t *d_cu = nullptr, *d_cd = nullptr, *d_chu = nullptr, *d_chd = nullptr, *d_pair = nullptr;
    QBH_TRY(upload(cu, &d_cu, pool));
    QBH_TRY(upload(cd, &d_cd, pool));
    QBH_TRY(upload(chunk_table(n_up), &d_chu, pool));
    QBH_TRY(upload(chunk_table(n_dn), &d_chd, pool));
    QBH_TRY(upload(pair, &d_pair, pool));
    t.cfg_u = d_cu;
    t.cfg_d = d_cd;
    t.chunk_u = d_chu;
    t.chunk_d = d_chd;
    t.pair = d_pair;
    const size_t lds = corr_hub_lds(n_sites, n_up, n_dn);
    void (*kernel)(CorrHub) = xr ? k_corr_hubbard<true> : k_corr_hubbard<false>;
    return corr_reduce_launch(who, kernel, corr_grid(t.Nu * t.Nd, lds, kCorrBlock), hp.n_pass, kHubAcc, kCorrBlock, lds, s, t,
                              nullptr, pool, comp);
}

}  // namespace
}  // namespace qbh

extern "C" int qbh_corr_spin_dev(int n_sites, int n_dn, const qbh_z *d_vec, const double *d_vec_re, double *norm2, double *sz, double *zz,
                                 qbh_z *pm, void *stream)
{
    using namespace qbh;
    static const char *who = "qbh_corr_spin_dev";
    if (n_sites <= 0 || n_sites > 62) {
        set_error("%s: n_sites = %d (1 .. 62 allowed)", who, n_sites);
        return QBH_EINVAL;
    }
    if (n_dn < 0 || n_dn > n_sites || n_dn > 33) {
        set_error("%s: n_dn = %d (0 .. min(n_sites, 33) allowed)", who, n_dn);
        return QBH_EINVAL;
    }
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    if (binom_u64(n_sites, n_dn) >= (1ULL << 62)) {
        set_error("%s: a sector of 2^62 rows or more", who);
        return QBH_EUNSUPP;
    }
    const size_t lds = corr_spin_lds(n_sites, n_dn);
    if (lds > kCorrLdsCap) {
        set_error("%s: tables (%zu bytes) do not fit LDS", who, lds);
        return QBH_EUNSUPP;
    }
    QBH_TRY(corr_check_device());
    const int N = n_sites, G = kSpinGroup;
    std::vector<void *> pool;
    std::vector<double> comp;
    CorrPasses sp;
    const int rc = corr_spin_run(who, N, n_dn, reinterpret_cast<const d2 *>(d_vec), d_vec_re, zz != nullptr, pm != nullptr, comp, sp,
                                 (hipStream_t)stream, pool);
    free_pool(pool);
    if (rc != QBH_OK) return rc;
    const bool rx = d_vec_re != nullptr;
    const int NA = rx ? spin_acc<true>() : spin_acc<false>();
    auto site_sum = [&](int site) { return sp.at(comp, kSpinSite, site, G, 0, NA); };
    const double n2 = sp.at(comp, kSpinSite, 0, G, 1, NA);
    if (norm2) *norm2 = n2;
    if (sz)
        for (int i = 0; i < N; ++i) sz[i] = site_sum(i);
    int q = 0;
    for (int i = 0; i < N; ++i) {
        if (zz) zz[(size_t)i * N + i] = 0.25 * n2;
        if (pm) pm[(size_t)i * N + i] = qbh_z{0.5 * n2 + site_sum(i), 0.0};
        for (int j = i + 1; j < N; ++j, ++q) {               // the pair's accumulators are present when zz or pm is asked for
            if (zz) zz[(size_t)i * N + j] = zz[(size_t)j * N + i] = corr_zz_pair(n2, sp.at(comp, kSpinPair, q, G, 0, NA));
            if (pm) corr_put_herm(pm, N, i, j, sp.at(comp, kSpinPair, q, G, 1, NA), rx ? 0.0 : sp.at(comp, kSpinPair, q, G, 2, NA));
        }
    }
    return QBH_OK;
}

extern "C" int qbh_corr_hubbard_dev(int n_sites, int n_up, int n_dn, const qbh_z *d_vec, const double *d_vec_re, double *norm2, double *dens,
                                    double *nn, qbh_z *hop, qbh_z *flip, void *stream)
{
    using namespace qbh;
    static const char *who = "qbh_corr_hubbard_dev";
    if (n_sites <= 0 || n_sites > 31) {
        set_error("%s: n_sites = %d (1 .. 31 allowed)", who, n_sites);
        return QBH_EINVAL;
    }
    if (n_up < 0 || n_dn < 0 || n_up > n_sites || n_dn > n_sites) {
        set_error("%s: (n_up, n_dn) = (%d, %d) (0 .. n_sites allowed)", who, n_up, n_dn);
        return QBH_EINVAL;
    }
    QBH_TRY(corr_check_vectors(who, d_vec, d_vec_re));
    const size_t lds = corr_hub_lds(n_sites, n_up, n_dn);
    if (lds > kCorrLdsCap) {
        set_error("%s: tables (%zu bytes) do not fit LDS", who, lds);
        return QBH_EUNSUPP;
    }
    QBH_TRY(corr_check_device());
    const int N = n_sites;
    const size_t NN = (size_t)N * N;
    std::vector<void *> pool;
    std::vector<double> comp;
    CorrPasses hp;
    const int rc = corr_hub_run(who, N, n_up, n_dn, reinterpret_cast<const d2 *>(d_vec), d_vec_re, nn != nullptr, hop != nullptr,
                                flip != nullptr, comp, hp, (hipStream_t)stream, pool);
    free_pool(pool);
    if (rc != QBH_OK) return rc;
    const bool rx = d_vec_re != nullptr;
    auto at = [&](int kind, int item, int per_pass, int slot) { return hp.at(comp, kind, item, per_pass, slot, kHubAcc); };
    if (norm2) *norm2 = at(kHubSite, 0, 8, 3);
    int q = 0;
    for (int i = 0; i < N; ++i) {
        const double nu = at(kHubSite, i, 8, 0), nd = at(kHubSite, i, 8, 1), docc = at(kHubSite, i, 8, 2);
        if (dens) {
            dens[i] = nu;
            dens[N + i] = nd;
        }
        if (nn) corr_put_nn_diag(nn, N, i, nu, docc, nd);
        corr_put_onsite_diag(hop, flip, N, i, nu, nd, docc);
        for (int j = i + 1; j < N; ++j, ++q) {
            if (nn) corr_put_nn_pair(nn, N, i, j, at(kHubNN, q, 8, 0), at(kHubNN, q, 8, 2), at(kHubNN, q, 8, 3), at(kHubNN, q, 8, 1));
            auto herm = [&](qbh_z *out, int kind) { corr_put_herm(out, N, i, j, at(kind, q, 16, 0), rx ? 0.0 : at(kind, q, 16, 1)); };
            if (hop) {
                herm(hop, kHubHopU);
                herm(hop + NN, kHubHopD);
            }
            if (flip) herm(flip, kHubFlip);
        }
    }
    return QBH_OK;
}
