// qbh_mf.hip -- matrix-free Hubbard and Heisenberg operators: kernels and launchers.
#include <algorithm>

#include "qbh_internal.hpp"
#include "qbh_mf_row.hpp"

namespace qbh {

// -------------------------------------------- matrix-free two-species operator --
// y <- alpha*(H x) + beta*y + gamma*x_local with H = T_up (x) 1 + 1 (x) T_dn + U*D applied from the hop tables
// (ELL layout, coalesced).  One lane per row (u, d); 256 consecutive rows per workgroup pass.  The up-species
// hops of consecutive rows read consecutive x elements (full-line coalesced), the down-species hops stay inside
// the 16*N_dn-byte window of the row's own u.  Same fused epilogue and partial sums as the CSR kernels.
template <bool REALX>
__global__ __launch_bounds__(kBlock) void k_mf_hubbard(MfArgs a)
{
    __shared__ double red[12];
    __shared__ double amp_s[16];
    double acc[3] = {0.0, 0.0, 0.0};
    const MfHubbard &t = a.t;
    if (threadIdx.x < 16) amp_s[threadIdx.x] = t.amp[threadIdx.x];
    __syncthreads();
    const int64_t n_chunks = (a.v.nrows + kBlock - 1) / kBlock;
    const bool need_x = a.v.gamma != 0.0 || a.v.partials != nullptr;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t lrow = chunk * kBlock + threadIdx.x;
        if (lrow < a.v.nrows) {
            const int64_t grow = a.v.row_begin + lrow;
            const int64_t u = grow / t.Nd, d = grow - u * t.Nd;
            d2 sum = {0.0, 0.0};
            // diagonal: U * number of doubly occupied sites
            const double diag = t.U * (double)__popc(t.cfg_u[u] & t.cfg_d[d]);
            if (REALX) sum.x = diag * a.v.xr[grow];
            else       sum = diag * a.v.xg[grow];
            // The tables are padded to a multiple of 8 hops with (target = the configuration itself, amplitude 0),
            // so each group of 8 table reads and 8 gathers is issued without a branch (8 loads in flight per lane).
            // up-species hops: x[u' * Nd + d], consecutive lanes -> consecutive addresses
            for (int k0 = 0; k0 < t.wu; k0 += 8) {
                int64_t c[8];
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    c[j] = (int64_t)t.tgt_u[(size_t)(k0 + j) * t.Nu + u] * t.Nd + d;
                    v[j] = amp_s[t.val_u[(size_t)(k0 + j) * t.Nu + u]];
                }
                if (REALX) {
                    double xr[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) xr[j] = a.v.xr[c[j]];
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum.x += v[j] * xr[j];
                } else {
                    d2 xv[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[j] = a.v.xg[c[j]];
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum += v[j] * xv[j];
                }
            }
            // down-species hops: x[u * Nd + d'] inside the row's own window
            const int64_t base = u * t.Nd;
            for (int k0 = 0; k0 < t.wd; k0 += 8) {
                int64_t c[8];
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    c[j] = base + t.tgt_d[(size_t)(k0 + j) * t.Nd + d];
                    v[j] = amp_s[t.val_d[(size_t)(k0 + j) * t.Nd + d]];
                }
                if (REALX) {
                    double xr[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) xr[j] = a.v.xr[c[j]];
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum.x += v[j] * xr[j];
                } else {
                    d2 xv[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[j] = a.v.xg[c[j]];
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum += v[j] * xv[j];
                }
            }
            d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
            if (a.v.y_re != nullptr) {                  // all-real operation (REALX): y and x_local as doubles
                if (a.v.beta != 0.0) yo.x = a.v.y_re[lrow];
                if (need_x) xi.x = a.v.xr[grow];
            } else {
                if (a.v.beta != 0.0) yo = a.v.y[lrow];
                if (need_x) xi = a.v.xl[lrow];
            }
            const d2 yn = a.v.alpha * sum + a.v.beta * yo + a.v.gamma * xi;
            if (a.v.y_re != nullptr) a.v.y_re[lrow] = yn.x;
            else                     a.v.y[lrow] = yn;
            acc[0] += xi.x * yn.x + xi.y * yn.y;
            acc[1] += xi.x * yn.y - xi.y * yn.x;
            acc[2] += yn.x * yn.x + yn.y * yn.y;
        }
    }
    if (a.v.partials != nullptr) {
        block_sum<3>(acc, red);
        if (threadIdx.x == 0) {
            a.v.partials[(size_t)blockIdx.x * 3 + 0] = acc[0];
            a.v.partials[(size_t)blockIdx.x * 3 + 1] = acc[1];
            a.v.partials[(size_t)blockIdx.x * 3 + 2] = acc[2];
        }
    }
}

// Row-staged variant for real vectors: X is the N_up x N_dn matrix x[u * N_dn + d].  One 1024-lane workgroup owns one
// up-configuration u at a time and keeps the whole row X[u][:] (8 * N_dn bytes) in LDS, so
//   * the down-species hops  Y[u][d] += sum_k a_k X[u][d'_k]  gather from LDS instead of through the texture path
//     (scattered 8-byte gathers are what bounds the lane-per-row kernel: one cache line per lane per cycle),
//   * the up-species hops  Y[u][:] += sum_j a_j X[u'_j][:]  are row AXPYs: fully coalesced 512-byte wave loads, the
//     ~17 neighbour rows shared through L2 / Infinity Cache with the workgroups working on nearby u,
//   * x_local of the fused epilogue comes from the staged row for free.
// The down-hop table is read as packed {target:24 | amplitude code:8} words, four hops per 16-byte load.
constexpr int kMfRowBlock = 1024;
constexpr int kMfMaxUp = 64;

// WINDOWED = false: the whole row X[u][:] is staged (8 * N_dn <= LDS).  WINDOWED = true (longer rows): a work item is
// (u, chunk of `chunk` consecutive d); LDS holds the window of `wcap` elements of the row centred on the chunk.  Hops
// in the colex order mostly move a configuration's rank a little (4x5 lattice, 6 particles: 84 % of the hops stay
// within +-8192), so most down-hop gathers still come from LDS; the rest read the row through L2.
template <bool WINDOWED>
__global__ __launch_bounds__(kMfRowBlock) void k_mf_hubbard_row(MfArgs a, int chunk, int wcap)
{
    extern __shared__ double xs[];                 // [Nd] or [wcap]
    __shared__ double amp_s[16];
    __shared__ double dd_s[256];                   // a.dcode: the value dictionary's real parts (the diagonal is dd_s[dcode[row]])
    __shared__ long long up_off[kMfMaxUp + 8];
    __shared__ double up_amp[kMfMaxUp + 8];
    __shared__ int up_n;
    __shared__ double red[3 * (kMfRowBlock / 64)];
    const MfHubbard &t = a.t;
    const int tid = threadIdx.x;
    const int64_t Nd = t.Nd;
    double acc[3] = {0.0, 0.0, 0.0};
    if (tid < 16) amp_s[tid] = t.amp[tid];
    if (a.dcode != nullptr && tid < 256) dd_s[tid] = a.ddict[tid];
    const int64_t u_first = a.v.row_begin / Nd, u_last = (a.v.row_begin + a.v.nrows - 1) / Nd;
    const bool need_y = a.v.beta != 0.0;
    const uint4 *pk = reinterpret_cast<const uint4 *>(t.pk_d);
    const int nk4 = t.wd / 4;
    const int64_t n_chunks = WINDOWED ? (Nd + chunk - 1) / chunk : 1;
    const int64_t n_items = (u_last - u_first + 1) * n_chunks;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t u = u_first + item / n_chunks;
        const int64_t c_lo = WINDOWED ? (item % n_chunks) * chunk : 0;
        const int64_t c_hi = WINDOWED ? (c_lo + chunk < Nd ? c_lo + chunk : Nd) : Nd;
        // window [w_lo, w_hi) of the row kept in LDS
        int64_t w_lo = 0, w_hi = Nd;
        if (WINDOWED) {
            w_lo = c_lo - (wcap - (c_hi - c_lo)) / 2;
            if (w_lo < 0) w_lo = 0;
            w_hi = w_lo + wcap;
            if (w_hi > Nd) {
                w_hi = Nd;
                w_lo = w_hi - wcap > 0 ? w_hi - wcap : 0;
            }
        }
        const double *xrow = a.v.xr + u * Nd;
        for (int64_t d = w_lo + tid; d < w_hi; d += kMfRowBlock) xs[d - w_lo] = xrow[d];
        if (tid < 64) {
            // the up-neighbours of u with a non-zero amplitude, compacted by one wavefront and padded to a group of 8
            // with (u itself, amplitude 0) so that the row loop below is branch-free
            const bool in = tid < t.wu;
            const int code = in ? t.val_u[(size_t)tid * t.Nu + u] : 0;
            const bool live = in && code != 0;
            const unsigned long long mask = __ballot(live);
            const int pos = __popcll(mask & ((1ULL << tid) - 1ULL));
            const int n = __popcll(mask);
            if (live) {
                up_off[pos] = (long long)t.tgt_u[(size_t)tid * t.Nu + u] * Nd;
                up_amp[pos] = amp_s[code];
            }
            const int npad = (n + 7) & ~7;
            if (tid >= n && tid < npad) {
                up_off[tid] = (long long)u * Nd;
                up_amp[tid] = 0.0;
            }
            if (tid == 0) up_n = npad;
        }
        __syncthreads();
        int64_t d_lo = a.v.row_begin > u * Nd ? a.v.row_begin - u * Nd : 0;
        int64_t d_hi = (a.v.row_begin + a.v.nrows - u * Nd) < Nd ? (a.v.row_begin + a.v.nrows - u * Nd) : Nd;
        if (d_lo < c_lo) d_lo = c_lo;
        if (d_hi > c_hi) d_hi = c_hi;
        const uint32_t cu = a.dcode != nullptr ? 0u : t.cfg_u[u];
        const int nu = up_n;
        for (int64_t d = d_lo + tid; d < d_hi; d += kMfRowBlock) {
            const double xd = xs[d - w_lo];
            double sum = (a.dcode != nullptr ? dd_s[a.dcode[u * Nd + d]] : t.U * (double)__popc(cu & t.cfg_d[d])) * xd;
            // up-species hops first (global, longest latency): 8 coalesced row loads in flight
            for (int j0 = 0; j0 < nu; j0 += 8) {
                double xv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] = a.v.xr[up_off[j0 + j] + d];
#pragma unroll
                for (int j = 0; j < 8; ++j) sum += up_amp[j0 + j] * xv[j];
            }
            // down-species hops from the staged row
            for (int k4 = 0; k4 < nk4; k4 += 2) {
                const uint4 e0 = pk[(size_t)k4 * Nd + d], e1 = pk[(size_t)(k4 + 1) * Nd + d];
                const uint32_t w[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
                double xv[8];
                if (WINDOWED) {
                    bool miss[8];
                    bool any_miss = false;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int64_t tg = (int64_t)(w[j] & 0xFFFFFFu);
                        miss[j] = tg < w_lo || tg >= w_hi;
                        any_miss = any_miss || miss[j];
                        xv[j] = xs[miss[j] ? 0 : tg - w_lo];
                    }
                    if (any_miss) {
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (miss[j]) xv[j] = xrow[w[j] & 0xFFFFFFu];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[j] = xs[w[j] & 0xFFFFFFu];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) sum += amp_s[w[j] >> 24] * xv[j];
            }
            const int64_t lrow = u * Nd + d - a.v.row_begin;
            d2 yo = {0.0, 0.0};
            if (need_y) {
                if (a.v.y_re != nullptr) yo.x = a.v.y_re[lrow];
                else                     yo = a.v.y[lrow];
            }
            d2 yn;
            yn.x = a.v.alpha * sum + a.v.beta * yo.x + a.v.gamma * xd;
            yn.y = a.v.beta * yo.y;
            if (a.v.y_re != nullptr) a.v.y_re[lrow] = yn.x;
            else                     a.v.y[lrow] = yn;
            acc[0] += xd * yn.x;
            acc[1] += xd * yn.y;
            acc[2] += yn.x * yn.x + yn.y * yn.y;
        }
        __syncthreads();                           // the row and the neighbour list are rewritten next
    }
    mf_block_partials<kMfRowBlock>(acc, red, a.v.partials);
}

// -------------------------------------------- matrix-free Heisenberg operator --
// One lane per row.  LDS holds the binomials (unranking), the chunk tables (re-ranking a flipped pattern costs one
// lookup per 6 bits) and the bond list; the only global traffic is the x gather, y and the epilogue operands.
constexpr int kMfHeisBlock = 512;

// NCH > 0: the number of chunks as a compile-time constant (re-ranking loop fully unrolled, 32-bit index arithmetic)
template <bool REALX, int NCH>
__global__ __launch_bounds__(kMfHeisBlock) void k_mf_heis(MfHeis t, MfVec a)
{
    extern __shared__ unsigned long long lds_u64[];
    __shared__ double red[3 * (kMfHeisBlock / 64)];
    const int nk = t.n_dn + 1;
    unsigned long long *binom = lds_u64;                                  // [(n_sites+1) * nk]
    unsigned long long *chunk = binom + (size_t)(t.n_sites + 1) * nk;     // [n_chunks * nk * 64]
    unsigned long long *mask = chunk + (size_t)t.n_chunks * nk * 64;      // [n_bonds]
    double *offd = reinterpret_cast<double *>(mask + t.n_bonds);          // [n_bonds]
    double *diag = offd + t.n_bonds;                                      // [n_bonds]
    const int tid = threadIdx.x;
    for (int i = tid; i < (t.n_sites + 1) * nk; i += kMfHeisBlock) binom[i] = t.binom[i];
    for (int i = tid; i < t.n_chunks * nk * 64; i += kMfHeisBlock) chunk[i] = t.chunk[i];
    for (int i = tid; i < t.n_bonds; i += kMfHeisBlock) {
        mask[i] = t.mask[i];
        offd[i] = t.offd[i];
        diag[i] = t.diag[i];
    }
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};
    const bool uniform = t.uniform != 0;
    const double offd0 = t.offd0, diag0 = t.diag0;
    const int64_t stride = (int64_t)gridDim.x * kMfHeisBlock;
    for (int64_t lrow = (int64_t)blockIdx.x * kMfHeisBlock + tid; lrow < a.nrows; lrow += stride) {
        const int64_t grow = a.row_begin + lrow;
        // unrank (colexicographic): largest p with C(p, k) <= r, for k = n_dn .. 1
        unsigned long long s = 0, r = (unsigned long long)grow;
        int p = t.n_sites - 1;
        for (int k = t.n_dn; k >= 1; --k) {
            while (binom[p * nk + k] > r) --p;
            s |= 1ULL << p;
            r -= binom[p * nk + k];
            --p;
        }
        // (a per-lane walk over only the flipping bonds was measured: 7 % faster at 39 % flipping bonds, 9 % slower at
        // Sz = 0 where half of them flip -- the uniform loop stays)
        double dg = 0.0;
        int ndiff = 0;
        d2 sum = {0.0, 0.0};
        for (int b0 = 0; b0 < t.n_bonds; b0 += 8) {
            long long idx[8];
            double amp[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned long long m = mask[b0 + j];
                const bool differ = __popcll(s & m) == 1;
                if (uniform) {
                    ndiff += differ ? 1 : 0;
                    amp[j] = differ ? offd0 : 0.0;
                } else {
                    dg += differ ? -diag[b0 + j] : diag[b0 + j];
                    amp[j] = differ ? offd[b0 + j] : 0.0;
                }
                long long q = grow;
                if (differ) {
                    const unsigned long long f = s ^ m;
                    unsigned long long rk = 0;
                    if (NCH > 0) {
                        const uint32_t flo = (uint32_t)f, fhi = (uint32_t)(f >> 30);      // chunks 0-4 | chunks 5-9
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
                            const int bits = (int)((f >> (6 * c)) & 63ULL);
                            rk += chunk[((size_t)c * nk + below) * 64 + bits];
                            below += __popc(bits);
                        }
                    }
                    q = (long long)rk;
                }
                idx[j] = q;
            }
            if (REALX) {
                double xv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] = a.xr[idx[j]];
#pragma unroll
                for (int j = 0; j < 8; ++j) sum.x += amp[j] * xv[j];
            } else {
                d2 xv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] = a.xg[idx[j]];
#pragma unroll
                for (int j = 0; j < 8; ++j) sum += amp[j] * xv[j];
            }
        }
        d2 yo, xi;
        mf_row_load<REALX>(a, lrow, grow, yo, xi);
        if (uniform) dg = diag0 * (double)(t.n_real - 2 * ndiff);
        mf_row_finish(a, lrow, sum, dg, xi, yo, acc);      // diagonal: sum_b +-J_b/4
    }
    mf_block_partials<kMfHeisBlock>(acc, red, a.partials);
}

int device_cu_count()
{
    static int ncu = 0;
    if (ncu == 0) {
        hipDeviceProp_t prop;
        int dev = 0;
        ncu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                  ? prop.multiProcessorCount : 256;
    }
    return ncu;
}

int launch_mf_heis(const MfHeis &t, const MfVec &a, hipStream_t s, int *nparts_out)
{
    const int ncu = device_cu_count();
    const size_t nk = (size_t)t.n_dn + 1;
    const size_t lds = ((size_t)(t.n_sites + 1) * nk + (size_t)t.n_chunks * nk * 64 + (size_t)t.n_bonds) * 8 + (size_t)t.n_bonds * 16;
    if (lds > (size_t)150 * 1024) {
        set_error("qbh_mf_heisenberg: tables (%zu bytes) do not fit LDS", lds);
        return QBH_EUNSUPP;
    }
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, ((size_t)158 * 1024) / (lds + 1024)));
    const int64_t nblk = (a.nrows + kMfHeisBlock - 1) / kMfHeisBlock;
    const int g = (int)std::min<int64_t>(nblk, (int64_t)ncu * per_cu);
#define QBH_HEIS_LAUNCH(RX, NC)                                                                                                    \
    do {                                                                                                                          \
        QBH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mf_heis<RX, NC>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                    (int)lds));                                                                                   \
        hipLaunchKernelGGL((k_mf_heis<RX, NC>), dim3(g), dim3(kMfHeisBlock), lds, s, t, a);                                        \
    } while (0)
    const bool rx = a.xr != nullptr;
    switch (t.n_chunks) {                                   // 24..36 sites get the unrolled forms
    case 4: if (rx) QBH_HEIS_LAUNCH(true, 4); else QBH_HEIS_LAUNCH(false, 4); break;
    case 5: if (rx) QBH_HEIS_LAUNCH(true, 5); else QBH_HEIS_LAUNCH(false, 5); break;
    case 6: if (rx) QBH_HEIS_LAUNCH(true, 6); else QBH_HEIS_LAUNCH(false, 6); break;
    default: if (rx) QBH_HEIS_LAUNCH(true, 0); else QBH_HEIS_LAUNCH(false, 0); break;
    }
#undef QBH_HEIS_LAUNCH
    QBH_HIP(hipGetLastError());
    if (nparts_out) *nparts_out = g;
    return QBH_OK;
}

// true when a row-staged kernel applies: real vectors, the neighbour list fits one wavefront
bool mf_row_kernel_ok(const MfArgs &a)
{
    if (a.v.xr == nullptr || a.t.pk_d == nullptr) return false;
    if (debug_sw().mf_row == 0) return false;
    return a.t.Nd >= 256 && a.t.Nd < (1 << 24) && a.t.wu <= kMfMaxUp && (a.t.wd % 8) == 0;
}

// *nparts_out = number of partial-sum triples written (workgroups launched)
int launch_mf_hubbard(const MfArgs &a, int grid, hipStream_t s, int *nparts_out)
{
    if (mf_row_kernel_ok(a)) {
        const int ncu = device_cu_count();
        const size_t lds_cap = (size_t)150 * 1024;
        const bool windowed = (size_t)a.t.Nd * sizeof(double) > lds_cap;
        const int64_t n_u = (a.v.row_begin + a.v.nrows - 1) / a.t.Nd - a.v.row_begin / a.t.Nd + 1;
        if (!windowed) {
            const size_t lds = (size_t)a.t.Nd * sizeof(double);
            QBH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mf_hubbard_row<false>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            // one workgroup per CU when the row takes most of the LDS, more when several rows fit
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, lds_cap / (lds + 2048)));
            const int g = (int)std::min<int64_t>(n_u, (int64_t)ncu * per_cu);
            hipLaunchKernelGGL(k_mf_hubbard_row<false>, dim3(g), dim3(kMfRowBlock), lds, s, a, 0, 0);
            QBH_HIP(hipGetLastError());
            if (nparts_out) *nparts_out = g;
            return QBH_OK;
        }
        int chunk = 8192, wcap = 18432;                // 144 KB window around an 8192-element chunk (measured: 2048..8192 within 5 %; bound by the up-row reads)
        if (debug_sw().mf_chunk) chunk = std::max(1024, debug_sw().mf_chunk);
        if (debug_sw().mf_window) wcap = std::max(chunk, std::min(18432, debug_sw().mf_window));
        const size_t lds = (size_t)wcap * sizeof(double);
        QBH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mf_hubbard_row<true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const int64_t n_items = n_u * ((a.t.Nd + chunk - 1) / chunk);
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, lds_cap / (lds + 2048)));
        const int g = (int)std::min<int64_t>(n_items, (int64_t)ncu * per_cu);
        hipLaunchKernelGGL(k_mf_hubbard_row<true>, dim3(g), dim3(kMfRowBlock), lds, s, a, chunk, wcap);
        QBH_HIP(hipGetLastError());
        if (nparts_out) *nparts_out = g;
        return QBH_OK;
    }
    if (a.v.xr != nullptr) hipLaunchKernelGGL((k_mf_hubbard<true>), dim3(grid), dim3(kBlock), 0, s, a);
    else                   hipLaunchKernelGGL((k_mf_hubbard<false>), dim3(grid), dim3(kBlock), 0, s, a);
    QBH_HIP(hipGetLastError());
    if (nparts_out) *nparts_out = grid;
    return QBH_OK;
}

}  // namespace qbh
