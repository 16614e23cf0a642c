// qbh_blas1.hip -- vector kernels of the solvers: reductions, BLAS-1 passes (complex and packed real), the Lanczos tail,
// start vector, Krylov-basis kernels and the real wire format.
#include "qbh_internal.hpp"
#include "qbh_device.hpp"

namespace qbh {

// -------------------------------------------------------------- BLAS-1 ---------
int blas_grid(int64_t n)
{
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g > kMaxRedBlocks) g = kMaxRedBlocks;
    if (g < 1) g = 1;
    return (int)g;
}

// second stage of every reduction: one workgroup sums `nparts` partials of `ncomp`
// components in a fixed order (run-to-run reproducible, no atomics).
__global__ __launch_bounds__(1024) void k_reduce_partials(const double *partials, int nparts, int ncomp,
                                                          double *out)
{
    __shared__ double sm[16];
    for (int c = 0; c < ncomp; ++c) {
        double v = 0.0;
        for (int i = threadIdx.x; i < nparts; i += 1024) v += partials[(size_t)i * ncomp + c];
        v = wave_sum(v);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < 16; ++w) t += sm[w];
            out[c] = t;
        }
    }
}

int launch_reduce_partials(const double *partials, int nparts, int ncomp, double *out, hipStream_t s)
{
    return launch_kernel(k_reduce_partials, 1, 1024, s, partials, nparts, ncomp, out);
}

// Tail of a pipelined Lanczos step (lanczos_core): the second stage of the axpy's |w'|^2 (the same summation order as
// k_reduce_partials, so b_m is the number the unpipelined step returns), then the scalars of src/lanczos.cc:200-214 in the
// arithmetic the host used to do -- a = sc_x * <u, w>, b = sqrt(|w'|^2), sc_new = 1 / b -- and the NEXT step's coefficients
// (alpha = sc_new, beta = -b * sc_x, axpy scale = -sc_new^2) left in state[] for the kernels of step m + 1, which the host has
// already enqueued.  The four numbers of this step go to a pinned host slot directly: no copy engine in the stream.
// sq_ready != nullptr (under a communicator): |w'|^2 has been reduced and all-reduced already (partials unused).
__global__ __launch_bounds__(1024) void k_lanczos_tail(const double *partials, int nparts, const double *dot, double *state, double *log_slot,
                                                       double sc_x_host, int use_host, const double *sq_ready)
{
    __shared__ double sm[16];
    double v = 0.0;
    if (sq_ready == nullptr)
        for (int i = threadIdx.x; i < nparts; i += 1024) v += partials[i];
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sq = 0.0;
        for (int w = 0; w < 16; ++w) sq += sm[w];
        if (sq_ready != nullptr) sq = sq_ready[0];
        const double sc_x = use_host ? sc_x_host : state[3];
        const double d = dot[0];
        const double a = sc_x * d;
        const double b = sqrt(sq);
        const double sc_new = 1.0 / b;
        state[0] = sc_new;
        state[1] = -b * sc_x;
        state[2] = -sc_new * sc_new;
        state[3] = sc_new;
        log_slot[0] = d;
        log_slot[1] = sq;
        log_slot[2] = a;
        log_slot[3] = b;
        __threadfence_system();
    }
}
int launch_lanczos_tail(const double *partials, int nparts, const double *dot, double *state, double *log_slot, double sc_x_host, int use_host,
                        hipStream_t s, const double *sq_ready)
{
    return launch_kernel(k_lanczos_tail, 1, 1024, s, partials, nparts, dot, state, log_slot, sc_x_host, use_host, sq_ready);
}

__global__ __launch_bounds__(kBlock) void k_dotc(const d2 *x, const d2 *y, int64_t n, double *partials)
{
    __shared__ double red[8];
    double acc[2] = {0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const d2 a = x[i], b = y[i];
        acc[0] += a.x * b.x + a.y * b.y;
        acc[1] += a.x * b.y - a.y * b.x;
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x * 2 + 0] = acc[0];
        partials[blockIdx.x * 2 + 1] = acc[1];
    }
}

int launch_dotc(const d2 *x, const d2 *y, int64_t n, double *partials, hipStream_t s)
{
    return launch_kernel(k_dotc, blas_grid(n), kBlock, s, x, y, n, partials);
}

// y += alpha*x ; partial |y|^2   (cblas_zaxpy + cblas_dznrm2 in one pass: K5+K6)
// yr (optional): packed real parts of the updated y -- the next SpMV's gather source in the real fast
// path, produced here instead of by a separate k_pack_real pass; flag as in k_pack_real.
// alpha_dev != nullptr: the coefficient is alpha.x * alpha_dev[0] (a scalar a previous kernel of the same stream left
// on the device -- the Lanczos step then needs one host synchronisation instead of two)
// scale_dev != nullptr (pipelined Lanczos step): alpha.x itself is read from the device as well
__global__ __launch_bounds__(kBlock) void k_axpy_norm(d2 alpha, const double *alpha_dev, const d2 *x, d2 *y, int64_t n,
                                                      double *partials, double *yr, int *flag, const double *scale_dev)
{
    __shared__ double red[4];
    double acc[1] = {0.0};
    bool bad = false;
    if (scale_dev != nullptr) alpha.x = scale_dev[0];
    if (alpha_dev != nullptr) alpha = d2{alpha.x * alpha_dev[0], 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        d2 v = y[i] + cmul(alpha, x[i]);
        y[i] = v;
        if (yr != nullptr) {
            yr[i] = v.x;
            bad |= (v.y != 0.0);
        }
        acc[0] += v.x * v.x + v.y * v.y;
    }
    if (bad) *flag = 1;
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

int launch_axpy_norm(d2 alpha, const double *alpha_dev, const d2 *x, d2 *y, int64_t n, double *partials, double *yr, int *flag,
                     hipStream_t s, const double *scale_dev)
{
    return launch_kernel(k_axpy_norm, blas_grid(n), kBlock, s, alpha, alpha_dev, x, y, n, partials, yr, flag, scale_dev);
}

// The same update for an operator with a Kronecker split (band 8): y is the next SpMV's x in every driver, and the far pass
// gathers from its TILED copy (KronTile) -- written here, by the pass that produces y, instead of by a k_kron_tile launch
// in front of the SpMV (one read of y and one launch less per step).  Work item = 32 major indices x 8 bands through LDS as in
// k_kron_tile8: 1 KB runs of x / y in, 1 KB runs of y and 4 KB runs of the tiled copy out; the narrow last band (S % 8 != 0)
// element-wise.  MODE 0: y += alpha x (alpha_dev as in k_axpy_norm), partial |y|^2.  MODE 1: y = x + alpha.x * y (k_xpby), no sum.
// Static assignment of the items to workgroups: the partial sums are run-to-run reproducible.
// item = TU major indices x TB bands: reads runs of TB * 128 bytes of x and y (TB * 8 minor indices of one major index), writes
// the updated y in natural order (the same runs) AND through LDS in tiled order (runs of TU * 128 bytes: TU major indices of one
// band).  TU * TB = 256 keeps the tile at 33 KB.  QBH_TILE_TU / QBH_TILE_TB: build-time tuning (round 4: 32 x 8; round 5, measured through whole bench lines: 8 x 32 saves 0.15-0.25 ms of the 2.2 ms pass).
#ifndef QBH_TILE_TU
#define QBH_TILE_TU 8
#endif
#ifndef QBH_TILE_TB
#define QBH_TILE_TB 32
#endif
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_axpy_norm_tile8(d2 alpha, const double *alpha_dev, const d2 *x, d2 *y, d2 *yt, KronTile t,
                                                            int64_t nfb, double *partials, const double *scale_dev, int yt_real, int *flag)
{
    bool bad = false;           // yt_real (real wire of a split shard): the tiled copy as packed real parts, *flag on a non-zero imaginary part
    constexpr int TU = QBH_TILE_TU, TB = QBH_TILE_TB, RW = TB * 8, LD = RW + 1;      // RW: elements of one major index in the item
    static_assert(TU * TB == 256 && (TU & (TU - 1)) == 0 && (TB & (TB - 1)) == 0, "TU x TB = 256, powers of two");
    __shared__ d2 tilebuf[TU * LD];
    __shared__ double red[4];
    double acc[1] = {0.0};
    if (MODE == 0 && scale_dev != nullptr) alpha.x = scale_dev[0];
    if (MODE == 0 && alpha_dev != nullptr) alpha = d2{alpha.x * alpha_dev[0], 0.0};
    auto upd = [&](d2 xv, d2 yv) -> d2 {
        if (MODE == 0) {
            const d2 v = yv + cmul(alpha, xv);
            acc[0] += v.x * v.x + v.y * v.y;
            return v;
        }
        return xv + alpha.x * yv;
    };
    const int64_t tiles_u = (t.NU + TU - 1) / TU, tiles_b = (nfb + TB - 1) / TB;
    for (int64_t w = blockIdx.x; w < tiles_u * tiles_b; w += gridDim.x) {
        const int64_t tb = w / tiles_u, tu = w - tb * tiles_u;
        const int64_t u0 = tu * TU, b0 = tb * TB;
        const int nu = (int)(t.NU - u0 < TU ? t.NU - u0 : TU), nb = (int)(nfb - b0 < TB ? nfb - b0 : TB);
        d2 xv[TU * TB * 8 / kBlock], yv[TU * TB * 8 / kBlock];
#pragma unroll
        for (int i = 0; i < TU * TB * 8 / kBlock; ++i) {
            const int idx = threadIdx.x + i * kBlock, ul = idx / RW, dl = idx % RW;
            const bool in = ul < nu && dl < nb * 8;
            const int64_t r = in ? (u0 + ul) * t.S + b0 * 8 + dl : 0;
            xv[i] = __builtin_nontemporal_load(x + r);
            yv[i] = __builtin_nontemporal_load(y + r);
        }
        __syncthreads();                               // the previous item's tile has been read
#pragma unroll
        for (int i = 0; i < TU * TB * 8 / kBlock; ++i) {
            const int idx = threadIdx.x + i * kBlock, ul = idx / RW, dl = idx % RW;
            if (ul < nu && dl < nb * 8) {
                const d2 v = upd(xv[i], yv[i]);
                y[(u0 + ul) * t.S + b0 * 8 + dl] = v;
                tilebuf[ul * LD + dl] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TU * TB * 8 / kBlock; ++i) {
            const int idx = threadIdx.x + i * kBlock, bl = idx / (TU * 8), rest = idx % (TU * 8), ul = rest >> 3, j = rest & 7;
            if (bl < nb && ul < nu) {
                const d2 v = tilebuf[ul * LD + bl * 8 + j];
                const int64_t o = (b0 + bl) * 8 * t.NU + (u0 + ul) * 8 + j;
                if (yt_real) {
                    reinterpret_cast<double *>(yt)[o] = v.x;
                    bad |= v.y != 0.0;
                } else {
                    yt[o] = v;
                }
            }
        }
    }
    const int64_t d0 = nfb * 8, we = t.S - d0;             // the narrow last band
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < t.NU * we; e += (int64_t)gridDim.x * kBlock) {
        const int64_t u = e / we, r = u * t.S + d0 + (e - u * we);
        const d2 v = upd(x[r], y[r]);
        y[r] = v;
        if (yt_real) {
            reinterpret_cast<double *>(yt)[t.tile(r)] = v.x;
            bad |= v.y != 0.0;
        } else {
            yt[t.tile(r)] = v;
        }
    }
    if (bad) *flag = 1;
    if (MODE == 0) {
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
    }
}

// grid = blas_grid(n): the partial sums are reduced by the same second stage as k_axpy_norm's
int launch_axpy_norm_tile(d2 alpha, const double *alpha_dev, const d2 *x, d2 *y, d2 *yt, int64_t n, const KronTile &t, double *partials,
                          hipStream_t s, const double *scale_dev, int yt_real, int *flag)
{
    if (t.B != 8 || t.S < 8 || (yt_real && !flag)) return QBH_EINVAL;
    hipLaunchKernelGGL(k_axpy_norm_tile8<0>, dim3(blas_grid(n)), dim3(kBlock), 0, s, alpha, alpha_dev, x, y, yt, t, t.S / 8, partials, scale_dev, yt_real, flag);
    QBH_HIP(hipGetLastError());
    return QBH_OK;
}
int launch_xpby_tile(const d2 *x, double b, d2 *y, d2 *yt, int64_t n, const KronTile &t, hipStream_t s, int yt_real, int *flag)
{
    if (t.B != 8 || t.S < 8 || (yt_real && !flag)) return QBH_EINVAL;
    hipLaunchKernelGGL(k_axpy_norm_tile8<1>, dim3(blas_grid(n)), dim3(kBlock), 0, s, d2{b, 0.0}, (const double *)nullptr, x, y, yt, t, t.S / 8,
                       (double *)nullptr, (const double *)nullptr, yt_real, flag);
    QBH_HIP(hipGetLastError());
    return QBH_OK;
}

// T = d2, or double for vectors stored as doubles (all-real CG, see qbh_eigenvec_cg_dev)
__device__ __forceinline__ double abs2(d2 v) { return v.x * v.x + v.y * v.y; }
__device__ __forceinline__ double abs2(double v) { return v * v; }

template <typename T>
__global__ __launch_bounds__(kBlock) void k_nrm2sq(const T *x, int64_t n, double *partials)
{
    __shared__ double red[4];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) acc[0] += abs2(x[i]);
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

int launch_nrm2sq(const d2 *x, int64_t n, double *partials, hipStream_t s)
{
    return launch_kernel(k_nrm2sq<d2>, blas_grid(n), kBlock, s, x, n, partials);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_scal(double a, T *x, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) x[i] = a * x[i];
}

// y = a * x (out of place: the exit of the pipelined Lanczos driver moves a vector into the caller's slot and normalises it in one pass)
__global__ __launch_bounds__(kBlock) void k_scal_to(double a, const d2 *x, d2 *y, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) y[i] = a * x[i];
}
int launch_scal_to(double a, const d2 *x, d2 *y, int64_t n, hipStream_t s)
{
    return launch_kernel(k_scal_to, blas_grid(n), kBlock, s, a, x, y, n);
}

int launch_scal(double a, d2 *x, int64_t n, hipStream_t s)
{
    return launch_kernel(k_scal<d2>, blas_grid(n), kBlock, s, a, x, n);
}

// y = x + b*y   (CG direction update p = r + beta^2 p, src/lanczos.cc:327-328)
// all-real Lanczos: y += alpha * x on vectors stored as doubles, partial |y|^2 (alpha_dev as in k_axpy_norm)
// yt != nullptr: the result also in the tiled order t (16 consecutive minor indices = one aligned 128-byte line): the next SpMV of
// a coded Kronecker split (qbh_kronc.hip) gathers its far part from it and needs no k_kron_tile_re
__global__ __launch_bounds__(kBlock) void k_axpy_norm_re(double alpha, const double *alpha_dev, const double *x, double *y,
                                                         int64_t n, double *partials, double *yt, KronTile t)
{
    __shared__ double red[4];
    double acc[1] = {0.0};
    if (alpha_dev != nullptr) alpha *= alpha_dev[0];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double v = y[i] + alpha * x[i];
        y[i] = v;
        if (yt != nullptr) {
            if (n < 2147483647LL && t.B == 16) {          // 32-bit index arithmetic (the 64-bit divisions of tile() cost more than the store)
                const uint32_t S32 = (uint32_t)t.S, u = (uint32_t)i / S32, d = (uint32_t)i - u * S32, b = d >> 4;
                const uint32_t wB = S32 - (b << 4) < 16u ? S32 - (b << 4) : 16u;
                yt[(int64_t)b * 16 * t.NU + (int64_t)(u * wB + (d & 15u))] = v;
            } else {
                yt[t.tile(i)] = v;
            }
        }
        acc[0] += v * v;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

int launch_axpy_norm_re(double alpha, const double *alpha_dev, const double *x, double *y, int64_t n, double *partials, hipStream_t s, double *yt,
                        const KronTile &t)
{
    return launch_kernel(k_axpy_norm_re, blas_grid(n), kBlock, s, alpha, alpha_dev, x, y, n, partials, yt, t);
}

// yr != nullptr: also the packed real parts of the result (it is the next SpMV's gather source in the real fast path)
__global__ __launch_bounds__(kBlock) void k_xpby(const d2 *x, double b, d2 *y, int64_t n, double *yr, int *flag)
{
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const d2 v = x[i] + b * y[i];
        y[i] = v;
        if (yr != nullptr) {
            yr[i] = v.x;
            bad |= (v.y != 0.0);
        }
    }
    if (bad) *flag = 1;
}

int launch_xpby(const d2 *x, double b, d2 *y, int64_t n, double *yr, int *flag, hipStream_t s)
{
    return launch_kernel(k_xpby, blas_grid(n), kBlock, s, x, b, y, n, yr, flag);
}

// v += alpha*p ; r -= alpha*pp ; partial |r|^2   (src/lanczos.cc:324-326 in one pass)
// delta_dev != nullptr: alpha = accu2 / delta with delta = <p, pp> left on the device by the SpMV that produced pp (no host
// round-trip between the SpMV and this pass); the arithmetic of the host expression, operation by operation (no contraction)
__global__ __launch_bounds__(kBlock) void k_cg_update(d2 alpha, const d2 *p, const d2 *pp, d2 *v, d2 *r,
                                                      int64_t n, double *partials, const double *delta_dev, double accu2)
{
    __shared__ double red[4];
    double acc[1] = {0.0};
    if (delta_dev != nullptr) {
        const double re = delta_dev[0], im = delta_dev[1];
        const double den = __dadd_rn(__dmul_rn(re, re), __dmul_rn(im, im));
        alpha = d2{__ddiv_rn(__dmul_rn(accu2, re), den), -__ddiv_rn(__dmul_rn(accu2, im), den)};
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        v[i] = v[i] + cmul(alpha, p[i]);
        const d2 rr = r[i] - cmul(alpha, pp[i]);
        r[i] = rr;
        acc[0] += rr.x * rr.x + rr.y * rr.y;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

int launch_cg_update(d2 alpha, const d2 *p, const d2 *pp, d2 *v, d2 *r, int64_t n, double *partials,
                     hipStream_t s, const double *delta_dev, double accu2)
{
    return launch_kernel(k_cg_update, blas_grid(n), kBlock, s, alpha, p, pp, v, r, n, partials, delta_dev, accu2);
}

// ---- the same passes on vectors stored as doubles (all-real CG, see qbh_eigenvec_cg_dev) ----
__global__ __launch_bounds__(kBlock) void k_cg_update_re(double alpha, const double *p, const double *pp, double *v, double *r,
                                                         int64_t n, double *partials)
{
    __shared__ double red[4];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        v[i] = v[i] + alpha * p[i];
        const double rr = r[i] - alpha * pp[i];
        r[i] = rr;
        acc[0] += rr * rr;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(kBlock) void k_xpby_re(const double *x, double b, double *y, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) y[i] = x[i] + b * y[i];
}

__global__ __launch_bounds__(kBlock) void k_dot_re(const double *x, const double *y, int64_t n, double *partials)
{
    __shared__ double red[4];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) acc[0] += x[i] * y[i];
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

int launch_dot_re(const double *x, const double *y, int64_t n, double *partials, hipStream_t s)
{
    return launch_kernel(k_dot_re, blas_grid(n), kBlock, s, x, y, n, partials);
}

int launch_cg_update_re(double alpha, const double *p, const double *pp, double *v, double *r, int64_t n, double *partials, hipStream_t s)
{
    return launch_kernel(k_cg_update_re, blas_grid(n), kBlock, s, alpha, p, pp, v, r, n, partials);
}
int launch_xpby_re(const double *x, double b, double *y, int64_t n, hipStream_t s)
{
    return launch_kernel(k_xpby_re, blas_grid(n), kBlock, s, x, b, y, n);
}
int launch_nrm2sq_re(const double *x, int64_t n, double *partials, hipStream_t s)
{
    return launch_kernel(k_nrm2sq<double>, blas_grid(n), kBlock, s, x, n, partials);
}
int launch_scal_re(double a, double *x, int64_t n, hipStream_t s)
{
    return launch_kernel(k_scal<double>, blas_grid(n), kBlock, s, a, x, n);
}

// ------------------------------------------------------ start vector -----------
// vec_randomize (src/miscellaneous.cc:371-386): std::minstd_rand0 is the Lehmer
// generator s <- 16807 s mod (2^31-1); element j takes draw j+1.  Each lane jumps ahead
// with a modular power and then walks a short run, so the device vector is bit-identical
// to the host one before normalisation.
constexpr int kRandRun = 16;

__device__ __forceinline__ uint64_t lehmer_pow(uint64_t e)
{
    const uint64_t M = 2147483647ULL;
    uint64_t base = 16807ULL, r = 1ULL;
    while (e) {
        if (e & 1ULL) r = (r * base) % M;
        base = (base * base) % M;
        e >>= 1;
    }
    return r;
}

// xr != nullptr: the vector is stored as packed doubles (qbh_vec_randomize_real), same stream of numbers
// major_inv != nullptr (qbh_opts.major_partition): local element j = (local major j / S, minor j % S) is drawn at position
// major_inv[j / S] * S + j % S of the stream -- the same physical vector whatever order the major indices are held in
__global__ __launch_bounds__(kBlock) void k_randomize(d2 *x, double *xr, int64_t n, int64_t global_offset, uint32_t seed,
                                                      double *partials, const int32_t *major_inv, int64_t S)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const uint64_t M = 2147483647ULL;
    double acc[1] = {0.0};
    const int64_t nruns = (n + kRandRun - 1) / kRandRun;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    uint64_t s0 = (uint64_t)seed % M;
    if (s0 == 0) s0 = 1;
    for (int64_t run = (int64_t)blockIdx.x * kBlock + threadIdx.x; run < nruns; run += stride) {
        const int64_t j0 = run * kRandRun;
        auto pos = [&](int64_t j) -> uint64_t { return major_inv ? (uint64_t)((int64_t)major_inv[j / S] * S + j % S) : (uint64_t)(global_offset + j); };
        uint64_t state = (s0 * lehmer_pow(pos(j0))) % M;   // state before the draw of element j0
        const int64_t j1 = (j0 + kRandRun < n) ? j0 + kRandRun : n;
        for (int64_t j = j0; j < j1; ++j) {
            if (major_inv != nullptr && j > j0 && j % S == 0) state = (s0 * lehmer_pow(pos(j))) % M;      // a new major index: another stretch of the stream
            state = (state * 16807ULL) % M;
            const double t = (double)state * (1.0 / 2147483647.0);
            d2 v;
            v.x = t - 0.5;
            v.y = 0.0;
            if (xr != nullptr) xr[j] = v.x;
            else               x[j] = v;
            acc[0] += v.x * v.x;
        }
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

int launch_randomize(d2 *x, double *xr, int64_t n, int64_t global_offset, uint32_t seed, double *partials, hipStream_t s, const int32_t *major_inv,
                     int64_t S)
{
    const int64_t nruns = (n + kRandRun - 1) / kRandRun;
    return launch_kernel(k_randomize, blas_grid(nruns), kBlock, s, x, xr, n, global_offset, seed, partials, major_inv, S);
}

__global__ __launch_bounds__(kBlock) void k_fill_const(d2 *x, int64_t n, double re)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    d2 v = {re, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) x[i] = v;
}

int launch_fill_const(d2 *x, int64_t n, double re, hipStream_t s)
{
    return launch_kernel(k_fill_const, blas_grid(n), kBlock, s, x, n, re);
}


// --------------------------------------------- Krylov-basis kernels (qbh_iram) --
// h_i = <V_i, w> for NV basis vectors in ONE pass over w (full re-orthogonalisation of the
// thick-restart Lanczos basis); partials[(block*NV + i)*2 + {re,im}].
template <int NV>
__global__ __launch_bounds__(kBlock) void k_multi_dot(const d2 *V, int64_t ldv, const d2 *w, int64_t n, int nv,
                                                      double *partials)
{
    __shared__ double red[2 * NV * 4];
    double acc[2 * NV];
#pragma unroll
    for (int i = 0; i < 2 * NV; ++i) acc[i] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        const d2 wv = w[e];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (i < nv) {
                const d2 vi = V[(size_t)i * ldv + e];
                acc[2 * i] += vi.x * wv.x + vi.y * wv.y;
                acc[2 * i + 1] += vi.x * wv.y - vi.y * wv.x;
            }
        }
    }
    block_sum<2 * NV>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 2 * NV; ++i) partials[(size_t)blockIdx.x * 2 * NV + i] = acc[i];
    }
}

int launch_multi_dot8(const d2 *V, int64_t ldv, const d2 *w, int64_t n, int nv, double *partials, hipStream_t s)
{
    return launch_kernel((k_multi_dot<8>), blas_grid(n), kBlock, s, V, ldv, w, n, nv, partials);
}

// w -= sum_i c_i V_i  (c complex), one pass; optionally the partial sums of |w|^2 of the result
__global__ __launch_bounds__(kBlock) void k_multi_axpy(const d2 *V, int64_t ldv, Coef8 c, int nv, d2 *w, int64_t n,
                                                       double *partials)
{
    __shared__ double red[4];
    double nrm[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        d2 acc = w[e];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < nv) {
                const d2 ci = {c.v[2 * i], c.v[2 * i + 1]};
                acc -= cmul(ci, V[(size_t)i * ldv + e]);
            }
        }
        w[e] = acc;
        nrm[0] += acc.x * acc.x + acc.y * acc.y;
    }
    if (partials != nullptr) {
        block_sum<1>(nrm, red);
        if (threadIdx.x == 0) partials[blockIdx.x] = nrm[0];
    }
}

int launch_multi_axpy8(const d2 *V, int64_t ldv, const Coef8 &c, int nv, d2 *w, int64_t n, double *partials, hipStream_t s)
{
    return launch_kernel(k_multi_axpy, blas_grid(n), kBlock, s, V, ldv, c, nv, w, n, partials);
}

// Restart rotation, in place: V[:, c] <- sum_i S[i + c*m] V[:, i]  for c < keep (S real, m <= 32).
// S is real, so the rotation acts on the real and imaginary parts independently: the basis is treated as vectors of
// doubles (2n per complex vector; n for the packed-real basis).  MMAX = 32 or 64 basis vectors are held in registers.
template <int MMAX>
__global__ __launch_bounds__(kBlock) void k_basis_rotate(double *V, int64_t ldv, int64_t n, int m, int keep, const double *S)
{
    __shared__ double Ss[MMAX * MMAX];
    for (int i = threadIdx.x; i < m * keep; i += kBlock) Ss[i] = S[i];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        double x[MMAX];
#pragma unroll
        for (int i = 0; i < MMAX; ++i)
            if (i < m) x[i] = V[(size_t)i * ldv + e];
        for (int c = 0; c < keep; ++c) {
            double y = 0.0;
#pragma unroll
            for (int i = 0; i < MMAX; ++i)
                if (i < m) y += Ss[i + c * m] * x[i];
            V[(size_t)c * ldv + e] = y;
        }
    }
}

// V (complex view: leading dimension ldv and length n in complex elements) <- V S[:, 0..keep), m <= 64
int launch_basis_rotate(d2 *V, int64_t ldv, int64_t n, int m, int keep, const double *d_S, hipStream_t s)
{
    double *Vd = reinterpret_cast<double *>(V);
    return launch_kernel(m <= 32 ? k_basis_rotate<32> : k_basis_rotate<64>, blas_grid(2 * n), kBlock, s, Vd, 2 * ldv, 2 * n, m, keep, d_S);
}

// ------------------------------------------------- real wire format -------------
// For a real Hamiltonian and real start vector every Lanczos / CG vector has an exactly zero imaginary
// part, so the all-gather of x can carry 8 instead of 16 bytes per element (lossless).  pack also raises
// *flag if it ever meets a non-zero imaginary part (checked by the drivers: never silently wrong).
__global__ __launch_bounds__(kBlock) void k_pack_real(const d2 *x, double *out, int64_t n, int *flag)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const d2 v = x[i];
        out[i] = v.x;
        bad |= (v.y != 0.0);
    }
    if (bad) *flag = 1;
}

__global__ __launch_bounds__(kBlock) void k_unpack_real(const double *in, d2 *out, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = d2{in[i], 0.0};
}

// partial sums of |Im x|^2 (entry check of the drivers)
__global__ __launch_bounds__(kBlock) void k_imag_norm(const d2 *x, int64_t n, double *partials)
{
    __shared__ double red[4];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) acc[0] += x[i].y * x[i].y;
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

int launch_pack_real(const d2 *x, double *out, int64_t n, int *flag, hipStream_t s)
{
    return launch_kernel(k_pack_real, blas_grid(n), kBlock, s, x, out, n, flag);
}

int launch_unpack_real(const double *in, d2 *out, int64_t n, hipStream_t s)
{
    return launch_kernel(k_unpack_real, blas_grid(n), kBlock, s, in, out, n);
}

int launch_imag_norm(const d2 *x, int64_t n, double *partials, hipStream_t s)
{
    return launch_kernel(k_imag_norm, blas_grid(n), kBlock, s, x, n, partials);
}

}  // namespace qbh
