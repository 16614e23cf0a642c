// qbh_kron_prep.hip -- preparation kernels of the Kronecker split: tiled copies, placement and packing of the exchanged
// pieces, structure check, count / fill of the near and far parts, slot descriptors of the sliced far part.
#include <algorithm>

#include "qbh_internal.hpp"

namespace qbh {

// ---- Kronecker split: tiled copy of x, structure check, count / fill of the two parts ----
// Tiled copy of x for B = 8, through LDS: a workgroup moves 32 major indices x 8 bands; it reads 1 KB runs of x (64 minor indices
// of one major index) and writes 4 KB runs of the tiled copy (32 major indices of one band) -- row stores in 128-byte pieces cost
// several times their share of the bytes (tools/lab/region_probe).  The last, narrower band (S % 8 != 0) and other band widths
// take the element-wise kernel.
// xt_real (real wire of a split shard, qbh_opts.real_wire): the tiled copy is written as packed REAL PARTS (8 bytes per element);
// a non-zero imaginary part raises *flag (finish_real_wire turns that into a loud error)
__global__ __launch_bounds__(kBlock) void k_kron_tile_edge(const d2 *x, d2 *xt, KronTile t, int64_t band0, int xt_real, int *flag)
{
    // elements of bands >= band0
    const int64_t d0 = band0 * t.B, w = t.S - d0;
    const int64_t cnt = t.NU * w;
    bool bad = false;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cnt; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = e / w, r = u * t.S + d0 + (e - u * w);
        const d2 v = x[r];
        if (xt_real) {
            reinterpret_cast<double *>(xt)[t.tile(r)] = v.x;
            bad |= v.y != 0.0;
        } else {
            xt[t.tile(r)] = v;
        }
    }
    if (bad) *flag = 1;
}
__global__ __launch_bounds__(kBlock) void k_kron_tile8(const d2 *x, d2 *xt, KronTile t, int64_t nfb, int xt_real, int *flag)
{
    constexpr int TU = 32, TB = 8, LD = TB * 8 + 1;          // +1: the band-major read of the tile walks rows of the LDS array
    __shared__ d2 tilebuf[TU * LD];
    const int64_t tiles_u = (t.NU + TU - 1) / TU, tiles_b = (nfb + TB - 1) / TB;
    bool bad = false;
    for (int64_t w = blockIdx.x; w < tiles_u * tiles_b; w += gridDim.x) {
        const int64_t tb = w / tiles_u, tu = w - tb * tiles_u;     // consecutive workgroups: the same bands, consecutive major indices
        const int64_t u0 = tu * TU, b0 = tb * TB;
        const int nu = (int)(t.NU - u0 < TU ? t.NU - u0 : TU), nb = (int)(nfb - b0 < TB ? nfb - b0 : TB);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TU * TB * 8 / kBlock; ++i) {
            const int idx = threadIdx.x + i * kBlock, ul = idx >> 6, dl = idx & 63;
            if (ul < nu && dl < nb * 8) tilebuf[ul * LD + dl] = __builtin_nontemporal_load(x + (u0 + ul) * t.S + b0 * 8 + dl);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TU * TB * 8 / kBlock; ++i) {
            const int idx = threadIdx.x + i * kBlock, bl = idx >> 8, rest = idx & 255, ul = rest >> 3, j = rest & 7;
            if (bl < nb && ul < nu) {
                const d2 v = tilebuf[ul * LD + bl * 8 + j];
                const int64_t o = (b0 + bl) * 8 * t.NU + (u0 + ul) * 8 + j;
                if (xt_real) {
                    reinterpret_cast<double *>(xt)[o] = v.x;
                    bad |= v.y != 0.0;
                } else {
                    xt[o] = v;
                }
            }
        }
    }
    if (bad) *flag = 1;
}
int launch_kron_tile(const d2 *x, d2 *xt, int64_t n, const KronTile &t, hipStream_t s, int xt_real, int *flag)
{
    (void)n;
    if (xt_real && !flag) return QBH_EINVAL;
    const int64_t nfb = t.B == 8 ? t.S / 8 : 0;                  // full bands through the LDS kernel
    if (nfb > 0) hipLaunchKernelGGL(k_kron_tile8, dim3(4096), dim3(kBlock), 0, s, x, xt, t, nfb, xt_real, flag);
    if (nfb * t.B < t.S) hipLaunchKernelGGL(k_kron_tile_edge, dim3(nfb > 0 ? 256 : 2048), dim3(kBlock), 0, s, x, xt, t, nfb, xt_real, flag);
    QBH_HIP(hipGetLastError());
    return QBH_OK;
}

// Under a communicator the tiled blocks of the ranks arrive rank after rank (d_xfull, or d_xfull_r as packed real parts); the far
// part of EVERY shard indexes the tiled order of the WHOLE vector (KronTile{S, NUg, B}) -- the same 2-byte columns as the
// one-GPU operator, relative to the block's band -- so the pieces are moved to their place: band b of rank q's block (NU_q
// consecutive major indices, one contiguous run) becomes the run behind major index cu[q] of band b.  One launch per gather
// part, blockIdx.y = source rank; real wire: the 8-byte elements are expanded on the way (zero imaginary part).
__global__ __launch_bounds__(kBlock) void k_kron_place(KronPlace a)
{
    const int q = blockIdx.y;
    const int64_t nuq = a.cu[q + 1] - a.cu[q], full = a.nfb * a.B * nuq, wE = a.S - a.nfb * a.B;     // elements of rank q's full bands; width of the edge band
    const double *sr = reinterpret_cast<const double *>(a.src);
    if (a.list != nullptr) {
        // needed major indices only: work item = (band, listed major), B elements each (one 128-byte line of complex128)
        if (a.compact && q == a.skip) return;
        const int64_t nl = a.lo[q + 1] - a.lo[q];
        const int32_t *lst = a.list + a.lo[q];
        const int64_t nb = a.band1 - a.band0;
        for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < nb * nl * a.B; w += (int64_t)gridDim.x * kBlock) {
            const int64_t j = w % a.B, t = w / a.B, i = t % nl, b = a.band0 + t / nl;
            const int64_t ul = lst[i];
            int64_t e, o;
            const int64_t um = a.compact ? i : ul, nm = a.compact ? nl : nuq;      // position and count of the major indices in the source piece
            if (b < a.nfb) {
                e = b * a.B * nm + um * a.B + j;
                o = b * a.B * a.NUg + (a.cu[q] + ul) * a.B + j;
            } else {                                         // the narrow edge band: wE elements per major index
                if (j >= wE) continue;
                e = a.nfb * a.B * nm + um * wE + j;
                o = a.nfb * a.B * a.NUg + (a.cu[q] + ul) * wE + j;
            }
            a.dst[o] = a.real ? d2{sr[a.base[q] + e], 0.0} : a.src[a.base[q] + e];
        }
        return;
    }
    const int64_t e0 = a.off[q], e1 = e0 + a.len[q];
    for (int64_t e = e0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; e < e1; e += (int64_t)gridDim.x * kBlock) {
        int64_t o;
        if (e < full) {
            const int64_t b = e / (a.B * nuq), r = e - b * a.B * nuq;
            o = b * a.B * a.NUg + a.cu[q] * a.B + r;
        } else {
            o = a.nfb * a.B * a.NUg + a.cu[q] * wE + (e - full);
        }
        a.dst[o] = a.real ? d2{sr[a.base[q] + e], 0.0} : a.src[a.base[q] + e];
    }
}
int launch_kron_place(const KronPlace &a, hipStream_t s)
{
    int64_t longest = 0;
    for (int q = 0; q < a.nr; ++q) {
        const int64_t n = a.list ? ((a.compact && q == a.skip) ? 0 : (a.band1 - a.band0) * (a.lo[q + 1] - a.lo[q]) * a.B) : a.len[q];
        longest = n > longest ? n : longest;
    }
    if (longest <= 0 || a.nr <= 0) return QBH_OK;
    const int64_t gx = std::min<int64_t>(2048, (longest + kBlock - 1) / kBlock);
    return launch_kernel(k_kron_place, dim3((unsigned)gx, (unsigned)a.nr), kBlock, s, a);
}

// personalised exchange, sender side: for destination p (blockIdx.y) the listed major indices of the own tiled block, band-major
__global__ __launch_bounds__(kBlock) void k_kron_pack(KronPack a)
{
    const int p = blockIdx.y;
    const int64_t nl = a.lo[p + 1] - a.lo[p], wE = a.S - a.nfb * a.B, nb = a.nfb + (wE > 0 ? 1 : 0);
    const int32_t *lst = a.list + a.lo[p];
    const double *sr = reinterpret_cast<const double *>(a.src);
    double *dr = reinterpret_cast<double *>(a.dst);
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < nb * nl * a.B; w += (int64_t)gridDim.x * kBlock) {
        const int64_t j = w % a.B, t = w / a.B, i = t % nl, b = t / nl;
        const int64_t ul = lst[i];
        int64_t e, o;
        if (b < a.nfb) {
            e = b * a.B * a.NUq + ul * a.B + j;
            o = b * a.B * nl + i * a.B + j;
        } else {
            if (j >= wE) continue;
            e = a.nfb * a.B * a.NUq + ul * wE + j;
            o = a.nfb * a.B * nl + i * wE + j;
        }
        if (a.real) dr[a.base[p] + o] = sr[e];
        else        a.dst[a.base[p] + o] = a.src[e];
    }
}
int launch_kron_pack(const KronPack &a, hipStream_t s)
{
    int64_t longest = 0;
    const int64_t nb = a.nfb + ((a.S - a.nfb * a.B) > 0 ? 1 : 0);
    for (int p = 0; p < a.nr; ++p) longest = std::max<int64_t>(longest, nb * (a.lo[p + 1] - a.lo[p]) * a.B);
    if (longest <= 0 || a.nr <= 0) return QBH_OK;
    const int64_t gx = std::min<int64_t>(2048, (longest + kBlock - 1) / kBlock);
    return launch_kernel(k_kron_pack, dim3((unsigned)gx, (unsigned)a.nr), kBlock, s, a);
}

// which major indices of the whole operator does this shard read through its far and cross parts?  (Columns are positions in the
// tiled order of the whole vector: full band b, major u, j -> b B NUg + u B + j; edge band -> nfb B NUg + u wE + j.)
__global__ __launch_bounds__(kBlock) void k_kron_need(const uint16_t *c16_f, const int32_t *ja_f, int64_t far_slots, const int32_t *ja_x, int64_t nnz_x,
                                                      int64_t S, int64_t NUg, int B, uint8_t *need)
{
    const int64_t nfb = S / B, fullx = nfb * B * NUg, wE = S - nfb * B;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < far_slots; i += stride) {
        int64_t u;
        if (c16_f != nullptr) u = (int64_t)c16_f[i] % NUg;
        else {
            const int64_t c = ja_f[i];
            u = c < fullx ? (c % (B * NUg)) / B : (c - fullx) / (wE > 0 ? wE : 1);
        }
        if (u >= 0 && u < NUg) need[u] = 1;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz_x; i += stride) {
        const int64_t c = ja_x[i];
        const int64_t u = c < fullx ? (c % (B * NUg)) / B : (c - fullx) / (wE > 0 ? wE : 1);
        if (u >= 0 && u < NUg) need[u] = 1;
    }
}
int launch_kron_need(const uint16_t *c16_f, const int32_t *ja_f, int64_t far_slots, const int32_t *ja_x, int64_t nnz_x, int64_t S, int64_t NUg, int B,
                     uint8_t *need, hipStream_t s)
{
    return launch_kernel(k_kron_need, 2048, kBlock, s, c16_f, ja_f, far_slots, ja_x, nnz_x, S, NUg, B, need);
}

// coded values: the same two parts with cw-byte codes instead of complex128 values
__global__ __launch_bounds__(kBlock) void k_kron_fill_codes(const int64_t *ia, const int32_t *ja, const uint8_t *code, int cw, int64_t nrows, KronTile t,
                                                            const int64_t *ia_n, int32_t *ja_n, uint8_t *code_n, const int64_t *ia_f, int32_t *ja_f,
                                                            uint8_t *code_f)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nrows; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t.orig(f);
        const int64_t maj = r / t.S;
        int64_t pn = ia_n[r], pf = ia_f[f];
        for (int64_t k = ia[r]; k < ia[r + 1]; ++k) {
            const int32_t c = ja[k];
            if ((c / t.S) != maj) {
                ja_f[pf] = (int32_t)t.tile(c);
                for (int b = 0; b < cw; ++b) code_f[pf * cw + b] = code[k * cw + b];
                ++pf;
            } else {
                ja_n[pn] = c;
                for (int b = 0; b < cw; ++b) code_n[pn * cw + b] = code[k * cw + b];
                ++pn;
            }
        }
    }
}
int launch_kron_fill_codes(const int64_t *ia, const int32_t *ja, const uint8_t *code, int cw, int64_t nrows, const KronTile &t, const int64_t *ia_n,
                           int32_t *ja_n, uint8_t *code_n, const int64_t *ia_f, int32_t *ja_f, uint8_t *code_f, hipStream_t s)
{
    return launch_kernel(k_kron_fill_codes, 4096, kBlock, s, ia, ja, code, cw, nrows, t, ia_n, ja_n, code_n, ia_f, ja_f, code_f);
}
__global__ __launch_bounds__(kBlock) void k_kron_tile_re(const double *x, double *xt, int64_t n, KronTile t)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) xt[t.tile(r)] = x[r];
}
int launch_kron_tile_re(const double *x, double *xt, int64_t n, const KronTile &t, hipStream_t s)
{
    return launch_kernel(k_kron_tile_re, 2048, kBlock, s, x, xt, n, t);
}

// product structure with minor size S: every entry keeps the major index (near) or keeps the minor index (far)
__global__ __launch_bounds__(kBlock) void k_kron_check(const int64_t *ia, const int32_t *ja, int64_t nrows, int64_t S, int *flag)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t maj = r / S, mnr = r - maj * S;
        bool bad = false;
        for (int64_t k = ia[r]; k < ia[r + 1]; ++k) {
            const int64_t c = ja[k], cm = c / S;
            bad = bad || (cm != maj && c - cm * S != mnr);
        }
        if (bad) *flag = 1;
    }
}
int launch_kron_check(const int64_t *ia, const int32_t *ja, int64_t nrows, int64_t S, int *d_flag, hipStream_t s)
{
    return launch_kernel(k_kron_check, 4096, kBlock, s, ia, ja, nrows, S, d_flag);
}

__global__ __launch_bounds__(kBlock) void k_kron_count(const int64_t *ia, const int32_t *ja, int64_t nrows, KronTile t, int32_t *cnt_near,
                                                       int32_t *cnt_far)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nrows; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t.orig(f);
        const int64_t maj = r / t.S;
        int nf = 0;
        const int64_t s0 = ia[r], e0 = ia[r + 1];
        for (int64_t k = s0; k < e0; ++k) nf += (ja[k] / t.S) != maj;
        cnt_far[f] = nf;
        cnt_near[r] = (int)(e0 - s0) - nf;
    }
}
int launch_kron_count(const int64_t *ia, const int32_t *ja, int64_t nrows, const KronTile &t, int32_t *cnt_near, int32_t *cnt_far, hipStream_t s)
{
    return launch_kernel(k_kron_count, 4096, kBlock, s, ia, ja, nrows, t, cnt_near, cnt_far);
}

// near entries keep their row and column; far entries go to the tiled row with the tiled column (ascending in both)
__global__ __launch_bounds__(kBlock) void k_kron_fill(const int64_t *ia, const int32_t *ja, const d2 *val, int64_t nrows, KronTile t,
                                                      const int64_t *ia_n, int32_t *ja_n, d2 *val_n, const int64_t *ia_f, int32_t *ja_f, d2 *val_f)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nrows; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t.orig(f);
        const int64_t maj = r / t.S;
        int64_t pn = ia_n[r], pf = ia_f[f];
        for (int64_t k = ia[r]; k < ia[r + 1]; ++k) {
            const int32_t c = ja[k];
            if ((c / t.S) != maj) {
                ja_f[pf] = (int32_t)t.tile(c);
                val_f[pf++] = val[k];
            } else {
                ja_n[pn] = c;
                val_n[pn++] = val[k];
            }
        }
    }
}
// sliced far part: slots of a group (8 consecutive far rows) = 8 * (longest far row of the group)
__global__ __launch_bounds__(kBlock) void k_kron_group_width(const int32_t *cnt_far, int64_t nrows, int64_t ngroups, int32_t *gw)
{
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
        int mx = 0;
        for (int j = 0; j < 8; ++j) {
            const int64_t f = g * 8 + j;
            const int c = f < nrows ? cnt_far[f] : 0;
            mx = c > mx ? c : mx;
        }
        gw[g] = 8 * (mx > 0 ? mx : 1);       // an empty group keeps one (padding) slot per row: every row belongs to a block
    }
}
int launch_kron_group_width(const int32_t *cnt_far, int64_t nrows, int64_t ngroups, int32_t *gw, hipStream_t s)
{
    return launch_kernel(k_kron_group_width, 2048, kBlock, s, cnt_far, nrows, ngroups, gw);
}

// blocks of the sliced far part: block i = slots [512 i, 512 (i + 1)); r0 = the group that holds its first slot
// shift: the arrays of the far part start `shift` entries behind a 128-byte boundary (they follow the near part inside the
// operator's own arrays): the blocks are cut `shift` slots early so that every block starts ON a boundary (8 lines per 1 KB
// value load instead of 9, 2 per 256-byte column load instead of 3); the first block is that much shorter
__global__ __launch_bounds__(kBlock) void k_build_slotdesc(const int64_t *gia, int64_t ngroups, int64_t slots, WaveDesc *wd, int64_t n_wb, int64_t shift)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_wb + 2; i += (int64_t)gridDim.x * blockDim.x) {
        WaveDesc d;
        if (i >= n_wb) {
            d.p0 = slots;
            d.r0 = (int32_t)ngroups;
            d.pad = 0;
        } else {
            const int64_t P = i * 512 > shift ? i * 512 - shift : 0;
            int64_t lo = 0, hi = ngroups;            // first group with gia[g] > P
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (gia[mid] > P) hi = mid;
                else lo = mid + 1;
            }
            d.p0 = P;
            d.r0 = (int32_t)(lo - 1);
            d.pad = gia[lo - 1] < P ? 1 : 0;
        }
        wd[i] = d;
    }
}
int launch_build_slotdesc(const int64_t *gia, int64_t ngroups, int64_t slots, WaveDesc *wd, int64_t n_wb, int64_t shift, hipStream_t s)
{
    return launch_kernel(k_build_slotdesc, 2048, kBlock, s, gia, ngroups, slots, wd, n_wb, shift);
}

// rows of the groups that a block boundary cuts: zero before the far pass adds both parts
__global__ __launch_bounds__(kBlock) void k_zero_cut_groups(const WaveDesc *wd, int64_t n_wb, int64_t nrows, d2 *far)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_wb * 8; t += (int64_t)gridDim.x * blockDim.x) {
        const WaveDesc d = wd[t >> 3];
        const int64_t row = (int64_t)d.r0 * 8 + (t & 7);
        if ((d.pad & 1) && row < nrows) far[row] = d2{0.0, 0.0};
    }
}
int launch_zero_cut_groups(const WaveDesc *wd, int64_t n_wb, int64_t nrows, d2 *far, hipStream_t s)
{
    return launch_kernel(k_zero_cut_groups, 2048, kBlock, s, wd, n_wb, nrows, far);
}

// near entries as in k_kron_fill; far entries of far row f = 8g + j go to gia[g] + 8k + j (k-th far entry of the row), the
// rest of the group's slots are padding: value 0, column = the row's own tiled index (always a valid element of the tiled x)
__global__ __launch_bounds__(kBlock) void k_kron_fill_sliced(const int64_t *ia, const int32_t *ja, const d2 *val, int64_t nrows, KronTile t,
                                                             const int64_t *ia_n, int32_t *ja_n, d2 *val_n, const int64_t *gia, int64_t ngroups,
                                                             int32_t *ja_f, d2 *val_f)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < ngroups * 8; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = f >> 3, jj = f & 7;
        const int64_t gb = gia[g], w = (gia[g + 1] - gb) >> 3;
        int64_t k = 0;
        if (f < nrows) {
            const int64_t r = t.orig(f);
            const int64_t maj = r / t.S;
            int64_t pn = ia_n[r];
            for (int64_t q = ia[r]; q < ia[r + 1]; ++q) {
                const int32_t c = ja[q];
                if ((c / t.S) != maj) {
                    ja_f[gb + 8 * k + jj] = (int32_t)t.tile(c);
                    val_f[gb + 8 * k + jj] = val[q];
                    ++k;
                } else {
                    ja_n[pn] = c;
                    val_n[pn++] = val[q];
                }
            }
        }
        for (; k < w; ++k) {
            ja_f[gb + 8 * k + jj] = (int32_t)(f < nrows ? f : 0);
            val_f[gb + 8 * k + jj] = d2{0.0, 0.0};
        }
    }
}
int launch_kron_fill_sliced(const int64_t *ia, const int32_t *ja, const d2 *val, int64_t nrows, const KronTile &t, const int64_t *ia_n,
                            int32_t *ja_n, d2 *val_n, const int64_t *gia, int64_t ngroups, int32_t *ja_f, d2 *val_f, hipStream_t s)
{
    return launch_kernel(k_kron_fill_sliced, 4096, kBlock, s, ia, ja, val, nrows, t, ia_n, ja_n, val_n, gia, ngroups, ja_f, val_f);
}

int launch_kron_fill(const int64_t *ia, const int32_t *ja, const d2 *val, int64_t nrows, const KronTile &t, const int64_t *ia_n, int32_t *ja_n,
                     d2 *val_n, const int64_t *ia_f, int32_t *ja_f, d2 *val_f, hipStream_t s)
{
    return launch_kernel(k_kron_fill, 4096, kBlock, s, ia, ja, val, nrows, t, ia_n, ja_n, val_n, ia_f, ja_f, val_f);
}

}  // namespace qbh
