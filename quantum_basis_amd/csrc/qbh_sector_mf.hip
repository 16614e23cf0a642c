// qbh_sector_mf.hip -- qbh_mf_hubbard_repr (toolkit and the Hubbard family: qbh_sector.hpp)
#include "qbh_sector.hpp"

// ---------------------- Hubbard momentum sector, matrix-free with a stored remainder --------
// qbh_mf_hubbard_repr: see MfSec in qbh_internal.hpp.  The operator is  y = MF(x) + R x : MF covers, for every row of a
// regular down block, the diagonal, all up hops (inside the block, g* = identity) and every down hop whose target block is
// regular; R (ordinary CSR, the handle's arrays) holds the complete rows of stabilised blocks and the few entries of
// regular rows that land in a stabilised block.  4x5 at half filling: 364 GB of CSR become ~40 MB of tables + ~1 GB of
// remainder, and the sector runs on ONE GPU.
namespace qbh {
namespace {

constexpr int kSecTile = 1024;     // rows of one work item unless the debug knob sec_tile says otherwise (MfSec::tile)

// row i of the remainder: full row for a stabilised block, otherwise only the flagged down hops (bit t of flags[blk])
__device__ int hubrepr_row_rem(const HubReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim,
                               int64_t i, const MfSecBlock *blk, int64_t n_blocks, const uint64_t *flags, int32_t *cols, d2 *vals)
{
    const uint64_t a = reps[i];
    const uint32_t d = (uint32_t)(a >> R.n_sites);
    int64_t lo = 0, hi = n_blocks;                     // block of this row: ascending down patterns
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (blk[mid].d < d) lo = mid + 1;
        else hi = mid;
    }
    if (!blk[lo].regular) return hubrepr_row(R, tab, reps, info, dim, i, cols, vals);
    const uint64_t *fl = flags + lo * 8;
    bool any = false;
    for (int w = 0; w < 8; ++w) any = any || fl[w] != 0;
    if (!any) return 0;
    const double sa = (double)(info[i] & 0x7f);
    const uint64_t mlow = (1ULL << R.n_sites) - 1ULL;
    const uint64_t au = a & mlow, ad = a >> R.n_sites;
    int n = 0;
    for (int t = 0; t < R.n_terms; ++t) {
        if (!((fl[t >> 6] >> (t & 63)) & 1ULL)) continue;
        const int ti = R.ti[t], tj = R.tj[t];
        const double ar = R.adn[t][0], ai = R.adn[t][1];
        if ((ar == 0.0 && ai == 0.0) || ti == tj) continue;
        if (!((ad >> ti) & 1ULL) || ((ad >> tj) & 1ULL)) continue;
        const int lo_s = ti < tj ? ti : tj, hi_s = ti < tj ? tj : ti;
        const uint64_t between = ((1ULL << hi_s) - 1ULL) & ~((2ULL << lo_s) - 1ULL);
        int par = __popcll(ad & between) & 1;
        const uint64_t occ2 = ad ^ (1ULL << ti) ^ (1ULL << tj);
        const uint64_t c = au | (occ2 << R.n_sites);
        int g = 0, pt = 0;
        const uint64_t b = hubrepr_canonical(R, tab, c, &g, &pt);
        par ^= pt;
        const int64_t l2 = sector_find(reps, dim, b);
        const uint8_t cj = info[l2];
        if (cj & 0x80) continue;
        const double f = (par ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
        const double cr = R.chr[2 * g], cim = -R.chr[2 * g + 1];
        const d2 v = {f * (ar * cr - ai * cim), f * (ar * cim + ai * cr)};
        row_merge(cols, vals, n, kHubReprMaxRow, 0, l2, v);    // no diagonal slot: the target is in another block
    }
    row_sort(cols, vals, n);
    return n;
}

__global__ __launch_bounds__(128) void k_secrem_count(const HubReprDev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                      int64_t dim, const MfSecBlock *blk, int64_t n_blocks, const uint64_t *flags,
                                                      int32_t *cnt)
{
    int32_t cols[kHubReprMaxRow];
    d2 vals[kHubReprMaxRow];
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x; i < dim; i += stride)
        cnt[i] = hubrepr_row_rem(*Rp, tab, reps, info, dim, i, blk, n_blocks, flags, cols, vals);
}

__global__ __launch_bounds__(256) void k_secrem_flag(const int32_t *cnt, int64_t dim, int32_t *flag)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += stride) flag[i] = cnt[i] > 0 ? 1 : 0;
}

// compact remainder: the p-th row with entries is row rrow[p], its entries sit at [ria[p], ria[p+1])
__global__ __launch_bounds__(128) void k_secrem_fill(const HubReprDev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                     int64_t dim, const MfSecBlock *blk, int64_t n_blocks, const uint64_t *flags,
                                                     const int64_t *ia_full, const int64_t *pos, int32_t *rrow, int64_t *ria,
                                                     int32_t *rja, d2 *rval)
{
    int32_t cols[kHubReprMaxRow];
    d2 vals[kHubReprMaxRow];
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x; i < dim; i += stride) {
        if (i == 0) ria[pos[dim]] = ia_full[dim];
        if (ia_full[i + 1] == ia_full[i]) continue;
        const int m = hubrepr_row_rem(*Rp, tab, reps, info, dim, i, blk, n_blocks, flags, cols, vals);
        const int64_t p = pos[i], p0 = ia_full[i];
        rrow[p] = (int32_t)i;
        ria[p] = p0;
        for (int q = 0; q < m; ++q) {
            rja[p0 + q] = cols[q];
            rval[p0 + q] = vals[q];
        }
    }
}

// ---- orbit order (MfSec): indices of the ascending order -> positions
__device__ __forceinline__ int64_t sec_orbit_index(const MfSecBlock *blk, int64_t n_blocks, const uint32_t *opos, int64_t i)
{
    int64_t lo = 0, hi = n_blocks - 1;                 // last block with row0 <= i
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (blk[mid].row0 <= i) lo = mid;
        else hi = mid - 1;
    }
    const MfSecBlock B = blk[lo];
    return B.regular ? B.row0 + (int64_t)opos[i - B.row0] : i;
}
__global__ __launch_bounds__(256) void k_sec_orbit_remap(const MfSecBlock *blk, int64_t n_blocks, const uint32_t *opos, int32_t *rrow,
                                                         int64_t n_rrows, int32_t *rja, int64_t rnnz)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n_rrows; q += stride)
        rrow[q] = (int32_t)sec_orbit_index(blk, n_blocks, opos, rrow[q]);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < rnnz; q += stride)
        rja[q] = (int32_t)sec_orbit_index(blk, n_blocks, opos, rja[q]);
}
__global__ __launch_bounds__(256) void k_sec_orbit_map(const MfSecBlock *blk, const int64_t *item, int64_t n_items, const uint32_t *opos,
                                                       uint32_t *map, int tile_rows)
{
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t w = item[it];
        const MfSecBlock B = blk[w >> 20];
        const int tile = (int)(w & 0xFFFFF);
        for (int j = 0; j < tile_rows / 256; ++j) {
            const int r = tile * tile_rows + j * 256 + (int)threadIdx.x;
            if (r >= B.nrows) break;
            map[B.row0 + r] = (uint32_t)(B.row0 + (B.regular ? (int64_t)opos[r] : (int64_t)r));
        }
    }
}

constexpr int kSecMaxHops = 128;

// y <- alpha MF(x) + beta y + gamma x for every row.  One work item = 1024 rows of one down block; an XCD takes a
// contiguous run of items, so the workgroups that share an L2 sweep the same block -- and, hop by hop, the same target
// blocks -- at the same time.
// ORD: the ordered walk of the wave kernels (qbh_spmv_wave.hip; DynWalk in qbh_device.hpp) at workgroup granularity -- every XCD owns one contiguous
// eighth of the items and its workgroups draw them one at a time from a counter, so they cannot drift apart over the ~1600 items
// each of them processes (the static assignment keeps them on one block only while they stay in lock step).
template <bool REALX, int kSecUnroll, bool ORD>
__global__ __launch_bounds__(256) void k_mf_sector(MfSecArgs a)
{
    const MfSec &T = *a.t;
    __shared__ MfSecHop sh[kSecMaxHops];
    __shared__ int64_t s_item;
    const int64_t cu = T.cu;
    const int nslot = (int)(gridDim.x >> 3), xcd = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3);
    const int64_t per = (a.n_items + 7) >> 3, xbase = xcd * per, xend = xbase + per < a.n_items ? xbase + per : a.n_items;
    for (int64_t base = 0; ORD || base < a.n_items; base += gridDim.x) {     // ORD: until the XCD's counter runs out
        int64_t it = base + (int64_t)xcd * nslot + slot;
        __syncthreads();
        if (ORD) {
            if (threadIdx.x == 0) s_item = xbase + (int64_t)atomicInc(a.ctr + xcd * 32, 0xFFFFFFFFu);
            __syncthreads();
            it = s_item;
            if (it >= xend) break;
        }
        if (it >= a.n_items) continue;
        const int64_t w = T.item[it];
        const MfSecBlock B = T.blk[w >> 20];
        const int tile = (int)(w & 0xFFFFF);
        if (B.regular)
            for (int h = threadIdx.x; h < B.nhop; h += 256) sh[h] = T.hop[B.hop0 + h];
        __syncthreads();
        for (int j = 0; j < T.tile / 256; ++j) {
            const int r = tile * T.tile + j * 256 + (int)threadIdx.x;
            if (r >= B.nrows) break;
            const int64_t row = B.row0 + r;
            d2 sum = {0.0, 0.0};
            if (B.regular) {
                const uint32_t u = T.ucfg[r], d = B.d;
                double dr = T.U * (double)__popc(u & d);
                for (int p = 0; p < T.n_pairs; ++p) {
                    const int iu = (u >> T.pi[p]) & 1, id = (d >> T.pi[p]) & 1, ju = (u >> T.pj[p]) & 1, jd = (d >> T.pj[p]) & 1;
                    dr += T.pv[p][0] * (iu & ju) + T.pv[p][1] * (iu & jd) + T.pv[p][2] * (id & ju) + T.pv[p][3] * (id & jd);
                }
                if (T.has_number_terms) {
                    for (uint32_t m = u; m; m &= m - 1) dr += T.nup[__ffs(m) - 1];
                    for (uint32_t m = d; m; m &= m - 1) dr += T.ndn[__ffs(m) - 1];
                }
                if (REALX) sum.x = dr * a.v.xr[row];
                else       sum = dr * a.v.xg[row];
                for (int k0 = 0; k0 < T.w_up; k0 += kSecUnroll) {          // up hops: inside the block
                    uint32_t e[kSecUnroll];
#pragma unroll
                    for (int q = 0; q < kSecUnroll; ++q) e[q] = k0 + q < T.w_up ? T.upell[(size_t)(k0 + q) * cu + r] : 0xFFFFFFFFu;
                    if (REALX) {
                        double xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = e[q] != 0xFFFFFFFFu ? a.v.xr[B.row0 + (e[q] & 0xFFFFFFu)] : 0.0;
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (e[q] != 0xFFFFFFFFu) sum.x += T.updict[e[q] >> 24] * xv[q];
                    } else {
                        d2 xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = e[q] != 0xFFFFFFFFu ? a.v.xg[B.row0 + (e[q] & 0xFFFFFFu)] : d2{0.0, 0.0};
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (e[q] != 0xFFFFFFFFu) sum += T.updict[e[q] >> 24] * xv[q];
                    }
                    if (e[kSecUnroll - 1] == 0xFFFFFFFFu) break;
                }
                for (int h0 = 0; h0 < B.nhop; h0 += kSecUnroll) {          // down hops into regular blocks
                    uint32_t pr[kSecUnroll];
#pragma unroll
                    for (int q = 0; q < kSecUnroll; ++q) pr[q] = h0 + q < B.nhop ? T.prank[(size_t)sh[h0 + q].g * cu + r] : 0u;
                    if (REALX) {
                        double xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = h0 + q < B.nhop ? a.v.xr[sh[h0 + q].off + (pr[q] & 0x7FFFFFFFu)] : 0.0;
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (h0 + q < B.nhop) sum.x += ((pr[q] >> 31) ? -sh[h0 + q].cr : sh[h0 + q].cr) * xv[q];
                    } else {
                        d2 xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            xv[q] = h0 + q < B.nhop ? a.v.xg[sh[h0 + q].off + (pr[q] & 0x7FFFFFFFu)] : d2{0.0, 0.0};
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (h0 + q < B.nhop) {
                                const double sg = (pr[q] >> 31) ? -1.0 : 1.0;
                                const double cr = sg * sh[h0 + q].cr, ci = sg * sh[h0 + q].ci;
                                sum += d2{cr * xv[q].x - ci * xv[q].y, cr * xv[q].y + ci * xv[q].x};
                            }
                    }
                }
            }
            d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
            if (a.v.beta != 0.0) yo = a.v.y_re ? d2{a.v.y_re[row], 0.0} : a.v.y[row];
            if (a.v.gamma != 0.0) xi = a.v.y_re ? d2{a.xl_re[row], 0.0} : a.v.xl[row];
            const d2 yn = a.v.alpha * sum + a.v.beta * yo + a.v.gamma * xi;
            if (a.v.y_re) a.v.y_re[row] = yn.x;
            else          a.v.y[row] = yn;
        }
    }
}

// The same product with the rows of a regular block in ORBIT ORDER (MfSec): no per-row rank tables.  A down hop reads the target
// block at the positions of the tile itself, permuted inside runs of <= n_trans rows (coalesced; every block is read front to
// back once per hop that lands in it, whatever the L2 holds); an up hop reads a run of the block's own x named by the ORBIT's
// slot table.  Per row and block 26 bytes of tables (pattern, orbit, element | kind, two sign masks) instead of
// 4 (w_up + nhop) = 170; the group tables (composition, position inside an orbit per stabiliser kind) sit in LDS.
// ORD: items drawn from per-XCD counters (the default: under the static assignment the workgroups finish far apart, 87 -> 61 ms on
// 4x5 with 8+8).  Loading the streams that are read once (row tables, target blocks, old y) non-temporally was measured and changes
// neither the L2 misses nor the time; smaller items keep more of the block's own x in the L2 (tile 256: -17 % misses) but pay more
// in per-item work than that saves (profiles/r5_lab/sector_orbit_order_timings.txt).
// a value every lane holds (read from LDS or through a lane-held index) moved to scalar registers, so that what is derived from
// it -- block descriptors, base addresses -- is scalar work and the gathers take the form  uniform base + 32-bit lane offset
__device__ __forceinline__ int sec_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t sec_uni(int64_t v)
{
    return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v));
}
template <typename V>
__device__ __forceinline__ V sec_at(const V *base, uint32_t i)               // base uniform, i < 2^32 / sizeof(V)
{
    return *reinterpret_cast<const V *>(reinterpret_cast<const char *>(base) + (size_t)(uint32_t)(i * (uint32_t)sizeof(V)));
}
template <bool REALX, int kSecUnroll, bool ORD>
__global__ __launch_bounds__(256) void k_mf_sector_orb(MfSecArgs a)
{
    const MfSec &T = *a.t;
    __shared__ MfSecHop sh[kSecMaxHops];
    __shared__ int64_t s_item;
    __shared__ uint8_t s_comp[64 * 64];     // [a][b]: the down hops read [g][e] -- g the same in every lane, e running with the lane
    __shared__ uint8_t s_compT[64 * 64];    // [b][a]: the up hops read comp[e][s] as [s][e] -- e * 64 would put all lanes into two banks
    __shared__ uint8_t s_kidx[16 * 64];
    __shared__ double s_dict[256];
    for (int i = threadIdx.x; i < 64 * 64 / 4; i += 256) reinterpret_cast<uint32_t *>(s_comp)[i] = reinterpret_cast<const uint32_t *>(T.comp)[i];
    for (int i = threadIdx.x; i < 64 * 64; i += 256) s_compT[(i & 63) * 64 + (i >> 6)] = T.comp[i];
    for (int i = threadIdx.x; i < 16 * 64 / 4; i += 256) reinterpret_cast<uint32_t *>(s_kidx)[i] = reinterpret_cast<const uint32_t *>(T.kidx)[i];
    s_dict[threadIdx.x] = T.updict[threadIdx.x];
    const int64_t n_orb = a.n_orb;
    const int W = a.w_orb;
    const int nslot = (int)(gridDim.x >> 3), xcd = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3);
    const int64_t per = (a.n_items + 7) >> 3, xbase = xcd * per, xend = xbase + per < a.n_items ? xbase + per : a.n_items;
    for (int64_t base = 0; ORD || base < a.n_items; base += gridDim.x) {
        int64_t it = base + (int64_t)xcd * nslot + slot;
        __syncthreads();
        if (ORD) {
            if (threadIdx.x == 0) s_item = xbase + (int64_t)atomicInc(a.ctr + xcd * 32, 0xFFFFFFFFu);
            __syncthreads();
            it = sec_uni(s_item);
            if (it >= xend) break;
        }
        if (it >= a.n_items) continue;
        const int64_t w = T.item[it];
        const MfSecBlock B = T.blk[w >> 20];
        const int tile = (int)(w & 0xFFFFF);
        if (B.regular)
            for (int h = threadIdx.x; h < B.nhop; h += 256) sh[h] = T.hop[B.hop0 + h];
        __syncthreads();
        const double *xrb = REALX ? a.v.xr + B.row0 : nullptr;              // the block's own x
        const d2 *xgb = REALX ? nullptr : a.v.xg + B.row0;
        for (int j = 0; j < a.tile / 256; ++j) {
            const int tb = tile * a.tile + j * 256;                       // the same in every lane
            const uint32_t ln = threadIdx.x;
            const int p = tb + (int)ln;
            if (p >= B.nrows) break;
            const int64_t row = B.row0 + p;
            d2 sum = {0.0, 0.0};
            if (B.regular) {
                const uint32_t u = sec_at(a.ucfg + tb, ln), d = B.d, o = sec_at(a.oid + tb, ln), ek = sec_at(a.oek + tb, ln);
                const uint64_t tp = sec_at(a.tpar + tb, ln), us = sec_at(a.usgn + tb, ln);
                const int e = (int)(ek & 63u), kind = (int)(ek >> 6);
                const uint8_t *kx = s_kidx + kind * 64;
                const uint32_t pb = (uint32_t)(p - (int)kx[e]);           // the orbit's first member inside a block
                double dr = T.U * (double)__popc(u & d);
                for (int q = 0; q < T.n_pairs; ++q) {
                    const int iu = (u >> T.pi[q]) & 1, id = (d >> T.pi[q]) & 1, ju = (u >> T.pj[q]) & 1, jd = (d >> T.pj[q]) & 1;
                    dr += T.pv[q][0] * (iu & ju) + T.pv[q][1] * (iu & jd) + T.pv[q][2] * (id & ju) + T.pv[q][3] * (id & jd);
                }
                if (T.has_number_terms) {
                    for (uint32_t m = u; m; m &= m - 1) dr += T.nup[__ffs(m) - 1];
                    for (uint32_t m = d; m; m &= m - 1) dr += T.ndn[__ffs(m) - 1];
                }
                if (REALX) sum.x = dr * sec_at(xrb + tb, ln);
                else       sum = dr * sec_at(xgb + tb, ln);
                const uint8_t *ce = s_compT + e;                          // comp[e][s] at ce[s * 64]
                for (int k0 = 0; k0 < W; k0 += kSecUnroll) {              // up hops: runs of the block's own x
                    uint32_t en[kSecUnroll], ex[kSecUnroll];
#pragma unroll
                    for (int q = 0; q < kSecUnroll; ++q) en[q] = k0 + q < W ? sec_at(a.utab + (size_t)(k0 + q) * (size_t)n_orb, o) : 0u;
#pragma unroll
                    for (int q = 0; q < kSecUnroll; ++q)                   // rare: another amplitude than the first, a stabilised target orbit
                        ex[q] = (en[q] & (1u << 30)) ? (uint32_t)sec_at(a.uext + (size_t)(k0 + q) * (size_t)n_orb, o) : 0u;
                    uint32_t ix[kSecUnroll];
#pragma unroll
                    for (int q = 0; q < kSecUnroll; ++q)
                        ix[q] = (en[q] & 0xFFFFFFu) + (uint32_t)s_kidx[(int)(ex[q] >> 8) * 64 + (int)ce[(int)((en[q] >> 18) & (63u << 6))]];
                    if (REALX) {
                        double xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = (en[q] >> 31) ? sec_at(xrb, ix[q]) : 0.0;
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) {
                            const double am = s_dict[(int)(ex[q] & 255u)];
                            sum.x += (((us >> (k0 + q)) & 1ULL) ? -am : am) * xv[q];
                        }
                    } else {
                        d2 xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = (en[q] >> 31) ? sec_at(xgb, ix[q]) : d2{0.0, 0.0};
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) {
                            const double am = s_dict[(int)(ex[q] & 255u)];
                            sum += (((us >> (k0 + q)) & 1ULL) ? -am : am) * xv[q];
                        }
                    }
                    if (!(en[kSecUnroll - 1] >> 31)) break;
                }
                for (int h0 = 0; h0 < B.nhop; h0 += kSecUnroll) {          // down hops into regular blocks: the same positions there
                    uint32_t ix[kSecUnroll];
                    int64_t off[kSecUnroll];
                    int gg[kSecUnroll];
#pragma unroll
                    for (int q = 0; q < kSecUnroll; ++q) {
                        const int hh = h0 + q < B.nhop ? h0 + q : 0;
                        off[q] = sec_uni(sh[hh].off);
                        gg[q] = sec_uni(sh[hh].g);
                        ix[q] = pb + (uint32_t)kx[(int)s_comp[gg[q] * 64 + e]];
                    }
                    if (REALX) {
                        double xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = h0 + q < B.nhop ? sec_at(a.v.xr + off[q], ix[q]) : 0.0;
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (h0 + q < B.nhop) sum.x += (((tp >> gg[q]) & 1ULL) ? -sh[h0 + q].cr : sh[h0 + q].cr) * xv[q];
                    } else {
                        d2 xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = h0 + q < B.nhop ? sec_at(a.v.xg + off[q], ix[q]) : d2{0.0, 0.0};
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (h0 + q < B.nhop) {
                                const double sg = ((tp >> gg[q]) & 1ULL) ? -1.0 : 1.0;
                                const double cr = sg * sh[h0 + q].cr, ci = sg * sh[h0 + q].ci;
                                sum += d2{cr * xv[q].x - ci * xv[q].y, cr * xv[q].y + ci * xv[q].x};
                            }
                    }
                }
            }
            d2 yo = {0.0, 0.0}, xi = {0.0, 0.0};
            if (a.v.beta != 0.0) yo = a.v.y_re ? d2{sec_at(a.v.y_re + B.row0 + tb, ln), 0.0} : sec_at(a.v.y + B.row0 + tb, ln);
            if (a.v.gamma != 0.0) xi = a.v.y_re ? d2{sec_at(a.xl_re + B.row0 + tb, ln), 0.0} : sec_at(a.v.xl + B.row0 + tb, ln);
            const d2 yn = a.v.alpha * sum + a.v.beta * yo + a.v.gamma * xi;
            if (a.v.y_re) a.v.y_re[row] = yn.x;
            else          a.v.y[row] = yn;
        }
    }
}

// the stored remainder: eight lanes per row that has entries (the rows of stabilised blocks hold ~40 entries, a regular row with
// a hop into a stabilised block one to three; with one lane per row every lane walked its own row and each 20-byte entry cost a
// 128-byte line: 40 GB and 6.0 ms per apply at C4 as written for a 3.4 GB remainder; now 2.6 ms)
template <bool REALX>
__global__ __launch_bounds__(256) void k_sec_remainder(MfSecArgs a)
{
    constexpr int TPR = 8;
    const int sub = (int)(threadIdx.x & (TPR - 1));
    const int64_t stride = (int64_t)gridDim.x * (256 / TPR);
    for (int64_t p = (int64_t)blockIdx.x * (256 / TPR) + (int64_t)(threadIdx.x / TPR); p < a.n_rrows; p += stride) {
        d2 sum = {0.0, 0.0};
        const int64_t q1 = a.ria[p + 1];
        for (int64_t q = a.ria[p] + sub; q < q1; q += TPR) {
            const d2 v = a.rval[q];
            if (REALX) {
                sum.x += v.x * a.v.xr[a.rja[q]];
            } else {
                const d2 xv = a.v.xg[a.rja[q]];
                sum += d2{v.x * xv.x - v.y * xv.y, v.x * xv.y + v.y * xv.x};
            }
        }
        for (int off = TPR / 2; off > 0; off >>= 1) {
            sum.x += __shfl_xor(sum.x, off, 64);
            if (!REALX) sum.y += __shfl_xor(sum.y, off, 64);
        }
        if (sub == 0) {
            const int64_t row = a.rrow[p];
            if (a.v.y_re) a.v.y_re[row] += a.v.alpha * sum.x;
            else          a.v.y[row] += a.v.alpha * sum;
        }
    }
}

// <x, y> and |y|^2 of the finished product
__global__ __launch_bounds__(256) void k_sec_reduce(MfSecArgs a)
{
    __shared__ double red[12];
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.dim; i += stride) {
        const d2 xi = a.v.y_re ? d2{a.xl_re[i], 0.0} : a.v.xl[i];
        const d2 yn = a.v.y_re ? d2{a.v.y_re[i], 0.0} : a.v.y[i];
        acc[0] += xi.x * yn.x + xi.y * yn.y;
        acc[1] += xi.x * yn.y - xi.y * yn.x;
        acc[2] += yn.x * yn.x + yn.y * yn.y;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < 3; ++c)
        for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_xor(acc[c], off, 64);
    if (lane == 0)
        for (int c = 0; c < 3; ++c) red[c * 4 + wave] = acc[c];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) a.v.partials[(size_t)blockIdx.x * 3 + c] = (red[c * 4] + red[c * 4 + 1]) + (red[c * 4 + 2] + red[c * 4 + 3]);
}

}  // namespace

template <bool REALX, int UN>
static int sector_orbit_launch_t(const MfSecArgs &a, hipStream_t s)
{
    static std::atomic<int> occ{0};            // the same value on every device of one model; a race writes it twice
    if (occ.load() == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_mf_sector_orb<REALX, UN, true>, 256, 0) != hipSuccess || n <= 0) n = 4;
        occ.store(n);
    }
    int grid = 256 * occ.load();
    if (debug_sw().sec_grid >= 8) grid = (debug_sw().sec_grid / 8) * 8;
    if (a.ctr != nullptr) hipLaunchKernelGGL((k_mf_sector_orb<REALX, UN, true>), dim3(grid), dim3(256), 0, s, a);
    else                  hipLaunchKernelGGL((k_mf_sector_orb<REALX, UN, false>), dim3(grid), dim3(256), 0, s, a);
    return QBH_OK;
}

template <bool REALX, int UN>
static int sector_launch_t(const MfSecArgs &a, hipStream_t s)
{
    // persistent grid: exactly the resident workgroups (a multiple of 8), so that the XCD-contiguous item order holds
    static std::atomic<int> occ{0};            // the same value on every device of one model; a race writes it twice
    if (occ.load() == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_mf_sector<REALX, UN, false>, 256, 0) != hipSuccess || n <= 0) n = 4;
        occ.store(n);
    }
    int grid = 256 * occ.load();
    if (debug_sw().sec_grid >= 8) grid = (debug_sw().sec_grid / 8) * 8;
    if (a.ctr != nullptr) hipLaunchKernelGGL((k_mf_sector<REALX, UN, true>), dim3(grid), dim3(256), 0, s, a);
    else                  hipLaunchKernelGGL((k_mf_sector<REALX, UN, false>), dim3(grid), dim3(256), 0, s, a);
    return QBH_OK;
}

int launch_mf_sector(const MfSecArgs &a, hipStream_t s, int *nparts_out)
{
    static int un = 0;
    if (un == 0) {
        un = 8;
        if (debug_sw().sec_unroll) un = debug_sw().sec_unroll;              // tuning experiments: 4, 8, 16
    }
    if (a.orbit) {
        if (a.v.xr != nullptr) {
            if (un == 4) sector_orbit_launch_t<true, 4>(a, s);
            else         sector_orbit_launch_t<true, 8>(a, s);
        } else {
            if (un == 4) sector_orbit_launch_t<false, 4>(a, s);
            else         sector_orbit_launch_t<false, 8>(a, s);
        }
    } else if (a.v.xr != nullptr) {
        if (un == 4)       sector_launch_t<true, 4>(a, s);
        else if (un == 16) sector_launch_t<true, 16>(a, s);
        else               sector_launch_t<true, 8>(a, s);
    } else {
        if (un == 4)       sector_launch_t<false, 4>(a, s);
        else               sector_launch_t<false, 8>(a, s);
    }
    QBH_HIP(hipGetLastError());
    if (a.n_rrows > 0) {
        const int rg = blas_grid(a.n_rrows * 8);
        if (a.v.xr != nullptr) hipLaunchKernelGGL(k_sec_remainder<true>, dim3(rg), dim3(256), 0, s, a);
        else                 hipLaunchKernelGGL(k_sec_remainder<false>, dim3(rg), dim3(256), 0, s, a);
        QBH_HIP(hipGetLastError());
    }
    const int parts = blas_grid(a.dim);
    if (a.v.partials != nullptr) {
        hipLaunchKernelGGL(k_sec_reduce, dim3(parts), dim3(256), 0, s, a);
        QBH_HIP(hipGetLastError());
    }
    if (nparts_out) *nparts_out = parts;
    return QBH_OK;
}

}  // namespace qbh

extern "C" int qbh_mf_hubbard_repr(qbh_csr **out, int n_sites, int n_up, int n_dn, int n_terms, const int32_t *term_sites,
                                   const qbh_z *amp_up, const qbh_z *amp_dn, double U, int n_pairs, const int32_t *pair_sites,
                                   const double *pair_v, int n_trans, const int32_t *perms, const double *chars, double fake_pos,
                                   int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    const char *who = "qbh_mf_hubbard_repr";
    if (!out || (n_terms > 0 && (!term_sites || !amp_up || !amp_dn)) || !perms || !chars || n_sites <= 0 || n_sites > 24 || n_up < 0 ||
        n_up > n_sites || n_dn < 0 || n_dn > n_sites || n_terms < 0 || n_pairs < 0 || n_pairs > 128 ||
        (n_pairs > 0 && (!pair_sites || !pair_v)) || n_trans < 1 || n_trans > kReprMaxTrans) {
        set_error("%s: invalid argument (<= 24 sites, <= 128 density-density terms, <= 64 translations)", who);
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP(hipSetDevice(opts->device));
    // ---- the operator, exactly as qbh_gen_hubbard_repr merges it (the non-regular blocks and the remainder rows go
    // through hubrepr_row); no spin-exchange terms here
    TermMap tmap;
    QBH_TRY(merge_terms(n_sites, n_terms, term_sites, amp_up, amp_dn, 0, who, tmap));
    std::vector<HubReprDev> rr(1);
    std::vector<uint64_t> tab;
    QBH_TRY(hubrepr_symmetry(rr[0], tab, n_sites, n_up, n_dn, n_trans, perms, chars, who));
    HubReprDev &R = rr[0];
    for (const auto &kv : tmap) {
        R.ti[R.n_terms] = (int8_t)kv.first.first;
        R.tj[R.n_terms] = (int8_t)kv.first.second;
        R.aup[R.n_terms][0] = kv.second[0];
        R.aup[R.n_terms][1] = kv.second[1];
        R.adn[R.n_terms][0] = kv.second[2];
        R.adn[R.n_terms][1] = kv.second[3];
        if (kv.second[1] != 0.0 || (kv.first.first == kv.first.second && kv.second[3] != 0.0)) {
            set_error("%s: complex up-species or number-operator amplitudes are not supported by the matrix-free form", who);
            return QBH_EUNSUPP;
        }
        R.n_terms++;
    }
    R.U = U;
    R.fake_pos = fake_pos;
    for (int p = 0; p < n_pairs; ++p) {
        const int i = pair_sites[2 * p], j = pair_sites[2 * p + 1];
        if (i < 0 || i >= n_sites || j < 0 || j >= n_sites) {
            set_error("%s: density-density term %d acts on a site outside the lattice", who, p);
            return QBH_EINVAL;
        }
        R.pi[p] = (int8_t)i;
        R.pj[p] = (int8_t)j;
        for (int c = 0; c < 4; ++c) R.pv[p][c] = pair_v[4 * p + c];
    }
    R.n_pairs = n_pairs;

    // ---- host tables
    std::vector<uint32_t> ucfg, dcfg;
    enumerate_configs(n_sites, n_up, ucfg);
    enumerate_configs(n_sites, n_dn, dcfg);
    const int64_t cu = (int64_t)ucfg.size();
    if (cu >= (1 << 24)) {
        set_error("%s: more than 2^24 up configurations", who);
        return QBH_EUNSUPP;
    }
    auto image = [&](int g, uint32_t s) {
        uint32_t o = 0;
        for (uint32_t m = s; m; m &= m - 1) o |= 1u << perms[(size_t)g * n_sites + __builtin_ctz(m)];
        return o;
    };
    auto parity = [&](int g, uint32_t s) {
        uint32_t seen = 0;
        int par = 0;
        for (uint32_t m = s; m; m &= m - 1) {
            const int img = perms[(size_t)g * n_sites + __builtin_ctz(m)];
            par ^= __builtin_popcount(seen >> img) & 1;
            seen |= 1u << img;
        }
        return par;
    };
    auto between_par = [](uint32_t occ, int i, int j) {
        const int lo = std::min(i, j), hi = std::max(i, j);
        const uint32_t between = (uint32_t)(((1ULL << hi) - 1ULL) & ~((2ULL << lo) - 1ULL));
        return __builtin_popcount(occ & between) & 1;
    };
    // translated up patterns: rank and parity
    std::vector<uint32_t> prank((size_t)n_trans * (size_t)cu), uimg((size_t)n_trans * (size_t)cu);
    for (int g = 0; g < n_trans; ++g)
        for (int64_t r = 0; r < cu; ++r) {
            const uint32_t im = image(g, ucfg[(size_t)r]);
            uimg[(size_t)g * cu + r] = im;
            const uint32_t rk = (uint32_t)(std::lower_bound(ucfg.begin(), ucfg.end(), im) - ucfg.begin());
            prank[(size_t)g * cu + r] = rk | ((uint32_t)parity(g, ucfg[(size_t)r]) << 31);
        }
    // up-hop table (ELL) with a dictionary of signed amplitudes
    std::vector<std::vector<std::pair<uint32_t, double>>> uprow((size_t)cu);
    int w_up = 0;
    for (int64_t r = 0; r < cu; ++r) {
        const uint32_t u = ucfg[(size_t)r];
        std::map<uint32_t, double> row;
        for (int t = 0; t < R.n_terms; ++t) {
            const int ti = R.ti[t], tj = R.tj[t];
            if (ti == tj || R.aup[t][0] == 0.0) continue;
            if (!((u >> ti) & 1u) || ((u >> tj) & 1u)) continue;
            const uint32_t u2 = u ^ (1u << ti) ^ (1u << tj);
            const uint32_t rk = (uint32_t)(std::lower_bound(ucfg.begin(), ucfg.end(), u2) - ucfg.begin());
            row[rk] += R.aup[t][0] * (between_par(u, ti, tj) ? -1.0 : 1.0);
        }
        for (const auto &e : row)
            if (e.second * e.second >= 1e-28) uprow[(size_t)r].push_back(e);
        w_up = std::max(w_up, (int)uprow[(size_t)r].size());
    }
    std::vector<double> updict;
    std::vector<uint32_t> upell((size_t)std::max(w_up, 1) * (size_t)cu, 0xFFFFFFFFu);
    for (int64_t r = 0; r < cu; ++r)
        for (size_t k = 0; k < uprow[(size_t)r].size(); ++k) {
            const double v = uprow[(size_t)r][k].second;
            size_t code = std::find(updict.begin(), updict.end(), v) - updict.begin();
            if (code == updict.size()) {
                if (updict.size() >= 255) {
                    set_error("%s: more than 255 distinct up-hop amplitudes", who);
                    return QBH_EUNSUPP;
                }
                updict.push_back(v);
            }
            upell[k * (size_t)cu + (size_t)r] = ((uint32_t)code << 24) | uprow[(size_t)r][k].first;
        }
    // ---- the orbit order of the up patterns (MfSec, qbh_opts.sector_orbit): built and CHECKED here, position by position and
    // translation by translation / slot by slot, against the rank tables above; anything that does not hold (translations that
    // are not a group, up amplitudes that are not translation invariant, too many stabiliser kinds or slots) keeps the
    // ascending order and the rank tables
    int sec_tile = kSecTile;
    if (debug_sw().sec_tile == 256 || debug_sw().sec_tile == 512 || debug_sw().sec_tile == 2048) sec_tile = debug_sw().sec_tile;
    const bool want_orbit = opts ? opts->sector_orbit != 0 : true;
    bool orbit = want_orbit && n_trans <= 64;
    std::vector<uint32_t> opos, oid, ucfg_o;        // old rank -> position; orbit of a position; pattern at a position
    std::vector<uint16_t> oek;
    std::vector<uint64_t> tpar, usgn;
    std::vector<uint32_t> utab;                     // base' | s << 24 | ext << 30 | valid << 31
    std::vector<uint16_t> uext;                     // code | kind' << 8 of the slots whose ext bit is set
    std::vector<uint8_t> gcomp((size_t)64 * 64, 0), kidx((size_t)16 * 64, 0);
    int w_orb = 0, n_kinds = 0;
    int64_t n_orb = 0;
    std::vector<double> odict;
    if (orbit) {
        for (int a = 0; a < n_trans && orbit; ++a)          // comp[a][b]: "b, then a"
            for (int b = 0; b < n_trans && orbit; ++b) {
                int c = -1;
                for (int q = 0; q < n_trans && c < 0; ++q) {
                    bool same = true;
                    for (int st = 0; st < n_sites && same; ++st)
                        same = perms[(size_t)q * n_sites + st] == perms[(size_t)a * n_sites + perms[(size_t)b * n_sites + st]];
                    if (same) c = q;
                }
                if (c < 0) orbit = false;
                else gcomp[(size_t)a * 64 + b] = (uint8_t)c;
            }
        for (int a = 0; a < n_trans && orbit; ++a)          // distinct elements
            for (int b = a + 1; b < n_trans && orbit; ++b) {
                bool same = true;
                for (int st = 0; st < n_sites && same; ++st) same = perms[(size_t)a * n_sites + st] == perms[(size_t)b * n_sites + st];
                if (same) orbit = false;
            }
    }
    if (orbit) {
        std::vector<int32_t> orb_of((size_t)cu, -1);
        std::vector<uint8_t> elem((size_t)cu, 0), kind_of_orb;
        std::vector<uint32_t> base_of_orb, rep_of_orb;
        std::vector<uint64_t> kind_mask;                  // stabiliser (bit a: image(a, u0) = u0) of every kind
        opos.assign((size_t)cu, 0);
        uint32_t nextpos = 0;
        for (int64_t r = 0; r < cu && orbit; ++r) {
            if (orb_of[(size_t)r] >= 0) continue;
            const int32_t o = (int32_t)base_of_orb.size();
            uint64_t stab = 0;
            uint8_t idx_here[64];
            int nm = 0;
            for (int a = 0; a < n_trans; ++a) {
                const int64_t rk = (int64_t)(prank[(size_t)a * cu + r] & 0x7FFFFFFFu);
                if (rk == r) stab |= 1ULL << a;
                if (orb_of[(size_t)rk] < 0) {
                    orb_of[(size_t)rk] = o;
                    elem[(size_t)rk] = (uint8_t)a;
                    opos[(size_t)rk] = nextpos + (uint32_t)nm;
                    ++nm;
                }
                idx_here[a] = (uint8_t)(opos[(size_t)rk] - nextpos);
            }
            int kd = -1;
            for (size_t q = 0; q < kind_mask.size(); ++q)
                if (kind_mask[q] == stab) kd = (int)q;
            if (kd < 0) {
                if (kind_mask.empty() && __builtin_popcountll(stab) != 1) {     // kind 0 is the trivial stabiliser: reserve it
                    uint64_t triv = 0;
                    for (int a = 0; a < n_trans; ++a) {
                        bool ident = true;
                        for (int st = 0; st < n_sites && ident; ++st) ident = perms[(size_t)a * n_sites + st] == st;
                        if (ident) triv |= 1ULL << a;
                    }
                    if (__builtin_popcountll(triv) != 1) { orbit = false; break; }
                    kind_mask.push_back(triv);
                    for (int a = 0; a < n_trans; ++a) kidx[(size_t)a] = (uint8_t)a;
                }
                if (kind_mask.size() >= 16) { orbit = false; break; }
                kd = (int)kind_mask.size();
                kind_mask.push_back(stab);
                for (int a = 0; a < n_trans; ++a) kidx[(size_t)kd * 64 + a] = idx_here[a];
            } else {
                for (int a = 0; a < n_trans; ++a)
                    if (kidx[(size_t)kd * 64 + a] != idx_here[a]) orbit = false;
            }
            kind_of_orb.push_back((uint8_t)kd);
            base_of_orb.push_back(nextpos);
            rep_of_orb.push_back((uint32_t)r);
            nextpos += (uint32_t)nm;
        }
        if (orbit && !kind_mask.empty() && __builtin_popcountll(kind_mask[0]) == 1) {
            for (int a = 0; a < n_trans; ++a)
                if (kidx[(size_t)a] != (uint8_t)a) orbit = false;     // kind 0: position inside the orbit = the group element
        } else if (orbit && !kind_mask.empty()) {
            orbit = false;                                 // no orbit with a trivial stabiliser came first and none was reserved
        }
        n_orb = (int64_t)base_of_orb.size();
        n_kinds = (int)kind_mask.size();
        if (orbit) {
            ucfg_o.assign((size_t)cu, 0);
            oid.assign((size_t)cu, 0);
            oek.assign((size_t)cu, 0);
            tpar.assign((size_t)cu, 0);
            usgn.assign((size_t)cu, 0);
            for (int64_t r = 0; r < cu; ++r) {
                const uint32_t pp = opos[(size_t)r];
                const int32_t o = orb_of[(size_t)r];
                ucfg_o[pp] = ucfg[(size_t)r];
                oid[pp] = (uint32_t)o;
                oek[pp] = (uint16_t)(elem[(size_t)r] | (kind_of_orb[(size_t)o] << 6));
                uint64_t tp = 0;
                for (int g = 0; g < n_trans; ++g) tp |= (uint64_t)(prank[(size_t)g * cu + r] >> 31) << g;
                tpar[pp] = tp;
            }
            // down hops: the translated pattern sits at  p - kidx[kind][e] + kidx[kind][comp[g][e]]
            for (int64_t r = 0; r < cu && orbit; ++r) {
                const uint32_t pp = opos[(size_t)r];
                const int e = oek[pp] & 63, kd = oek[pp] >> 6;
                for (int g = 0; g < n_trans; ++g) {
                    const uint32_t want = opos[(size_t)(prank[(size_t)g * cu + r] & 0x7FFFFFFFu)];
                    const uint32_t got = pp - kidx[(size_t)kd * 64 + e] + kidx[(size_t)kd * 64 + gcomp[(size_t)g * 64 + e]];
                    if (want != got) { orbit = false; break; }
                }
            }
        }
        // up hops: the slots of an orbit are the allowed terms of its smallest member, in term order
        if (orbit) {
            std::vector<std::vector<uint64_t>> slots((size_t)n_orb);
            std::vector<std::vector<int>> slot_term((size_t)n_orb);
            for (int64_t o = 0; o < n_orb && orbit; ++o) {
                const uint32_t u0 = ucfg[(size_t)rep_of_orb[(size_t)o]];
                for (int t = 0; t < R.n_terms; ++t) {
                    const int ti = R.ti[t], tj = R.tj[t];
                    if (ti == tj || R.aup[t][0] * R.aup[t][0] < 1e-28) continue;
                    if (!((u0 >> ti) & 1u) || ((u0 >> tj) & 1u)) continue;
                    const uint32_t v = u0 ^ (1u << ti) ^ (1u << tj);
                    const int64_t rv = (int64_t)(std::lower_bound(ucfg.begin(), ucfg.end(), v) - ucfg.begin());
                    const int32_t o2 = orb_of[(size_t)rv];
                    size_t code = std::find(odict.begin(), odict.end(), R.aup[t][0]) - odict.begin();
                    if (code == odict.size()) {
                        if (odict.size() >= 255) { orbit = false; break; }
                        odict.push_back(R.aup[t][0]);
                    }
                    slots[(size_t)o].push_back((uint64_t)base_of_orb[(size_t)o2] | ((uint64_t)elem[(size_t)rv] << 24) | ((uint64_t)code << 32) |
                                               ((uint64_t)kind_of_orb[(size_t)o2] << 40) | (1ULL << 63));
                    slot_term[(size_t)o].push_back(t);
                }
                w_orb = std::max(w_orb, (int)slots[(size_t)o].size());
            }
            if (w_orb > 64) orbit = false;
            if (orbit) {
                utab.assign((size_t)std::max(w_orb, 1) * (size_t)n_orb, 0u);
                uext.assign((size_t)std::max(w_orb, 1) * (size_t)n_orb, 0);
                for (int64_t o = 0; o < n_orb; ++o)
                    for (size_t k = 0; k < slots[(size_t)o].size(); ++k) {
                        const uint64_t en = slots[(size_t)o][k];
                        const uint32_t code = (uint32_t)((en >> 32) & 255u), kd2 = (uint32_t)((en >> 40) & 63u);
                        const bool ext = code != 0 || kd2 != 0;
                        utab[k * (size_t)n_orb + (size_t)o] = (uint32_t)(en & 0x3FFFFFFFu) | (ext ? 1u << 30 : 0u) | (1u << 31);
                        uext[k * (size_t)n_orb + (size_t)o] = (uint16_t)(code | (kd2 << 8));
                    }
            }
            // every member: the image of slot k is an allowed term of the same amplitude, lands where the table says, and the
            // member has no other hop
            for (int64_t r = 0; r < cu && orbit; ++r) {
                const uint32_t pp = opos[(size_t)r], u = ucfg[(size_t)r];
                const int32_t o = orb_of[(size_t)r];
                const int e = oek[pp] & 63;
                uint64_t sg = 0;
                if (slots[(size_t)o].size() != uprow[(size_t)r].size()) { orbit = false; break; }
                for (size_t k = 0; k < slots[(size_t)o].size() && orbit; ++k) {
                    const int t = slot_term[(size_t)o][k];
                    const int i2 = perms[(size_t)e * n_sites + R.ti[t]], j2 = perms[(size_t)e * n_sites + R.tj[t]];
                    const auto f = tmap.find({i2, j2});
                    if (f == tmap.end() || f->second[0] != R.aup[t][0] || !((u >> i2) & 1u) || ((u >> j2) & 1u)) { orbit = false; break; }
                    const uint32_t v = u ^ (1u << i2) ^ (1u << j2);
                    const int64_t rv = (int64_t)(std::lower_bound(ucfg.begin(), ucfg.end(), v) - ucfg.begin());
                    const uint64_t ent = slots[(size_t)o][k];
                    const uint32_t got = (uint32_t)(ent & 0xFFFFFFu) +
                                         kidx[(size_t)((ent >> 40) & 63) * 64 + gcomp[(size_t)e * 64 + (size_t)((ent >> 24) & 63)]];
                    if (opos[(size_t)rv] != got) { orbit = false; break; }
                    if (between_par(u, i2, j2)) sg |= 1ULL << k;
                }
                usgn[pp] = sg;
            }
        }
    }
    // canonical down patterns, their stabilisers, the rows of every block
    struct HostBlock { uint32_t d; std::vector<int> stab; int64_t nrows, row0; };
    std::vector<HostBlock> hb;
    for (uint32_t d : dcfg) {
        bool canon = true;
        std::vector<int> stab;
        for (int g = 1; g < n_trans && canon; ++g) {
            const uint32_t im = image(g, d);
            if (im < d) canon = false;
            else if (im == d) stab.push_back(g);
        }
        if (!canon) continue;
        HostBlock b{d, stab, 0, 0};
        if (stab.empty()) {
            b.nrows = cu;
        } else {
            for (int64_t r = 0; r < cu; ++r) {
                bool rep = true;
                for (int g : stab)
                    if (uimg[(size_t)g * cu + r] < ucfg[(size_t)r]) {
                        rep = false;
                        break;
                    }
                b.nrows += rep ? 1 : 0;
            }
        }
        hb.push_back(b);
    }
    int64_t dim = 0;
    for (auto &b : hb) {
        b.row0 = dim;
        dim += b.nrows;
    }
    if (dim <= 0 || dim >= 2147483647LL) {
        set_error("%s: sector dimension %lld out of range", who, (long long)dim);
        return QBH_EUNSUPP;
    }
    const int64_t n_blocks = (int64_t)hb.size();
    auto block_of = [&](uint32_t d) {
        int64_t lo = 0, hi = n_blocks;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (hb[(size_t)mid].d < d) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    std::vector<MfSecBlock> blk((size_t)n_blocks);
    std::vector<MfSecHop> hops;
    std::vector<uint64_t> flags((size_t)n_blocks * 8, 0ULL);
    std::vector<int64_t> items;
    bool all_real = true;
    for (int64_t bi = 0; bi < n_blocks; ++bi) {
        const HostBlock &b = hb[(size_t)bi];
        MfSecBlock &B = blk[(size_t)bi];
        B.row0 = b.row0;
        B.d = b.d;
        B.nrows = (int32_t)b.nrows;
        B.regular = b.stab.empty() ? 1 : 0;
        B.hop0 = (int32_t)hops.size();
        B.nhop = 0;
        for (int64_t tl = 0; tl * sec_tile < b.nrows; ++tl) items.push_back((bi << 20) | tl);
        if (!B.regular) continue;
        std::map<std::pair<int64_t, int>, std::pair<double, double>> acc;     // (target row0, g) -> coefficient
        for (int t = 0; t < R.n_terms; ++t) {
            const int ti = R.ti[t], tj = R.tj[t];
            const double ar = R.adn[t][0], ai = R.adn[t][1];
            if (ti == tj || (ar == 0.0 && ai == 0.0)) continue;
            if (!((b.d >> ti) & 1u) || ((b.d >> tj) & 1u)) continue;
            const uint32_t d2p = b.d ^ (1u << ti) ^ (1u << tj);
            uint32_t best = d2p;
            int gb = 0;
            for (int g = 1; g < n_trans; ++g) {
                const uint32_t im = image(g, d2p);
                if (im < best) {
                    best = im;
                    gb = g;
                }
            }
            const int64_t tb = block_of(best);
            if (!hb[(size_t)tb].stab.empty()) {             // stabilised target: the entry goes to the stored remainder
                flags[(size_t)bi * 8 + (size_t)(t >> 6)] |= 1ULL << (t & 63);
                continue;
            }
            const double sg = ((between_par(b.d, ti, tj) ^ (gb ? parity(gb, d2p) : 0)) ? -1.0 : 1.0);
            const double cr = chars[2 * gb], cim = -chars[2 * gb + 1];                 // conj(chi(g*))
            auto &c = acc[{hb[(size_t)tb].row0, gb}];
            c.first += sg * (ar * cr - ai * cim);
            c.second += sg * (ar * cim + ai * cr);
        }
        for (const auto &e : acc) {
            if (e.second.first * e.second.first + e.second.second * e.second.second < 1e-28) continue;
            hops.push_back(MfSecHop{e.first.first, e.first.second, 0, e.second.first, e.second.second});
            if (e.second.second != 0.0) all_real = false;
            B.nhop++;
        }
    }
    if (hb.size() >= (1u << 20) * 2048ULL) {
        set_error("%s: too many blocks", who);
        return QBH_EUNSUPP;
    }

    // ---- device: representatives (for the remainder), tables, remainder CSR
    std::vector<void *> pool;
    uint64_t *d_flags = nullptr;
    MfSec *ms = new MfSec();
    auto drop_tables = [&]() {
        for (void *q : {(void *)ms->blk, (void *)ms->hop, (void *)ms->item, (void *)ms->ucfg, (void *)ms->upell, (void *)ms->prank,
                        (void *)ms->oid, (void *)ms->oek, (void *)ms->tpar, (void *)ms->usgn, (void *)ms->utab, (void *)ms->uext})
            if (q) (void)hipFree(q);
        delete ms;
    };
    SectorDev<HubReprDev> S;
    int rc = sector_enumerate(R, tab, pool, S, who);
    if (rc == QBH_OK && S.dim != dim) {
        set_error("%s: block table (%lld rows) and enumeration (%lld representatives) disagree", who, (long long)dim, (long long)S.dim);
        rc = QBH_EHIP;
    }
    int32_t *d_cnt = nullptr, *d_flg = nullptr;
    int64_t *d_ia = nullptr, *d_pos = nullptr;
    int64_t nnz = 0, n_rrows = 0;
    hipError_t e = hipSuccess;
    auto up = [&](auto **dst, const auto &h) {
        using T = typename std::remove_reference<decltype(h)>::type::value_type;
        if (e != hipSuccess || rc != QBH_OK) return;
        e = qbh::dev_alloc((void **)dst, std::max<size_t>(h.size(), 1) * sizeof(T));
        if (e == hipSuccess && !h.empty()) e = hipMemcpy(*dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    };
    up(&ms->blk, blk);
    up(&ms->hop, hops);
    up(&ms->item, items);
    uint32_t *d_opos = nullptr;                      // old rank -> position: for the remainder's indices and the vector map
    if (orbit) {
        up(&ms->ucfg, ucfg_o);
        up(&ms->oid, oid);
        up(&ms->oek, oek);
        up(&ms->tpar, tpar);
        up(&ms->usgn, usgn);
        up(&ms->utab, utab);
        up(&ms->uext, uext);
        up(&d_opos, opos);
    } else {
        up(&ms->ucfg, ucfg);
        up(&ms->upell, upell);
        up(&ms->prank, prank);
    }
    up(&d_flags, flags);
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&d_cnt, (size_t)dim * sizeof(int32_t));
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&d_flg, (size_t)dim * sizeof(int32_t));
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&d_ia, (size_t)(dim + 1) * sizeof(int64_t));
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&d_pos, (size_t)(dim + 1) * sizeof(int64_t));
    const int rgrid = (int)std::min<int64_t>((dim + 127) / 128, 256 * 16);
    if (rc == QBH_OK && e == hipSuccess) {
        hipLaunchKernelGGL(k_secrem_count, dim3(rgrid), dim3(128), 0, 0, S.R, S.tab, S.reps, S.info, dim, ms->blk, n_blocks, d_flags, d_cnt);
        hipLaunchKernelGGL(k_secrem_flag, dim3(blas_grid(dim)), dim3(256), 0, 0, d_cnt, dim, d_flg);
        e = hipGetLastError();
    }
    if (rc == QBH_OK && e == hipSuccess) rc = exclusive_scan(d_cnt, dim, d_ia, 0);
    if (rc == QBH_OK && e == hipSuccess) rc = exclusive_scan(d_flg, dim, d_pos, 0);
    if (rc == QBH_OK && e == hipSuccess) e = hipMemcpy(&nnz, d_ia + dim, sizeof(int64_t), hipMemcpyDeviceToHost);
    if (rc == QBH_OK && e == hipSuccess) e = hipMemcpy(&n_rrows, d_pos + dim, sizeof(int64_t), hipMemcpyDeviceToHost);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_flg) (void)hipFree(d_flg);
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&ms->rrow, (size_t)std::max<int64_t>(n_rrows, 1) * sizeof(int32_t));
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&ms->ria, (size_t)(n_rrows + 1) * sizeof(int64_t));
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&ms->rja, (size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t));
    if (rc == QBH_OK && e == hipSuccess) e = qbh::dev_alloc(&ms->rval, (size_t)std::max<int64_t>(nnz, 1) * sizeof(d2));
    if (rc == QBH_OK && e == hipSuccess) {
        hipLaunchKernelGGL(k_secrem_fill, dim3(rgrid), dim3(128), 0, 0, S.R, S.tab, S.reps, S.info, dim, ms->blk, n_blocks, d_flags, d_ia, d_pos,
                           ms->rrow, ms->ria, ms->rja, ms->rval);
        e = hipGetLastError();
    }
    uint32_t *d_vmap = nullptr;                      // caller's row -> internal row (the handle's basis map)
    if (rc == QBH_OK && e == hipSuccess && orbit) {
        // the remainder was generated with the rows and columns of the ascending order: move both to the positions
        hipLaunchKernelGGL(k_sec_orbit_remap, dim3(blas_grid(std::max<int64_t>(nnz, n_rrows))), dim3(256), 0, 0, ms->blk, n_blocks, d_opos,
                           ms->rrow, n_rrows, ms->rja, nnz);
        e = hipGetLastError();
        if (e == hipSuccess) e = qbh::dev_alloc(&d_vmap, (size_t)dim * sizeof(uint32_t));
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_sec_orbit_map, dim3((unsigned)std::min<int64_t>((int64_t)items.size(), 1 << 20)), dim3(256), 0, 0, ms->blk,
                               ms->item, (int64_t)items.size(), d_opos, d_vmap, sec_tile);
            e = hipGetLastError();
        }
    }
    if (rc == QBH_OK && e == hipSuccess) e = hipDeviceSynchronize();
    free_pool(pool);
    for (void *q : {(void *)d_flags, (void *)d_ia, (void *)d_pos, (void *)d_opos})
        if (q) (void)hipFree(q);
    auto drop_all = [&]() {
        for (void *q : {(void *)ms->rrow, (void *)ms->ria, (void *)ms->rja, (void *)ms->rval, (void *)d_vmap})
            if (q) (void)hipFree(q);
        drop_tables();
    };
    if (rc != QBH_OK || e != hipSuccess) {
        drop_all();
        if (rc != QBH_OK) return rc;
        set_error("%s: %s", who, hipGetErrorString(e));
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? QBH_ENOMEM : QBH_EHIP;
    }
    ms->n_sites = n_sites;
    ms->n_up = n_up;
    ms->n_dn = n_dn;
    ms->n_trans = n_trans;
    ms->w_up = w_up;
    ms->n_pairs = n_pairs;
    ms->dim = dim;
    ms->cu = cu;
    ms->n_blocks = n_blocks;
    ms->n_items = (int64_t)items.size();
    ms->tile = sec_tile;
    ms->U = U;
    ms->n_rrows = n_rrows;
    ms->rnnz = nnz;
    for (size_t c = 0; c < updict.size(); ++c) ms->updict[c] = updict[c];
    if (orbit) {
        ms->orbit = 1;
        ms->w_orb = w_orb;
        ms->n_kinds = n_kinds;
        ms->n_orb = n_orb;
        for (size_t c = 0; c < 256; ++c) ms->updict[c] = c < odict.size() ? odict[c] : 0.0;
        std::copy(gcomp.begin(), gcomp.end(), ms->comp);
        std::copy(kidx.begin(), kidx.end(), ms->kidx);
    }
    for (int t = 0; t < R.n_terms; ++t)
        if (R.ti[t] == R.tj[t]) {
            ms->nup[(int)R.ti[t]] += R.aup[t][0];
            ms->ndn[(int)R.ti[t]] += R.adn[t][0];
            if (R.aup[t][0] != 0.0 || R.adn[t][0] != 0.0) ms->has_number_terms = true;
        }
    for (int p = 0; p < n_pairs; ++p) {
        ms->pi[p] = R.pi[p];
        ms->pj[p] = R.pj[p];
        for (int c = 0; c < 4; ++c) ms->pv[p][c] = R.pv[p][c];
    }
    // real operator: real hop coefficients and a real remainder
    if (all_real && nnz > 0) {
        double *tmp = nullptr;
        std::vector<double> hp((size_t)blas_grid(nnz));
        if (qbh::dev_alloc(&tmp, (size_t)kMaxRedBlocks * sizeof(double)) == hipSuccess) {
            if (launch_imag_norm(ms->rval, nnz, tmp, 0) == QBH_OK &&
                hipMemcpy(hp.data(), tmp, hp.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess) {
                double sum = 0.0;
                for (double v : hp) sum += v;
                all_real = sum == 0.0;
            } else {
                all_real = false;
            }
            (void)hipFree(tmp);
        } else {
            all_real = false;
        }
    }
    ms->all_real = all_real;
    if ((int)hops.size() > 0) {
        int mx = 0;
        for (const auto &bq : blk) mx = std::max(mx, (int)bq.nhop);
        if (mx > kSecMaxHops) {
            drop_all();
            set_error("%s: more than %d down hops per block", who, kSecMaxHops);
            return QBH_EUNSUPP;
        }
    }
    MfSec *d_ms = nullptr;
    if (qbh::dev_alloc(&d_ms, sizeof(MfSec)) != hipSuccess || hipMemcpy(d_ms, ms, sizeof(MfSec), hipMemcpyHostToDevice) != hipSuccess) {
        if (d_ms) (void)hipFree(d_ms);
        drop_all();
        set_error("%s: could not place the operator tables", who);
        return QBH_ENOMEM;
    }
    // nnz the stored CSR of the same sector would hold (~ one entry per allowed hop): for the byte accounting only
    const int64_t nnz_equiv = nnz + (int64_t)((double)dim * (double)(1 + w_up));
    rc = adopt_mf_sector(out, ms, d_ms, dim, nnz_equiv, opts);
    if (rc != QBH_OK) {
        (void)hipFree(d_ms);
        drop_all();
        return rc;
    }
    if (orbit) {                                     // device vectors of this handle are in the orbit order; the seams translate
        (*out)->basis.kind = QBH_BASIS_SECTOR_ORBIT;
        (*out)->basis.d_map = d_vmap;
    }
    if (dim_out) *dim_out = dim;
    return QBH_OK;
}
