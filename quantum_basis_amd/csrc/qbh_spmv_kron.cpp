// qbh_spmv_kron.cpp -- spmv_kron: the SpMV of an operator split in place (kron_build), as a sequence of steps: the walk, the
// tiled x, the exchange under a communicator (whole gather, gather in band ranges, personalised sparse exchange), the
// arguments of the far / near / cross passes, and the passes themselves on one GPU and under a communicator.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "qbh_api_priv.hpp"

using qbh::d2;
using namespace qbhapi;

namespace {

typedef qbh_csr::KronSplit KronSplit;

struct KronCall {            // one split SpMV: its arguments and what it decides before the first launch
    qbh_csr  *A;
    const d2 *x, *xl;        // the caller's x and the rank's own block of it
    d2       *y;
    double    alpha, beta, gamma;
    double   *red;
    int       walk;          // how both passes walk their blocks (SpmvArgs::swizzle)
    // under a communicator: the wire format of this solve (8-byte real parts when the drivers agreed on it), and whether the
    // gather travels in parts (with real parts only through the hook that names the format)
    int       realw;
    bool      sparse;        // personalised exchange: only what each peer reads travels
    int       parts;         // band ranges the exchange travels in
    bool      async_gather;
    int64_t   nfb, w_edge;   // full bands of the minor index, width of the narrow edge band behind them
};

#ifdef QBH_XCD_TIMING
int xcd_timing_seed(qbh_csr *A)      // slot 2 of every XCD collects a minimum
{
    unsigned long long h[3 * 128] = {0};
    for (int p = 0; p < 3; ++p)
        for (int k = 0; k < 8; ++k) h[p * 128 + k * 16 + 2] = ~0ull;
    QBH_HIP(hipMemcpyAsync(A->d_wctr, h, sizeof(h), hipMemcpyHostToDevice, A->stream));
    QBH_HIP(hipStreamSynchronize(A->stream));
    return QBH_OK;
}

// debug build: last and first wavefront of every XCD to run out of blocks, relative to the earliest of the pass (100 MHz ticks -> us)
int xcd_timing_dump(qbh_csr *A)
{
    unsigned long long h[3 * 128];
    QBH_HIP(hipStreamSynchronize(A->stream));
    QBH_HIP(hipMemcpy(h, A->d_wctr, sizeof(h), hipMemcpyDeviceToHost));
    for (int pass = 1; pass <= 2; ++pass) {
        const unsigned long long *d = h + pass * 128;
        unsigned long long lo = ~0ull, hi = 0;
        for (int k = 0; k < 8; ++k) {
            lo = std::min(lo, d[k * 16 + 2]);
            hi = std::max(hi, d[k * 16 + 1]);
        }
        fprintf(stderr, "[xcd timing] %s pass: last wavefront of each XCD done at (us before the pass ends):", pass == 1 ? "far" : "near");
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %.0f", (double)(hi - d[k * 16 + 1]) * 0.01);
        fprintf(stderr, " | first wavefront anywhere idle %.0f us before the end\n", (double)(hi - lo) * 0.01);
    }
    return QBH_OK;
}
#endif

#ifdef QBH_WAVE_TIMING
// debug build: where the wavefronts of the two passes spend their cycles (s_memtime ticks, 100 MHz)
int wave_timing_dump(qbh_csr *A)
{
    unsigned long long h[3 * 128];
    QBH_HIP(hipStreamSynchronize(A->stream));
    QBH_HIP(hipMemcpy(h, A->d_wctr, sizeof(h), hipMemcpyDeviceToHost));
    for (int pass = 1; pass <= 2; ++pass) {
        const unsigned long long *d = h + (pass + 1) * 128 - 8;
        const double nb = d[4] ? (double)d[4] : 1.0;
        fprintf(stderr, "[wave timing] %s pass: blocks %llu, ticks per block: issue+column wait %.1f, gather wait %.1f, reduce %.1f, stream rest %.1f\n",
                pass == 1 ? "far" : "near", d[4], d[0] / nb, d[1] / nb, d[2] / nb, d[3] / nb);
    }
    return QBH_OK;
}
#endif

// the dynamic ordered walk per XCD -- also for a caller who wants bit-reproducible results: y does not depend on which wavefront
// computes a row, and the fused reductions are collected per CHUNK of blocks and added in a fixed order (k_spmv_wave2's
// CHUNKRED, k_reduce_chunks) since round 5; qbh_opts.wave_walk = 2 still names the static walk
int choose_walk(qbh_csr *A, int *walk)
{
    const KronSplit &K = A->kron;
    *walk = A->opts.wave_walk >= 0 ? A->opts.wave_walk : 3;
    if (*walk != 3) return QBH_OK;
    if (!A->d_wctr) {
        *walk = 2;
        return QBH_OK;
    }
    const int regions = A->has_comm && (K.n_parts > 1 || K.sparse) ? qbh::kWctrRegions : 3;
    QBH_HIP(hipMemsetAsync(A->d_wctr, 0, (size_t)regions * 128 * sizeof(unsigned long long), A->stream));
#ifdef QBH_XCD_TIMING
    QBH_TRY(xcd_timing_seed(A));
#endif
    return QBH_OK;
}

int ensure_tiled_x(const KronCall &c)    // first use: the tiled copy of the full-length x
{
    qbh_csr *A = c.A;
    KronSplit &K = A->kron;
    if (K.xt_cap >= A->ncols) return QBH_OK;
    if (K.d_xt) (void)hipFree(K.d_xt);
    K.d_xt = nullptr;
    K.xt_cap = 0;
    QBH_HIP(qbh::dev_alloc(&K.d_xt, (size_t)A->ncols * sizeof(d2)));
    K.xt_cap = A->ncols;
    if (A->dbg.print_ptrs) fprintf(stderr, "qbhip kron xt %p x %p y %p\n", (void *)K.d_xt, (const void *)c.x, (void *)c.y);
    K.xt_of = nullptr;
    return QBH_OK;
}

// part k of the exchange = bands [pb0, pb1) of every piece, the last part takes the narrow edge band along
void part_bands(const KronCall &c, int k, int64_t *pb0, int64_t *pb1, bool *with_edge)
{
    const KronSplit &K = c.A->kron;
    *pb0 = c.parts > 1 ? K.part_band[k] : 0;
    *pb1 = c.parts > 1 ? K.part_band[k + 1] : c.nfb;
    *with_edge = k == c.parts - 1 && c.w_edge > 0;
}

// what every move into the tiled x shares: the geometry, the ranks' cuts, and the list of the major indices this shard reads
qbh::KronPlace place_common(const KronCall &c, const d2 *src)
{
    const KronSplit &K = c.A->kron;
    qbh::KronPlace p{};
    p.real = c.realw;
    p.src = src;
    p.dst = K.d_xt;
    p.nr = c.A->comm.nranks;
    p.B = K.t.B;
    p.S = K.t.S;
    p.NUg = K.NUg;
    p.nfb = c.nfb;
    for (int q = 0; q <= p.nr; ++q) p.cu[q] = K.rank_cu[q];
    p.list = K.d_need;
    return p;
}

// sparse exchange: where every peer's packed piece begins in d_vrecv (the own rank sends itself nothing)
void recv_bases(const qbh_csr *A, int64_t *base)
{
    const KronSplit &K = A->kron;
    int64_t rbase = 0;
    for (int q = 0; q < A->comm.nranks; ++q) {
        base[q] = rbase;
        if (q != A->comm.rank) rbase += (K.need_lo[q + 1] - K.need_lo[q]) * K.t.S;
    }
}

int gather_started(int hrc)
{
    if (hrc == 0) return QBH_OK;
    qbh::set_error("allgather hook failed");
    return QBH_ECOMM;
}

int gather_whole(const KronCall &c)
{
    const qbh_comm &cm = c.A->comm;
    return gather_started(c.async_gather ? cm.allgather_begin(cm.ctx, c.realw) : cm.allgather_x(cm.ctx, c.realw));
}

int gather_in_parts(const KronCall &c)   // band ranges one after another: the far pass follows them (far_after_gather)
{
    const qbh_comm &cm = c.A->comm;
    int hrc = 0;
    for (int k = 0; k < c.parts && hrc == 0; ++k) {
        const int64_t *ol = c.A->kron.part_off_len.data() + (size_t)k * 2 * (size_t)cm.nranks;
        hrc = c.realw ? cm.allgather_part_begin_w(cm.ctx, k, c.parts, ol, 1) : cm.allgather_part_begin(cm.ctx, k, c.parts, ol);
    }
    return gather_started(hrc);
}

// (1) the rank's own needed major indices straight from its tiled block into the tiled x
int sparse_place_own(const KronCall &c, const d2 *send)
{
    const KronSplit &K = c.A->kron;
    const int me = c.A->comm.rank;
    qbh::KronPlace po = place_common(c, send);
    for (int q = 0; q <= po.nr; ++q) po.lo[q] = q <= me ? K.need_lo[me] : K.need_lo[me + 1];     // only the own rank has entries
    po.band0 = 0;
    po.band1 = c.nfb + (c.w_edge > 0 ? 1 : 0);
    return qbh::launch_kron_place(po, c.A->stream);
}

// (2) per destination: the major indices it reads, packed band-major
int sparse_pack(const KronCall &c, const d2 *send)
{
    const KronSplit &K = c.A->kron;
    qbh::KronPack pk{};
    pk.src = send;
    pk.dst = K.d_vsend;
    pk.real = c.realw;
    pk.nr = c.A->comm.nranks;
    pk.B = K.t.B;
    pk.S = K.t.S;
    pk.NUq = K.t.NU;
    pk.nfb = c.nfb;
    pk.list = K.d_send_list;
    for (int q = 0; q <= pk.nr; ++q) pk.lo[q] = K.send_lo[q];
    for (int q = 0; q < pk.nr; ++q) pk.base[q] = K.send_lo[q] * K.t.S;
    return qbh::launch_kron_pack(pk, c.A->stream);
}

// (3) the pieces, band range after band range
int sparse_exchange(const KronCall &c)
{
    const KronSplit &K = c.A->kron;
    const qbh_comm &cm = c.A->comm;
    const int npk = cm.nranks, me = cm.rank;
    std::vector<int64_t> so((size_t)2 * npk), ro((size_t)2 * npk), rb((size_t)npk, 0);
    recv_bases(c.A, rb.data());
    int hrc = 0;
    for (int k = 0; k < c.parts && hrc == 0; ++k) {
        int64_t pb0, pb1;
        bool with_edge;
        part_bands(c, k, &pb0, &pb1, &with_edge);
        for (int q = 0; q < npk; ++q) {
            const int64_t ns = q == me ? 0 : K.send_lo[q + 1] - K.send_lo[q], nr_ = q == me ? 0 : K.need_lo[q + 1] - K.need_lo[q];
            so[(size_t)2 * q] = K.send_lo[q] * K.t.S + pb0 * K.t.B * ns;
            so[(size_t)2 * q + 1] = (pb1 - pb0) * K.t.B * ns + (with_edge ? ns * c.w_edge : 0);
            ro[(size_t)2 * q] = rb[(size_t)q] + pb0 * K.t.B * nr_;
            ro[(size_t)2 * q + 1] = (pb1 - pb0) * K.t.B * nr_ + (with_edge ? nr_ * c.w_edge : 0);
        }
        hrc = cm.exchange_v(cm.ctx, k, c.parts, so.data(), ro.data(), c.realw ? 1 : 2, K.d_vsend, K.d_vrecv);
    }
    return gather_started(hrc);
}

// every rank sends the TILED copy of its own block (made here unless the pass that produced x wrote it)
int start_exchange(KronCall &c)
{
    qbh_csr *A = c.A;
    KronSplit &K = A->kron;
    d2 *send = reinterpret_cast<d2 *>(A->comm.d_xsend);
    if (K.xt_of != (const void *)c.x) QBH_TRY(qbh::launch_kron_tile(c.x, send, A->nrows, K.t, A->stream, c.realw, A->d_flag));
    K.xt_of = nullptr;
    c.async_gather = A->comm.allgather_begin && A->comm.allgather_wait;
    if (c.sparse) {
        QBH_TRY(sparse_place_own(c, send));
        QBH_TRY(sparse_pack(c, send));
        QBH_TRY(sparse_exchange(c));
    } else {
        QBH_TRY(c.parts > 1 ? gather_in_parts(c) : gather_whole(c));
    }
    A->stats.n_gather++;
    A->wire_bytes_last = c.realw ? 8 : 16;
    return QBH_OK;
}

// the pieces of the gathered blocks -> their place in the tiled x (part k of c.parts, or everything)
int place(const KronCall &c, int k)
{
    const qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    int64_t pb0, pb1;
    bool with_edge;
    part_bands(c, k, &pb0, &pb1, &with_edge);
    const d2 *gathered = c.realw ? reinterpret_cast<const d2 *>(A->comm.d_xfull_r) : reinterpret_cast<const d2 *>(A->comm.d_xfull);
    qbh::KronPlace pa = place_common(c, c.sparse ? K.d_vrecv : gathered);
    for (int q = 0; q <= pa.nr; ++q) pa.lo[q] = K.need_lo[q];
    pa.band0 = pb0;
    pa.band1 = pb1 + (with_edge ? 1 : 0);                    // the narrow last band travels with the last piece
    if (c.sparse) {                                          // the peers' packed pieces: only the listed major indices, compact
        pa.compact = 1;
        // the list keeps the own rank's entries in the middle: the peers' ranges are named one by one, the own range is empty
        recv_bases(A, pa.base);
        pa.skip = A->comm.rank;
        return qbh::launch_kron_place(pa, A->stream);
    }
    for (int q = 0; q < pa.nr; ++q) {
        pa.base[q] = A->comm.row_cuts ? A->comm.row_cuts[q] : (int64_t)q * A->comm.nblk;
        if (c.parts > 1) {
            pa.off[q] = K.part_off_len[((size_t)k * (size_t)pa.nr + (size_t)q) * 2];
            pa.len[q] = K.part_off_len[((size_t)k * (size_t)pa.nr + (size_t)q) * 2 + 1];
        } else {
            pa.off[q] = 0;
            pa.len[q] = (K.rank_cu[q + 1] - K.rank_cu[q]) * K.t.S;
        }
    }
    return qbh::launch_kron_place(pa, A->stream);
}

qbh::SpmvArgs far_args(const KronCall &c)
{
    const qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    qbh::SpmvArgs f{};
    f.ia = K.ia_f;
    f.ja = K.ja_f;
    f.ja16 = K.c16_f;
    f.ja8 = K.c8_f;
    f.val8 = K.v8_f;
    f.kS = K.t.S;
    f.kNU = K.NUg;
    f.kB = K.t.B;
    f.val = K.val_f;
    f.wd = K.wd_f;
    f.n_wb = K.nwb_f;
    f.nrows = K.map.nfar_rows();                             // sliced: whole groups of the full bands
    f.xg = K.d_xt;                                           // what the far pass gathers from: the tiled copy of the WHOLE x
    f.xl = c.xl;
    f.y = K.d_far;
    f.alpha = 1.0;
    f.colmask = -1;
    f.chunk_mult = A->chunk_mult;
    f.swizzle = c.walk == 3 ? 3 : 1;        // one contiguous eighth of the bands per XCD: a band of x stays in that XCD's L2
    f.wctr = A->d_wctr ? A->d_wctr + 128 : nullptr;
    return f;
}

int near_args(const KronCall &c, qbh::SpmvArgs *out)
{
    const qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    qbh::SpmvArgs nr{};
    nr.ia = K.ia_n;
    nr.ja = K.ja_n;
    nr.ja16 = K.c16_n;
    nr.len8 = K.len_n;                                       // one class only (kron_near_lens): pass forms 1 and 2
    if (K.vp_n && K.c16_n) {                                 // the values once per pattern of S rows (kron_near_vals): only beside the 2-byte columns
        nr.valp = K.vp_n;
        nr.diag = K.dg_n;
        nr.dpos8 = K.dp_n;
        nr.kK = K.pat_n;
    }
    nr.val = K.val_n;
    nr.wd = K.wd_n;
    nr.n_wb = K.nwb_n;
    nr.nrows = A->nrows;
    nr.xg = K.c16_n ? c.xl : c.xl - A->row_offset;           // near columns are global indices of locally-owned elements (2-byte: relative to the shard)
    nr.xl = c.xl;
    nr.y = c.y;
    nr.alpha = c.alpha;
    nr.beta = c.beta;
    nr.gamma = c.gamma;
    nr.colmask = -1;
    nr.chunk_mult = A->chunk_mult;
    nr.kS = K.t.S;
    nr.kNU = K.t.NU;
    nr.kB = K.t.B;
    nr.swizzle = c.walk;
    nr.wctr = A->d_wctr ? A->d_wctr + 256 : nullptr;
    nr.chunk_red = K.d_chunk_red;                            // dynamic walk: the near pass's reduction partials, one slot per chunk
    nr.yin = A->ovr_yin;                                     // pipelined three-term step (lanczos_core): out of place, coefficients on the device
    nr.coef = A->ovr_coef;
    nr.coef_mode = A->ovr_coef ? 1 : 0;
    if (c.walk == 3 && !K.d_chunk_red) {
        qbh::set_error("Kronecker split: the chunk partials of the near pass were not allocated");
        return QBH_EHIP;
    }
    *out = nr;
    return QBH_OK;
}

// several classes, third pass: the unstructured part, accumulating onto y; reductions on the finished y
qbh::SpmvArgs cross_args(const KronCall &c)
{
    const qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    qbh::SpmvArgs cr{};
    cr.ia = K.ia_x;
    cr.ja = K.ja_x;
    cr.val = K.val_x;
    cr.wd = K.wd_x;
    cr.n_wb = K.nwb_x;
    cr.nrows = A->nrows;
    cr.xg = K.d_xt;                  // columns are stored in the tiled order of x
    cr.xl = c.xl;
    cr.y = c.y;
    cr.alpha = c.alpha;
    cr.beta = 1.0;
    cr.gamma = 0.0;
    cr.coef = A->ovr_coef;
    cr.coef_mode = A->ovr_coef ? 2 : 0;
    cr.colmask = -1;
    cr.chunk_mult = A->chunk_mult;
    cr.swizzle = (A->opts.xcd_swizzle == 3 && !A->opts.deterministic && A->d_wctr) ? 3 : (A->opts.xcd_swizzle == 3 ? 2 : A->opts.xcd_swizzle);
    cr.wctr = A->d_wctr;
    cr.partials = c.red ? A->d_partials : nullptr;
    return cr;
}

// the near pass's chunk sums -> partial sums (dynamic walk; the static walks write their partials themselves)
int reduce_chunks(const KronCall &c, int *nparts)
{
    const KronSplit &K = c.A->kron;
    if (c.walk != 3) return QBH_OK;
    return qbh::launch_reduce_chunks(K.d_chunk_red, K.n_chunk_slots, c.A->d_partials, nparts, c.A->stream);
}

int near_one_class(const KronCall &c, qbh::SpmvArgs &nr, int *nparts)
{
    qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    // the far entries of the rows that do not fill a band: their sums go into those rows' slots of the far buffer
    QBH_TRY(qbh::launch_kron_cross_rows(K.ia_x, K.xrow, K.n_xrows, K.ja_x, K.val_x, K.d_xt, K.t, K.d_far, A->stream));
    nr.partials = c.red ? A->d_partials : nullptr;
    QBH_TRY(qbh::launch_spmv_wave2(nr, K.tpr_n, 2, K.grid_n, A->stream));
    if (c.red) QBH_TRY(reduce_chunks(c, nparts));
    return QBH_OK;
}

int near_classes(const KronCall &c, qbh::SpmvArgs &nr, int *nparts)
{
    qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    nr.kcls = K.d_cls;
    nr.partials = (c.red && K.nnz_x == 0) ? A->d_partials : nullptr;
    QBH_TRY(qbh::launch_spmv_wave2(nr, K.tpr_n, 4, K.grid_n, A->stream));
    if (K.nnz_x == 0) return c.red ? reduce_chunks(c, nparts) : QBH_OK;
    QBH_TRY(qbh::launch_spmv_wave(cross_args(c), K.tpr_x, K.grid_x, A->stream));
    *nparts = K.grid_x;
    return QBH_OK;
}

// One GPU (or a shard driven with the full-length x): tiled copy of x unless the pass that produced x wrote it, far pass (row
// sums in tiled order), near pass (+ far result, fused epilogue and reductions).
int apply_one_gpu(const KronCall &c, int *nparts)
{
    qbh_csr *A = c.A;
    KronSplit &K = A->kron;
    hipStream_t s = A->stream;
    QBH_TRY(prof_begin(A));
    if (K.xt_of != (const void *)c.x) {
        if (K.map.nc == 1) {
            QBH_TRY(qbh::launch_kron_tile(c.x, K.d_xt, A->ncols, qbh::KronTile{K.t.S, K.NUg, K.t.B}, s));
        } else {                         // every class is a product basis of its own: tiled class by class
            for (int k = 0; k < K.map.nc; ++k)
                QBH_TRY(qbh::launch_kron_tile(c.x + K.map.rbase[k], K.d_xt + K.map.rbase[k], K.map.rbase[k + 1] - K.map.rbase[k],
                                              qbh::KronTile{K.map.S[k], K.map.NU[k], K.map.B}, s));
        }
    }
    K.xt_of = nullptr;
    const qbh::SpmvArgs f = far_args(c);
    qbh::SpmvArgs nr;
    QBH_TRY(near_args(c, &nr));
    if (K.sliced) QBH_TRY(qbh::launch_zero_cut_groups(K.wd_f, K.nwb_f, f.nrows, K.d_far, s));
    QBH_TRY(qbh::launch_spmv_wave2(f, K.tpr_f, K.sliced ? 3 : 0, K.grid_f, s));
    nr.far = K.d_far;
    QBH_TRY(K.map.nc == 1 ? near_one_class(c, nr, nparts) : near_classes(c, nr, nparts));
#ifdef QBH_XCD_TIMING
    QBH_TRY(xcd_timing_dump(A));
#endif
#ifdef QBH_WAVE_TIMING
    QBH_TRY(wave_timing_dump(A));
#endif
    return prof_mark(A, 1);
}

// qbh_opts.comm_reserve: room for RCCL's own kernels beside the persistent passes -- workgroups left out of the grids (multiples
// of 8: one per XCD) and at most two far workgroups per CU (QBH_DEBUG=comm_reserve=W / comm_far_cap=C override both for A/B runs)
void comm_grids(qbh_csr *A, int *grid_n, int *grid_f)
{
    const KronSplit &K = A->kron;
    int reserve = 0, far_cap = K.grid_f;
    if (A->comm.nranks > 1 && A->opts.comm_reserve >= 0) {
        reserve = A->opts.comm_reserve > 0 ? (A->opts.comm_reserve / 8) * 8 : 64;
        far_cap = std::min(K.grid_f, 2 * cu_count(A));
    }
    if (A->dbg.comm_reserve != 0) reserve = A->dbg.comm_reserve > 0 ? (A->dbg.comm_reserve / 8) * 8 : 0;
    if (A->dbg.comm_far_cap != 0) far_cap = A->dbg.comm_far_cap > 0 ? std::min(K.grid_f, A->dbg.comm_far_cap * std::max(A->ncu, 256)) : K.grid_f;
    // (a small shard keeps at least half of either grid; grids stay multiples of 8 -- the static walks count slots per XCD)
    auto mult8 = [](int g) { return std::max(8, (g / 8) * 8); };
    *grid_n = mult8(std::max(K.grid_n / 2, K.grid_n - reserve));
    *grid_f = mult8(std::max(std::min(far_cap, K.grid_f) / 2, far_cap - reserve));
}

// the far pass behind the exchange: of everything once the whole gather is there, or band range by band range
int far_after_gather(const KronCall &c, const qbh::SpmvArgs &f, int grid_f)
{
    qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    hipStream_t s = A->stream;
    if (c.parts == 1 && !c.sparse) {
        if (c.async_gather) QBH_TRY(gather_wait(A, false));
        QBH_TRY(prof_mark(A, 2));
        QBH_TRY(place(c, 0));
        if (K.sliced) QBH_TRY(qbh::launch_zero_cut_groups(K.wd_f, K.nwb_f, f.nrows, K.d_far, s));
        return qbh::launch_spmv_wave2(f, K.tpr_f, K.sliced ? 3 : 0, grid_f, s);
    }
    // every band range of the far part as soon as its piece of the gathered x is there and has been moved to its place; a
    // block that straddles a range boundary belongs to the later range (the pieces complete in order), its cut groups add
    // up through the atomics
    QBH_TRY(qbh::launch_zero_cut_groups(K.wd_f, K.nwb_f, f.nrows, K.d_far, s));
    for (int k = 0; k < c.parts; ++k) {
        if (A->comm.allgather_part_wait(A->comm.ctx, k) != 0) {
            qbh::set_error("allgather_part_wait hook failed");
            return QBH_ECOMM;
        }
        if (k == 0) QBH_TRY(prof_mark(A, 2));
        QBH_TRY(place(c, k));
        qbh::SpmvArgs fk = f;
        fk.wd = K.wd_f + (c.parts > 1 ? K.part_blk[k] : 0);
        fk.n_wb = c.parts > 1 ? K.part_blk[k + 1] - K.part_blk[k] : K.nwb_f;
        fk.wctr = A->d_wctr ? A->d_wctr + (3 + k) * 128 : nullptr;
        if (fk.n_wb > 0) QBH_TRY(qbh::launch_spmv_wave2(fk, K.tpr_f, 3, (int)std::min<int64_t>(grid_f, std::max<int64_t>(fk.n_wb, 8)), s));
    }
    return QBH_OK;
}

// Under a communicator the near pass needs only the rank's own x and runs while the exchange is in flight (epilogue without
// the far addend), then the far pass reads the gathered blocks and a light third pass adds its result and produces the
// reductions on the finished y.
int apply_comm(const KronCall &c, int *nparts)
{
    qbh_csr *A = c.A;
    const KronSplit &K = A->kron;
    hipStream_t s = A->stream;
    const qbh::SpmvArgs f = far_args(c);
    qbh::SpmvArgs nr;
    QBH_TRY(near_args(c, &nr));
    QBH_TRY(prof_begin(A));
    int grid_n, grid_f;
    comm_grids(A, &grid_n, &grid_f);
    QBH_TRY(qbh::launch_spmv_wave2(nr, K.tpr_n, 1, grid_n, s));          // y = alpha H_near x + beta y + gamma x
    QBH_TRY(prof_mark(A, 1));
    QBH_TRY(far_after_gather(c, f, grid_f));
    QBH_TRY(qbh::launch_kron_cross_rows(K.ia_x, K.xrow, K.n_xrows, K.ja_x, K.val_x, K.d_xt, K.t, K.d_far, s));
    QBH_TRY(qbh::launch_kron_combine(K.d_far, K.t, c.xl, c.y, A->nrows, c.alpha, c.red ? A->d_partials : nullptr, nparts, s, A->ovr_coef));
    return prof_mark(A, 3);
}

}  // namespace

namespace qbhapi {

int spmv_kron(qbh_csr *A, const d2 *x, d2 *y, double alpha, double beta, double gamma, double *red)
{
    const KronSplit &K = A->kron;
    if (!kron_path(A)) {
        qbh::set_error("this operator is stored split in place (qbh_opts.kron_split): the requested form of the SpMV (%s) needs its CSR",
                       A->has_comm ? "a communicator whose ranks do not all exchange tiled blocks" : (A->debug & 1) ? "QBH_DEBUG column mask"
                                                                                                             : "packed-real vectors");
        return QBH_EUNSUPP;
    }
    const bool comm = A->has_comm;
    KronCall c{};
    c.A = A;
    c.x = x;
    c.xl = comm ? x : x + A->row_offset;
    c.y = y;
    c.alpha = alpha;
    c.beta = beta;
    c.gamma = gamma;
    c.red = red;
    QBH_TRY(choose_walk(A, &c.walk));
    QBH_TRY(ensure_tiled_x(c));
    c.realw = tiled_real(A);
    c.sparse = comm && K.sparse && A->comm.exchange_v != nullptr;
    c.parts = c.sparse ? std::max(1, K.n_parts) : (comm && K.n_parts > 1 && (!c.realw || A->comm.allgather_part_begin_w)) ? K.n_parts : 1;
    c.nfb = K.t.S / K.t.B;
    c.w_edge = K.t.S - c.nfb * K.t.B;
    int nparts = K.grid_n;
    if (comm) {
        QBH_TRY(start_exchange(c));
        QBH_TRY(apply_comm(c, &nparts));
    } else {
        QBH_TRY(apply_one_gpu(c, &nparts));
    }
    return spmv_finish(A, nparts, red, false);
}

}  // namespace qbhapi
