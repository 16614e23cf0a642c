// qbh_spmv.cpp -- reductions and timing events, the steps every SpMV route shares, SpMV dispatch (spmv_run: the guard and the
// choice of route; the matrix-free route; the stored-CSR route with its local and remote parts and the three forms of the coded
// split -- the split in place is qbh_spmv_kron.cpp), the real wire format, the BLAS-1 runs, the device building blocks
// (qbh_spmv_dev ...) and the host-vector seam qbh_multmv / qbh_multmv2 (src/sparse.cc:262-297).
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "qbh_api_priv.hpp"

using qbh::d2;
using namespace qbhapi;

// ------------------------------------------------- reductions / scalars --------
namespace qbhapi {


// partials[nparts*ncomp] -> host_out[ncomp], summed over ranks under a communicator.
int finish_reduction(qbh_csr *A, int nparts, int ncomp, double *host_out)
{
    double *ds = scal_buf(A);
    QBH_TRY(qbh::launch_reduce_partials(A->d_partials, nparts, ncomp, ds, A->stream));
    if (A->has_comm) {
        if (A->comm.allreduce_sum(A->comm.ctx, 0, ncomp) != 0) {
            qbh::set_error("allreduce_sum hook failed");
            return QBH_ECOMM;
        }
    }
    QBH_HIP(hipMemcpyAsync(A->h_scal, ds, (size_t)ncomp * sizeof(double), hipMemcpyDeviceToHost, A->stream));
    QBH_HIP(hipStreamSynchronize(A->stream));
    for (int c = 0; c < ncomp; ++c) host_out[c] = A->h_scal[c];
    return QBH_OK;
}

static void harvest_set(qbh_csr *A, hipEvent_t e0, hipEvent_t e1, hipEvent_t e2, hipEvent_t e3, bool p, bool p2, bool drop)
{
    float ms = 0.f, total = 0.f;
    bool any = false;
    if (p && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
        total += ms;
        any = true;
    }
    if (p2 && hipEventSynchronize(e3) == hipSuccess && hipEventElapsedTime(&ms, e2, e3) == hipSuccess) {
        total += ms;
        any = true;
    }
    if (any && !drop) {
        A->stats.ms_spmv += total;
        if (total < A->stats.ms_spmv_min) A->stats.ms_spmv_min = total;
    }
}

// everything that is pending: the sets queued behind the current one (oldest first), then the current one
// defer_red: the three fused sums stay on the device -- in the scalar buffer the communicator's all-reduce works on, summed
// over the ranks in stream order (no copy, no synchronisation)
int deferred_reduction(qbh_csr *A, int nparts)
{
    double *ds = scal_buf(A);
    QBH_TRY(qbh::launch_reduce_partials(A->d_partials, nparts, 3, ds, A->stream));
    if (A->has_comm && A->comm.allreduce_sum(A->comm.ctx, 0, 3) != 0) {
        qbh::set_error("allreduce_sum hook failed");
        return QBH_ECOMM;
    }
    return QBH_OK;
}

void harvest_events(qbh_csr *A)
{
    for (int i = 0; i < A->n_ev_old; ++i) {
        qbh_csr::EvSet &o = A->ev_old[i];
        harvest_set(A, o.e[0], o.e[1], o.e[2], o.e[3], o.p, o.p2, o.drop);
        o.p = o.p2 = o.drop = false;
    }
    // the queued sets keep their events (reused by next_event_set); they are simply no longer pending
    harvest_set(A, A->ev0, A->ev1, A->ev2, A->ev3, A->ev_pending, A->ev_pending2, A->ev_drop);
    A->ev_pending = A->ev_pending2 = A->ev_drop = false;
}

// In front of an SpMV's first timing event.  Ordinarily: wait for the previous SpMV's events (as ever).  Under a pipelined driver
// (ev_keep) the previous SpMV may not even have started: its set is queued and a free one becomes current; only a set three
// SpMVs old is ever waited for.
int next_event_set(qbh_csr *A)
{
    if (!A->ev_keep) {
        harvest_events(A);
        return QBH_OK;
    }
    if (!A->ev_pending && !A->ev_pending2) return QBH_OK;            // the current set is free
    constexpr int NQ = (int)(sizeof(A->ev_old) / sizeof(A->ev_old[0]));
    // a slot whose set is no longer pending (or was never created) takes the current events; its own become current
    int slot = -1;
    for (int i = 0; i < NQ && slot < 0; ++i)
        if (!A->ev_old[i].p && !A->ev_old[i].p2) slot = i;
    if (slot < 0) {                                                   // all in flight: the oldest is three SpMVs old
        qbh_csr::EvSet &o = A->ev_old[0];
        harvest_set(A, o.e[0], o.e[1], o.e[2], o.e[3], o.p, o.p2, o.drop);
        o.p = o.p2 = o.drop = false;
        qbh_csr::EvSet first = A->ev_old[0];
        for (int i = 0; i + 1 < NQ; ++i) A->ev_old[i] = A->ev_old[i + 1];
        A->ev_old[NQ - 1] = first;
        slot = NQ - 1;
    }
    qbh_csr::EvSet &q = A->ev_old[slot];
    for (int k = 0; k < 4; ++k)
        if (!q.e[k]) QBH_HIP(hipEventCreate(&q.e[k]));
    std::swap(q.e[0], A->ev0);
    std::swap(q.e[1], A->ev1);
    std::swap(q.e[2], A->ev2);
    std::swap(q.e[3], A->ev3);
    q.p = A->ev_pending;
    q.p2 = A->ev_pending2;
    q.drop = A->ev_drop;
    A->ev_pending = A->ev_pending2 = A->ev_drop = false;
    if (slot + 1 > A->n_ev_old) A->n_ev_old = slot + 1;
    return QBH_OK;
}

// ------------------------------------------------- steps every route shares ----
// qbh_opts.profile brackets the launches of an SpMV: ev0 in front of the first ...
int prof_begin(qbh_csr *A)
{
    if (!A->opts.profile) return QBH_OK;
    QBH_TRY(next_event_set(A));
    QBH_HIP(hipEventRecord(A->ev0, A->stream));
    return QBH_OK;
}

// ... ev1 behind the first part, ev2 / ev3 around the part that had to wait for the exchange; 1 and 3 close a bracket
int prof_mark(qbh_csr *A, int k)
{
    if (!A->opts.profile) return QBH_OK;
    QBH_HIP(hipEventRecord(k == 1 ? A->ev1 : k == 2 ? A->ev2 : A->ev3, A->stream));
    if (k == 1) A->ev_pending = true;
    if (k == 3) A->ev_pending2 = true;
    return QBH_OK;
}

int cu_count(qbh_csr *A)
{
    if (A->ncu <= 0) {
        hipDeviceProp_t prop;
        A->ncu = (hipGetDeviceProperties(&prop, A->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    return A->ncu;
}

static int expand_packed(qbh_csr *A)          // d_xfull_r (doubles) -> d_xfull (complex, zero imaginary part)
{
    return qbh::launch_unpack_real(A->comm.d_xfull_r, reinterpret_cast<d2 *>(A->comm.d_xfull), A->comm_full, A->stream);
}

// the whole gather begun with allgather_begin; expand: the wire is packed and the kernel that reads x is not the real one
int gather_wait(qbh_csr *A, bool expand)
{
    if (A->comm.allgather_wait(A->comm.ctx) != 0) {
        qbh::set_error("allgather_wait hook failed");
        return QBH_ECOMM;
    }
    return expand ? expand_packed(A) : QBH_OK;
}

// behind the last launch: the counters, and the three fused sums of the nparts partial-sum blocks
int spmv_finish(qbh_csr *A, int nparts, double *red, bool real_gather)
{
    A->xr_of = nullptr;                      // the packed copy is consumed by exactly one SpMV
    A->stats.n_spmv++;
    if (real_gather) A->stats.n_spmv_real++;
    if (red && A->defer_red) return deferred_reduction(A, nparts);
    if (red) {
        QBH_TRY(finish_reduction(A, nparts, 3, red));
        if (A->opts.profile) harvest_events(A);
    }
    return QBH_OK;
}

// ------------------------------------------------- spmv_run and its routes -----
struct SpmvCall {            // one unsplit SpMV: its arguments and where its x comes from (start_gather)
    qbh_csr  *A;
    const d2 *x;
    d2       *y;
    double    alpha, beta, gamma;
    double   *red;
    const d2 *xg, *xl;       // gather source (full length), the rank's own block
    bool      packed;        // the exchange carries packed real parts ...
    bool      realm;         // ... and the row kernel gathers them as they are (else they are expanded to complex first)
    bool      async_gather;  // the gather is in flight and has to be waited for
    const double *xr_nocomm; // packed real parts of x when there is no communicator
};

static int start_gather(SpmvCall &c)
{
    qbh_csr *A = c.A;
    const d2 *x = c.x;
    c.packed = A->has_comm && A->real_wire;
    c.realm = A->real_mode && A->kernel == QBH_KERNEL_ROWS && (c.packed || !A->has_comm);
    c.async_gather = false;
    if (A->has_comm) {
        if (c.packed) {
            if (!(c.realm && A->xr_of == x))
                QBH_TRY(qbh::launch_pack_real(x, reinterpret_cast<double *>(A->comm.d_xsend), A->nrows, A->d_flag, A->stream));
        } else
            QBH_HIP(hipMemcpyAsync(A->comm.d_xsend, x, (size_t)A->nrows * sizeof(d2), hipMemcpyDeviceToDevice,
                                   A->stream));
        c.async_gather = A->comm.allgather_begin && A->comm.allgather_wait;
        const int hrc = c.async_gather ? A->comm.allgather_begin(A->comm.ctx, c.packed ? 1 : 0)
                                       : A->comm.allgather_x(A->comm.ctx, c.packed ? 1 : 0);
        if (hrc != 0) {
            qbh::set_error("allgather hook failed");
            return QBH_ECOMM;
        }
        if (!c.async_gather && c.packed && !c.realm) QBH_TRY(expand_packed(A));
        A->stats.n_gather++;
        A->wire_bytes_last = c.packed ? 8 : 16;
        c.xg = reinterpret_cast<const d2 *>(A->comm.d_xfull);
        c.xl = x;
    } else if (A->ovr_yr != nullptr) {           // all-real operation on packed vectors (driver-internal)
        if (!c.realm || A->nrows != A->ncols) {
            qbh::set_error("all-real SpMV needs the real fast path on an unsharded operator");
            return QBH_EINVAL;
        }
        c.xg = c.xl = nullptr;
    } else {
        c.xg = x;
        c.xl = x + A->row_offset;
        if (c.realm && A->xr_of != x) QBH_TRY(qbh::launch_pack_real(x, A->d_xr, A->ncols, A->d_flag, A->stream));
    }
    c.xr_nocomm = A->ovr_yr != nullptr ? A->ovr_xr : A->d_xr;
    return QBH_OK;
}

static int mf_sector_args(qbh_csr *A, const qbh::MfVec &v, const double *xr_nocomm, qbh::MfSecArgs *out)
{
    const qbh::MfSec &t = *A->mfsec;
    qbh::MfSecArgs ms{};
    ms.t = A->d_mfsec;
    ms.n_items = t.n_items;
    ms.dim = A->nrows;
    ms.n_rrows = t.n_rrows;
    ms.rrow = t.rrow;
    ms.ria = t.ria;
    ms.rja = t.rja;
    ms.rval = t.rval;
    ms.v = v;
    ms.xl_re = v.y_re ? xr_nocomm : nullptr;
    ms.orbit = t.orbit;
    ms.ucfg = t.ucfg;
    ms.oid = t.oid;
    ms.utab = t.utab;
    ms.oek = t.oek;
    ms.uext = t.uext;
    ms.tpar = t.tpar;
    ms.usgn = t.usgn;
    ms.n_orb = t.n_orb;
    ms.w_orb = t.w_orb;
    ms.tile = t.tile;
    // items drawn from per-XCD counters: the orbit-order kernel by default (its workgroups finish far apart under a
    // static assignment: 87 -> 61 ms on 4x5 with 8+8), the rank-table kernel only on request (it got slower: 223 -> 233 ms)
    const int sec_walk = A->dbg.sec_walk < 0 ? (ms.orbit ? 1 : 0) : A->dbg.sec_walk;
    if (sec_walk) {
        if (!A->d_wctr) QBH_HIP(qbh::dev_alloc(&A->d_wctr, qbh::kWctrRegions * 128 * sizeof(unsigned long long)));
        QBH_HIP(hipMemsetAsync(A->d_wctr, 0, 3 * 128 * sizeof(unsigned long long), A->stream));
        ms.ctr = reinterpret_cast<unsigned int *>(A->d_wctr);
    }
    *out = ms;
    return QBH_OK;
}

// matrix-free operator: one launch, needs the whole gathered x
static int spmv_mf(SpmvCall &c)
{
    qbh_csr *A = c.A;
    QBH_TRY(start_gather(c));
    if (c.async_gather) QBH_TRY(gather_wait(A, c.packed && !c.realm));
    qbh::MfVec v{};
    v.row_begin = A->row_offset;
    v.nrows = A->nrows;
    v.xg = c.xg;
    v.xl = c.xl;
    v.xr = c.realm ? (A->has_comm ? A->comm.d_xfull_r : c.xr_nocomm) : nullptr;
    v.y = c.y;
    v.y_re = A->has_comm ? nullptr : A->ovr_yr;
    v.alpha = c.alpha;
    v.beta = c.beta;
    v.gamma = c.gamma;
    v.partials = c.red ? A->d_partials : nullptr;
    QBH_TRY(prof_begin(A));
    int mf_parts = A->grid;
    switch (A->kind) {
    case 1: QBH_TRY(qbh::launch_mf_hubbard(qbh::MfArgs{A->mf, v}, A->grid, A->stream, &mf_parts)); break;
    case 2: QBH_TRY(qbh::launch_mf_heis(A->mfh, v, A->stream, &mf_parts)); break;
    case 4: QBH_TRY(qbh::launch_mf_qudit(A->mfq, v, A->stream, &mf_parts)); break;
    case 5: QBH_TRY(qbh::launch_mf_kondo(A->mfk, v, A->stream, &mf_parts)); break;
    case 6: QBH_TRY(qbh::launch_mf_qudit_repr(A->mfqr, v, A->stream, &mf_parts)); break;
    case 7: QBH_TRY(qbh::launch_mf_kondo_repr(A->mfkr, v, A->stream, &mf_parts)); break;
    case 3: {
        qbh::MfSecArgs ms;
        QBH_TRY(mf_sector_args(A, v, c.xr_nocomm, &ms));
        QBH_TRY(qbh::launch_mf_sector(ms, A->stream, &mf_parts));
        break;
    }
    default:
        qbh::set_error("internal: operator kind %d has no matrix-free kernel", A->kind);
        return QBH_EUNSUPP;
    }
    QBH_TRY(prof_mark(A, 1));
    return spmv_finish(A, mf_parts, c.red, c.realm);
}

// the parts of a stored operator share one argument block: this names the arrays and launch geometry of one of them (the
// handle's own, `rem`, the parts of the coded split; a coded part has no values, like the handle it was cut from)
static void part_args(qbh::SpmvArgs &a, const CsrPart &p)
{
    a.ia = p.d_ia;
    a.ja = p.d_ja;
    a.val = p.d_val;
    a.code = p.d_code;
    a.rb = p.d_rb;
    a.bp = p.d_bp;
    a.n_blocks = p.n_blocks;
    a.unroll = p.unroll;
}

// the arguments of the launch over the handle's own arrays: everything, or the locally-owned columns of a split shard
static qbh::SpmvArgs local_args(const SpmvCall &c)
{
    const qbh_csr *A = c.A;
    CsrPart own;
    own.d_ia = A->d_ia;
    own.d_ja = A->d_ja;
    own.d_val = A->d_val;
    own.d_code = A->d_code;
    own.d_rb = A->d_rb;
    own.d_bp = A->d_bp;
    own.n_blocks = A->n_blocks;
    own.unroll = A->unroll;
    qbh::SpmvArgs a{};
    part_args(a, own);
    a.dict = A->d_dict;
    a.dict_mode = A->dict_mode;
    a.nrows = A->nrows;
    // the local part indexes x by GLOBAL column but only touches [row_offset, row_offset + nrows):
    // serve it from the local block so it does not depend on the gather
    a.xg = (A->has_rem && A->has_comm) ? c.xl - A->row_offset : c.xg;
    a.xr = nullptr;
    a.y_re = A->has_comm ? nullptr : A->ovr_yr;
    a.xl_re = a.y_re ? c.xr_nocomm : nullptr;
    if (c.realm) {
        if (!A->has_comm) a.xr = c.xr_nocomm;
        else if (A->has_rem) a.xr = reinterpret_cast<const double *>(A->comm.d_xsend) - A->row_offset;   // own block, packed
        else a.xr = A->comm.d_xfull_r;
    }
    a.xl = c.xl;
    a.y = c.y;
    a.alpha = c.alpha;
    a.beta = c.beta;
    a.gamma = c.gamma;
    a.yin = A->ovr_yin;
    a.coef = A->ovr_coef;
    a.coef_mode = A->ovr_coef ? 1 : 0;
    a.partials = (c.red && !A->has_rem) ? A->d_partials : nullptr;
    a.swizzle = A->opts.xcd_swizzle;
    a.chunk_mult = A->chunk_mult;
    a.colmask = (A->debug & 1) ? 1023 : -1;
    if ((A->debug & 1) && A->dbg.colmask) a.colmask = A->dbg.colmask;    // gather-window experiments (results wrong by design)
    return a;
}

// complex128 values, complex vectors: the wave kernel; the real gather / all-real forms stay on the row kernel
static bool takes_wave(const qbh_csr *A, const qbh::SpmvArgs &a) { return A->use_wave && a.xr == nullptr && a.y_re == nullptr; }

// qbh_opts.comm_reserve on a plain shard: the launch of the locally-owned columns runs while the gather is on the links; its
// grid is persistent (wave and row kernels), so it leaves room for RCCL's kernel (280 registers per lane, see the split path):
// at most cap workgroups per CU, cap - 1 on `reserve` of them, with cap from the registers a wavefront of this launch can own at
// its occupancy (512 / occ, an upper bound) so that 512 - (cap - 1) * v >= 280
static int overlap_grid(const SpmvCall &c, int g)
{
    qbh_csr *A = c.A;
    if (!(A->has_comm && A->has_rem && c.async_gather && A->comm.nranks > 1 && A->opts.comm_reserve >= 0)) return g;
    const int ncu = cu_count(A), occ = g / ncu;
    if (occ < 1) return g;                   // does not fill the chip anyway
    const int v = std::max(8, (512 / occ) / 8 * 8), cap = std::max(1, std::min(occ, 1 + 232 / v));
    const int reserve = A->opts.comm_reserve > 0 ? (A->opts.comm_reserve / 8) * 8 : 64;
    const int capped = std::min(g, cap * ncu);
    return std::max(8, (std::max(capped / 2, capped - reserve) / 8) * 8);
}

// T (x) 1 + 1 (x) T' + D recognised: the row-staged table kernel applies it from T, T' and one diagonal code per row --
// no tiled copy, no far sums: x read (+ its neighbour rows through the caches), old y read, y written
static int kronc_table(const SpmvCall &c, const qbh::SpmvArgs &a, int *nparts)
{
    qbh_csr::KronCoded &K = c.A->kronc;
    qbh::MfArgs m{};
    m.t = K.tables;
    m.v.row_begin = 0;
    m.v.nrows = c.A->nrows;
    m.v.xr = a.xr;
    m.v.y_re = a.y_re;
    m.v.alpha = a.alpha;
    m.v.beta = a.beta;
    m.v.gamma = a.gamma;
    m.v.partials = c.red ? c.A->d_partials : nullptr;
    m.dcode = K.sl.dcode;
    m.ddict = K.sl.d_dictr;
    K.xt_of = nullptr;
    return qbh::launch_mf_hubbard(m, 0, c.A->stream, nparts);
}

// sliced form: far pass (row sums in group order), near pass from the LDS-resident block of x with the whole epilogue
static int kronc_sliced(const SpmvCall &c, const qbh::SpmvArgs &a, int *nparts)
{
    qbh_csr *A = c.A;
    return qbh::launch_kronc(A->kronc.sl, A->d_dict, A->n_dict, A->kronc.d_xt, a.xr, a.y_re, a.alpha, a.beta, a.gamma, c.red ? A->d_partials : nullptr,
                             reinterpret_cast<unsigned int *>(A->d_wctr), A->opts.deterministic != 0, nparts, A->stream);
}

// two parts for the row kernel: near launch (full epilogue), far launch (tiled rows and columns, accumulates at orig(row),
// fused reductions of the finished y)
static int kronc_two_part(const SpmvCall &c, const qbh::SpmvArgs &a, int *nparts)
{
    qbh_csr *A = c.A;
    const qbh_csr::KronCoded &K = A->kronc;
    qbh::SpmvArgs np = a;
    part_args(np, K.near_p);
    np.partials = nullptr;
    QBH_TRY(qbh::launch_spmv(np, A->kernel, K.near_p.npb, K.near_p.tpr, K.near_p.grid, A->stream));
    qbh::SpmvArgs fp = a;
    part_args(fp, K.far_p);
    fp.xr = K.d_xt;
    fp.beta = 1.0;
    fp.gamma = 0.0;
    fp.partials = c.red ? A->d_partials : nullptr;
    fp.swizzle = 1;                             // contiguous eighths of the bands per XCD
    fp.rowmap = 1;
    fp.kS = K.t.S;
    fp.kNU = K.t.NU;
    fp.kB = K.t.B;
    QBH_TRY(qbh::launch_spmv(fp, A->kernel, K.far_p.npb, K.far_p.tpr, K.far_p.grid, A->stream));
    *nparts = K.far_p.grid;
    return QBH_OK;
}

// coded Kronecker split, all-real operation: one of its three forms; the two that gather from the tiled copy of the packed x
// make it unless the pass that produced x wrote it
static int kronc_part(const SpmvCall &c, const qbh::SpmvArgs &a, int *nparts)
{
    qbh_csr *A = c.A;
    qbh_csr::KronCoded &K = A->kronc;
    // (mf_row=0: the debug switch that turns the row-staged kernel off)
    if (K.sl.active && K.table_route && A->dbg.mf_row != 0) return kronc_table(c, a, nparts);
    if (K.xt_of != (const void *)a.xr) QBH_TRY(qbh::launch_kron_tile_re(a.xr, K.d_xt, A->nrows, K.t, A->stream));
    K.xt_of = nullptr;                           // an alias is good for one SpMV
    return K.sl.active ? kronc_sliced(c, a, nparts) : kronc_two_part(c, a, nparts);
}

// the launch over the handle's own arrays: the coded split, the wave kernel or the kernel the handle names.  `a` keeps what the
// wave kernel was given: the remote part goes on from it.
static int local_part(const SpmvCall &c, qbh::SpmvArgs &a, int *nparts)
{
    qbh_csr *A = c.A;
    if (A->kronc.active && c.realm && a.xr != nullptr && a.y_re != nullptr && !A->has_comm && !A->has_rem && !(A->debug & 1))
        return kronc_part(c, a, nparts);
    if (!takes_wave(A, a)) {
        *nparts = A->grid;
        return qbh::launch_spmv(a, A->kernel, A->npb, A->tpr, A->kernel == QBH_KERNEL_ROWS ? overlap_grid(c, A->grid) : A->grid, A->stream);
    }
    // The two passes of a Kronecker split take the dynamic ordered walk per XCD (DynWalk: C3 far pass 86 -> 64 GB, near pass
    // 92 -> 68 GB, 31.7 -> 31.0 ms); the unsplit wave kernel keeps the static chunked walk (xcd_swizzle 2), under which all XCDs
    // stream from ONE region -- ordered eighths cost it 34 -> 43 ms on C3.  xcd_swizzle 3 / QBH_WAVE_SWIZZLE choose by name.
    a.swizzle = A->opts.wave_walk >= 0 ? A->opts.wave_walk : A->opts.xcd_swizzle;
    if (a.swizzle == 3) {
        if (!A->d_wctr || A->opts.deterministic) a.swizzle = 2;
        else QBH_HIP(hipMemsetAsync(A->d_wctr, 0, 3 * 128 * sizeof(unsigned long long), A->stream));
    }
    a.wd = A->d_wd;
    a.n_wb = A->n_wb;
    a.wctr = A->d_wctr;
    *nparts = A->wgrid;
    return qbh::launch_spmv_wave(a, A->wtpr, overlap_grid(c, A->wgrid), A->stream);
}

// remote part of a split shard: the columns other ranks own, accumulating onto the local part's result once the gather is there
static int remote_part(const SpmvCall &c, qbh::SpmvArgs &a, int *nparts)
{
    qbh_csr *A = c.A;
    const CsrPart &R = A->rem;
    if (c.async_gather) QBH_TRY(gather_wait(A, c.packed && !c.realm));
    part_args(a, R);
    a.xg = c.xg;
    if (c.realm) a.xr = A->has_comm ? A->comm.d_xfull_r : c.xr_nocomm;
    a.beta = 1.0;
    a.gamma = 0.0;
    a.yin = nullptr;
    a.coef_mode = A->ovr_coef ? 2 : 0;
    a.partials = c.red ? A->d_partials : nullptr;
    QBH_TRY(prof_mark(A, 2));
    const bool wave = takes_wave(A, a);
    if (wave) {
        a.wd = R.d_wd;
        a.n_wb = R.n_wb;
        a.wctr = A->d_wctr + 128;          // the remote part's own counters (the local part may still be running)
        QBH_TRY(qbh::launch_spmv_wave(a, R.wtpr, R.wgrid, A->stream));
    } else {
        QBH_TRY(qbh::launch_spmv(a, A->kernel, R.npb, R.tpr, R.grid, A->stream));
    }
    *nparts = wave ? R.wgrid : R.grid;
    return prof_mark(A, 3);
}

static int spmv_csr(SpmvCall &c)
{
    qbh_csr *A = c.A;
    QBH_TRY(start_gather(c));
    qbh::SpmvArgs a = local_args(c);
    if (c.async_gather && !A->has_rem) {          // nothing to overlap with: the single part needs the gathered x
        QBH_TRY(gather_wait(A, c.packed && !c.realm));
        c.async_gather = false;
    }
    int nparts = 0;
    QBH_TRY(prof_begin(A));
    QBH_TRY(local_part(c, a, &nparts));
    QBH_TRY(prof_mark(A, 1));
    if (A->has_rem) QBH_TRY(remote_part(c, a, &nparts));
    return spmv_finish(A, nparts, c.red, c.realm);
}

int spmv_run(qbh_csr *A, const d2 *x, d2 *y, double alpha, double beta, double gamma, double *red)
{
    if (A->broken) {
        qbh::set_error("the operator was left inconsistent by an earlier failed call (qbh_csr_set_comm / creation): destroy it");
        return QBH_EINVAL;
    }
    if (A->kron.active) return spmv_kron(A, x, y, alpha, beta, gamma, red);
    if ((A->ovr_yin || A->ovr_coef) && (A->kind != 0 || A->ovr_yr != nullptr)) {
        qbh::set_error("internal: the pipelined three-term step needs a stored operator and complex vectors");
        return QBH_EUNSUPP;
    }
    SpmvCall c{A, x, y, alpha, beta, gamma, red};
    return A->kind != 0 ? spmv_mf(c) : spmv_csr(c);
}

// Drivers call this at entry with the vectors of their recurrence: when the operator is real and all of them
// have exactly zero imaginary parts (on every rank), the x exchange carries only real parts for this solve.
int enable_real_wire(qbh_csr *A, std::initializer_list<const d2 *> vecs)
{
    A->real_wire = false;
    A->real_mode = false;
    A->xr_of = nullptr;
    if (A->has_comm && !A->comm.d_xfull_r) return QBH_OK;
    // split shards exchanging tiled blocks: qbh_opts.real_wire alone decides (their kernels have no real forms to select);
    // everything else: the real fast path and its forms
    const bool tiled = A->has_comm && A->kron.active && A->kron.comm_tiled;
    if (tiled) {
        if (!A->opts.real_wire) return QBH_OK;
    } else {
        if (!A->opts.real_fast_path) return QBH_OK;
        if (!(A->opts.real_forms & 1)) return QBH_OK;
    }
    double total = A->values_real ? 0.0 : 1.0;
    // every rank must take the same decision: sum the per-vector |Im|^2 (and the operator flag) over ranks
    for (const d2 *v : vecs) {
        double sq = 0.0;
        QBH_TRY(qbh::launch_imag_norm(v, A->nrows, A->d_partials, A->stream));
        QBH_TRY(finish_reduction(A, qbh::blas_grid(A->nrows), 1, &sq));
        total += sq;
    }
    double flag_sum = 0.0;
    {   // the operator flag also has to be agreed on
        const double mine = A->values_real ? 0.0 : 1.0;
        QBH_HIP(hipMemcpyAsync(A->d_partials, &mine, sizeof(double), hipMemcpyHostToDevice, A->stream));
        QBH_HIP(hipStreamSynchronize(A->stream));
        QBH_TRY(finish_reduction(A, 1, 1, &flag_sum));
    }
    if (total == 0.0 && flag_sum == 0.0) {
        QBH_HIP(hipMemsetAsync(A->d_flag, 0, sizeof(int), A->stream));
        A->real_wire = A->has_comm;
        // the row kernel can then gather 8-byte real parts (bit-identical result, half the x traffic)
        A->real_mode = A->kernel == QBH_KERNEL_ROWS && !tiled;
        if (!(A->opts.real_forms & 2)) A->real_mode = false;
        if (A->real_mode && !A->has_comm && !A->d_xr) QBH_HIP(qbh::dev_alloc(&A->d_xr, (size_t)A->ncols * sizeof(double)));
    }
    return QBH_OK;
}

// ... and this at exit: a non-zero imaginary part met while packing means results are wrong -> loud error.
int finish_real_wire(qbh_csr *A)
{
    A->xr_of = nullptr;
    if (!A->real_wire && !A->real_mode) return QBH_OK;
    A->real_wire = false;
    A->real_mode = false;
    int f = 0;
    QBH_HIP(hipMemcpyAsync(&f, A->d_flag, sizeof(int), hipMemcpyDeviceToHost, A->stream));
    QBH_HIP(hipStreamSynchronize(A->stream));
    const double mine = (double)f;
    double all = 0.0;
    QBH_HIP(hipMemcpyAsync(A->d_partials, &mine, sizeof(double), hipMemcpyHostToDevice, A->stream));
    QBH_HIP(hipStreamSynchronize(A->stream));
    QBH_TRY(finish_reduction(A, 1, 1, &all));
    if (all != 0.0) {
        qbh::set_error("real wire format met a non-zero imaginary part (internal error)");
        return QBH_EHIP;
    }
    return QBH_OK;
}


int dotc_run(qbh_csr *A, const d2 *x, const d2 *y, double *res2)
{
    QBH_TRY(qbh::launch_dotc(x, y, A->nrows, A->d_partials, A->stream));
    return finish_reduction(A, qbh::blas_grid(A->nrows), 2, res2);
}


int axpy_norm_run(qbh_csr *A, d2 alpha, const d2 *x, d2 *y, double *nrm2sq)
{
    double *yr = packed_target(A);          // y is the next SpMV's x in every driver: emit its packed copy here
    if (d2 *yt = tiled_target(A)) {         // ... or, for a Kronecker split, its tiled copy
        QBH_TRY(qbh::launch_axpy_norm_tile(alpha, nullptr, x, y, yt, A->nrows, A->kron.t, A->d_partials, A->stream, nullptr, tiled_real(A), A->d_flag));
        A->kron.xt_of = y;
        A->xr_of = nullptr;
        return finish_reduction(A, qbh::blas_grid(A->nrows), 1, nrm2sq);
    }
    QBH_TRY(qbh::launch_axpy_norm(alpha, nullptr, x, y, A->nrows, A->d_partials, yr, A->d_flag, A->stream));
    A->xr_of = yr ? y : nullptr;
    A->kron.xt_of = nullptr;
    return finish_reduction(A, qbh::blas_grid(A->nrows), 1, nrm2sq);
}

// Single-GPU Lanczos step tail: y += (scale * d_scal[0]) x with d_scal[0] = <x, w> left on the device by a deferred
// spmv_run, then |y|^2; ONE copy + synchronisation returns both scalars (dot_out = d_scal[0], *nrm2sq).
int axpy_norm_deferred(qbh_csr *A, double scale, const d2 *x, d2 *y, double *dot_out, double *nrm2sq)
{
    double *yr = packed_target(A);
    if (d2 *yt = tiled_target(A)) {
        QBH_TRY(qbh::launch_axpy_norm_tile(d2{scale, 0.0}, A->d_scal, x, y, yt, A->nrows, A->kron.t, A->d_partials, A->stream, nullptr, tiled_real(A), A->d_flag));
        A->kron.xt_of = y;
        A->xr_of = nullptr;
    } else {
        QBH_TRY(qbh::launch_axpy_norm(d2{scale, 0.0}, A->d_scal, x, y, A->nrows, A->d_partials, yr, A->d_flag, A->stream));
        A->xr_of = yr ? y : nullptr;
        A->kron.xt_of = nullptr;
    }
    QBH_TRY(qbh::launch_reduce_partials(A->d_partials, qbh::blas_grid(A->nrows), 1, A->d_scal + 4, A->stream));
    QBH_HIP(hipMemcpyAsync(A->h_scal, A->d_scal, 5 * sizeof(double), hipMemcpyDeviceToHost, A->stream));
    QBH_HIP(hipStreamSynchronize(A->stream));
    *dot_out = A->h_scal[0];
    *nrm2sq = A->h_scal[4];
    if (A->opts.profile) harvest_events(A);
    return QBH_OK;
}

int nrm2_run(qbh_csr *A, const d2 *x, double *nrm)
{
    double sq = 0.0;
    QBH_TRY(qbh::launch_nrm2sq(x, A->nrows, A->d_partials, A->stream));
    QBH_TRY(finish_reduction(A, qbh::blas_grid(A->nrows), 1, &sq));
    *nrm = std::sqrt(sq);
    return QBH_OK;
}

}  // namespace qbhapi

// ----------------------------------------------- device building blocks --------
extern "C" int qbh_spmv_dev(const qbh_csr *Ac, const qbh_z *d_x, qbh_z *d_y, double alpha, double beta,
                            double gamma, double *red)
{
    qbh_csr *A = const_cast<qbh_csr *>(Ac);
    if (!A || !d_x || !d_y) return QBH_EINVAL;
    Bind bind(A);
    return spmv_run(A, reinterpret_cast<const d2 *>(d_x), reinterpret_cast<d2 *>(d_y), alpha, beta, gamma, red);
}

extern "C" int qbh_dotc_dev(const qbh_csr *Ac, const qbh_z *d_x, const qbh_z *d_y, double *res)
{
    qbh_csr *A = const_cast<qbh_csr *>(Ac);
    if (!A || !d_x || !d_y || !res) return QBH_EINVAL;
    Bind bind(A);
    return dotc_run(A, reinterpret_cast<const d2 *>(d_x), reinterpret_cast<const d2 *>(d_y), res);
}

extern "C" int qbh_axpy_norm_dev(const qbh_csr *Ac, qbh_z alpha, const qbh_z *d_x, qbh_z *d_y, double *nrm2_sq)
{
    qbh_csr *A = const_cast<qbh_csr *>(Ac);
    if (!A || !d_x || !d_y || !nrm2_sq) return QBH_EINVAL;
    Bind bind(A);
    return axpy_norm_run(A, d2{alpha.re, alpha.im}, reinterpret_cast<const d2 *>(d_x),
                         reinterpret_cast<d2 *>(d_y), nrm2_sq);
}

extern "C" int qbh_scal_dev(const qbh_csr *Ac, double a, qbh_z *d_x)
{
    qbh_csr *A = const_cast<qbh_csr *>(Ac);
    if (!A || !d_x) return QBH_EINVAL;
    Bind bind(A);
    return qbh::launch_scal(a, reinterpret_cast<d2 *>(d_x), A->nrows, A->stream);
}

extern "C" int qbh_nrm2_dev(const qbh_csr *Ac, const qbh_z *d_x, double *nrm)
{
    qbh_csr *A = const_cast<qbh_csr *>(Ac);
    if (!A || !d_x || !nrm) return QBH_EINVAL;
    Bind bind(A);
    return nrm2_run(A, reinterpret_cast<const d2 *>(d_x), nrm);
}

// -------------------------------------------------- host-vector seam -----------
namespace qbhapi {
int multmv_host(qbh_csr *A, const qbh_z *x_host, qbh_z *y_host, double beta)
{
    if (!A || !x_host || !y_host) return QBH_EINVAL;
    if (A->has_comm || A->nrows != A->ncols) {
        qbh::set_error("qbh_multmv: host-vector seam needs an unsharded operator");
        return QBH_EUNSUPP;
    }
    Bind bind(A);
    const size_t bytes = (size_t)A->nrows * sizeof(d2);
    if (!A->d_stage_x) QBH_HIP(qbh::dev_alloc(&A->d_stage_x, bytes));
    if (!A->d_stage_y) QBH_HIP(qbh::dev_alloc(&A->d_stage_y, bytes));
    if (A->basis.kind != 0) {                     // the caller's order at the seam, the internal one in HBM
        QBH_TRY(vec_h2d(A, A->d_stage_x, x_host, A->nrows));
        if (beta != 0.0) QBH_TRY(vec_h2d(A, A->d_stage_y, y_host, A->nrows));
        QBH_TRY(spmv_run(A, A->d_stage_x, A->d_stage_y, 1.0, beta, 0.0, nullptr));
        return vec_d2h(A, y_host, A->d_stage_y, A->nrows);
    }
    QBH_HIP(hipMemcpyAsync(A->d_stage_x, x_host, bytes, hipMemcpyHostToDevice, A->stream));
    if (beta != 0.0) QBH_HIP(hipMemcpyAsync(A->d_stage_y, y_host, bytes, hipMemcpyHostToDevice, A->stream));
    QBH_TRY(spmv_run(A, A->d_stage_x, A->d_stage_y, 1.0, beta, 0.0, nullptr));
    QBH_HIP(hipMemcpyAsync(y_host, A->d_stage_y, bytes, hipMemcpyDeviceToHost, A->stream));
    QBH_HIP(hipStreamSynchronize(A->stream));
    return QBH_OK;
}
}  // namespace qbhapi

extern "C" int qbh_multmv(const qbh_csr *A, const qbh_z *x_host, qbh_z *y_host)
{
    return multmv_host(const_cast<qbh_csr *>(A), x_host, y_host, 0.0);
}

extern "C" int qbh_multmv2(const qbh_csr *A, const qbh_z *x_host, qbh_z *y_host)
{
    return multmv_host(const_cast<qbh_csr *>(A), x_host, y_host, 1.0);
}
