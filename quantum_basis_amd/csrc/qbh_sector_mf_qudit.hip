// qbh_sector_mf_qudit.hip -- qbh_mf_qudit_repr (toolkit and the d-level family: qbh_sector.hpp)
//
// The sector operator of qbh_gen_qudit_repr applied from its basis, without a stored matrix (MfQuditRepr in qbh_internal.hpp).
// What stays in HBM is the representative list (8 B per row), one info byte per row, the directory of the enumeration (8 B per
// 4096 words) and the tables: no row pointers, no columns, no values.  One lane handles one representative row and walks the
// merged terms in the order qrepr_row walks them; for each entry it forms the word c, canonicalises it with the byte-sliced
// translation tables (sector_canonical: n_trans x n_chunks table reads), finds the position of the representative b and
// accumulates <a|M|c> conj(chi(g*)) sqrt(|S_b|/|S_a|) x[b] as the entries arrive.  Nothing is staged per row, so the limit of
// 160 entries per row of the stored form does not apply, and the order of the sums of a row does not depend on which rows
// the launch covers: a row shard is bit-identical to the same rows of the whole operator.
//
// The position of b is not looked up in the whole list: rank(b) >> 12 (qd_rank, the inverse of the enumeration's qd_unrank)
// names the chunk of 4096 words that holds b, the directory gives the positions of that chunk's first and last
// representatives, and a bisection of at most 12 steps inside those (at most 32 KB, contiguous) ends at what sector_find
// returns from 31 steps over the whole list.
#include "qbh_sector.hpp"
#include "qbh_mf_row.hpp"

namespace qbh {
namespace {

constexpr int kMfQreprBlock = 1024;      // one workgroup per CU when the tables fill LDS: 4 waves per SIMD
constexpr size_t kMfQreprLdsCap = (size_t)150 * 1024;        // the budget of launch_mf_heis

inline size_t mf_qrepr_lds_bytes(const MfQuditRepr &t) { return t.tables_lds ? ((size_t)t.n_tab + (size_t)t.n_cum) * 8 : 0; }

// the terms of the row of representative a (|S_a| = sa, nonzero norm) in the order of qrepr_row: sink(position of b, value)
// for every off-diagonal term entry whose target has nonzero norm; returns the diagonal of the single-site and pair terms
template <class Sink>
__device__ __forceinline__ double qrepr_walk(const QuditReprDev &R, const uint64_t *tab, const uint64_t *cum, const uint64_t *reps,
                                             const uint8_t *info, const int64_t *chunk_pos, int64_t dim, uint64_t a, double sa, Sink sink)
{
    const int d2n = R.d * R.d;
    const uint64_t field = (1ULL << R.bits) - 1ULL;
    double dg = 0.0;
    for (int s = 0; s < R.n_sites; ++s) dg += R.sdiag[s * R.d + qd_level(a, R.bits, s)];
    for (int p = 0; p < R.n_pairs; ++p) {
        const int ij = R.pair_ij[p];
        const int si = ij & 0xff, sj = ij >> 8;
        const int in = qd_level(a, R.bits, si) * R.d + qd_level(a, R.bits, sj);
        dg += R.pdiag[p * d2n + in];
        const int e1 = R.eoff[p * d2n + in + 1];
        for (int e = R.eoff[p * d2n + in]; e < e1; ++e) {
            const uint64_t c = qrepr_target(a, R.bits, field, si, sj, R.eout[e]);
            int g = 0;
            const uint64_t b = sector_canonical(R, tab, c, &g);
            const int64_t lo = sector_dir_find(reps, chunk_pos, dim, b, qd_rank(cum, R.n_sites, R.bits, R.tw, b));
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;      // zero-norm target: dropped
            sink(lo, qrepr_value(R, R.eval[e], g, cj, sa));
        }
    }
    return dg;
}

// tab | cum into LDS (TLDS) and the pointers the row walk reads them through
template <bool TLDS>
__device__ __forceinline__ void qrepr_stage(const MfQuditRepr &t, uint64_t *lds, int nthreads, const uint64_t *&tab, const uint64_t *&cum)
{
    if (TLDS) {
        for (int k = threadIdx.x; k < t.n_tab; k += nthreads) lds[k] = t.tab[k];
        for (int k = threadIdx.x; k < t.n_cum; k += nthreads) lds[t.n_tab + k] = t.cum[k];
        __syncthreads();
        tab = lds;
        cum = lds + t.n_tab;
    } else {
        tab = t.tab;
        cum = t.cum;
    }
}

// y <- alpha H x + beta y + gamma x on rows [row_begin, row_begin + nrows) of the sector: one lane per row, grid-stride over
// a resident grid, every row gathers (no atomics).  Epilogue and partial sums: qbh_mf_row.hpp.
template <bool REALX, bool TLDS>
__global__ __launch_bounds__(kMfQreprBlock) void k_mf_qudit_repr(MfQuditRepr t, MfVec a)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t qr_lds[];
    __shared__ double red[3 * (kMfQreprBlock / 64)];
    const QuditReprDev &R = *static_cast<const QuditReprDev *>(t.R);
    const int tid = threadIdx.x;
    const uint64_t *tab, *cum;
    qrepr_stage<TLDS>(t, qr_lds, kMfQreprBlock, tab, cum);
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kMfQreprBlock;
    for (int64_t lrow = (int64_t)blockIdx.x * kMfQreprBlock + tid; lrow < a.nrows; lrow += stride) {
        const int64_t grow = a.row_begin + lrow;
        const uint8_t ci = t.info[grow];
        d2 yo, xi;
        mf_row_load<REALX>(a, lrow, grow, yo, xi);
        d2 sum = {0.0, 0.0};
        double dg;
        if (ci & 0x80) {                  // zero norm at this momentum: the decoupled row of row_zero_norm
            dg = R.fake_pos + (double)grow / (double)t.dim;
        } else {
            dg = qrepr_walk(R, tab, cum, t.reps, t.info, t.chunk_pos, t.dim, t.reps[grow], (double)(ci & 0x7f),
                            [&](int64_t lo, d2 v) { mf_gather_add<REALX>(a, sum, v, lo); });
        }
        mf_row_finish(a, lrow, sum, dg, xi, yo, acc);
    }
    mf_block_partials<kMfQreprBlock>(acc, red, a.partials);
}

// the contributions the apply kernel makes for rows [row_begin, row_end): one diagonal per row and every off-diagonal term
// entry whose target has nonzero norm, before duplicates merge.  One sum per workgroup.
template <bool TLDS>
__global__ __launch_bounds__(kMfQreprBlock) void k_mf_qudit_repr_count(MfQuditRepr t, int64_t row_begin, int64_t row_end,
                                                                       unsigned long long *part)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t qr_lds[];
    __shared__ unsigned long long red[kMfQreprBlock / 64];
    const QuditReprDev &R = *static_cast<const QuditReprDev *>(t.R);
    const uint64_t *tab, *cum;
    qrepr_stage<TLDS>(t, qr_lds, kMfQreprBlock, tab, cum);
    unsigned long long c = 0;
    const int64_t stride = (int64_t)gridDim.x * kMfQreprBlock;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * kMfQreprBlock + threadIdx.x; row < row_end; row += stride) {
        const uint8_t ci = t.info[row];
        c += 1;
        if (!(ci & 0x80))
            (void)qrepr_walk(R, tab, cum, t.reps, t.info, t.chunk_pos, t.dim, t.reps[row], (double)(ci & 0x7f),
                             [&](int64_t, d2) { c += 1; });
    }
    mf_block_count<kMfQreprBlock>(c, red, part);
}

// the resident grid of both kernels: as many workgroups per CU as the LDS they stage allows (at most two of 1024 lanes)
inline int mf_qrepr_grid(const MfQuditRepr &t, int64_t nrows)
{
    const size_t lds = mf_qrepr_lds_bytes(t);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, ((size_t)158 * 1024) / (lds + 1024)));
    const int64_t nblk = (nrows + kMfQreprBlock - 1) / kMfQreprBlock;
    return (int)std::min<int64_t>(nblk, std::min<int64_t>((int64_t)device_cu_count() * per_cu, kMaxRedBlocks));
}

}  // namespace

int launch_mf_qudit_repr(const MfQuditRepr &t, const MfVec &a, hipStream_t s, int *nparts_out)
{
    const bool tl = t.tables_lds != 0;
    const size_t lds = mf_qrepr_lds_bytes(t);
    const int g = mf_qrepr_grid(t, a.nrows);
#define QBH_QREPR_LAUNCH(RX, TL)                                                                                                        \
    do {                                                                                                                               \
        if (TL)                                                                                                                        \
            QBH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mf_qudit_repr<RX, TL>),                                       \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                        \
        hipLaunchKernelGGL((k_mf_qudit_repr<RX, TL>), dim3(g), dim3(kMfQreprBlock), lds, s, t, a);                                     \
    } while (0)
    if (a.xr != nullptr) {
        if (tl) QBH_QREPR_LAUNCH(true, true); else QBH_QREPR_LAUNCH(true, false);
    } else {
        if (tl) QBH_QREPR_LAUNCH(false, true); else QBH_QREPR_LAUNCH(false, false);
    }
#undef QBH_QREPR_LAUNCH
    QBH_HIP(hipGetLastError());
    if (nparts_out) *nparts_out = g;
    return QBH_OK;
}

}  // namespace qbh

extern "C" int qbh_mf_qudit_repr(qbh_csr **out, int n_sites, int d, int total, int n_pairs, const int32_t *pair_sites,
                                 const qbh_z *pair_mat, int n_single, const int32_t *single_sites, const double *single_diag,
                                 int n_trans, const int32_t *perms, const double *chars, double fake_pos, int64_t row_begin,
                                 int64_t row_end, int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    const char *who = "qbh_mf_qudit_repr";
    if (!out) {
        set_error("%s: out is NULL", who);
        return QBH_EINVAL;
    }
    QBH_TRY(qudit_check_shape(who, n_sites, d));
    if (total < 0 || total > n_sites * (d - 1) || n_pairs < 0 || n_single < 0 || (n_pairs > 0 && (!pair_sites || !pair_mat)) ||
        (n_single > 0 && (!single_sites || !single_diag))) {
        set_error("%s: invalid charge %d (0 .. %d) or term arrays", who, total, n_sites * (d - 1));
        return QBH_EINVAL;
    }
    if (!perms || !chars || n_trans < 1 || n_trans > kReprMaxTrans) {
        set_error("%s: invalid symmetry argument (1 .. %d translations)", who, kReprMaxTrans);
        return QBH_EINVAL;
    }
    QuditTerms T;
    QBH_TRY(qudit_merge_terms(who, n_sites, d, n_pairs, pair_sites, pair_mat, n_single, single_sites, single_diag, T));
    QuditReprDev R;
    std::vector<uint64_t> tab;
    QBH_TRY(qrepr_symmetry(R, tab, n_sites, d, total, n_trans, perms, chars, who));
    QBH_TRY(qrepr_invariant(T, n_sites, d, n_trans, perms, who));
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));
    // what can be said about the row range before the sector is enumerated: the dimension is at most the number of words
    if (row_begin < 0 || row_end < -1 || (row_end >= 0 && row_begin >= row_end) || row_begin >= nstates || row_end > nstates) {
        set_error("%s: bad row range [%lld, %lld) of a sector of %lld words", who, (long long)row_begin, (long long)row_end,
                  (long long)nstates);
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {        // every refusal above comes before the device is looked for
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP_WHO(who, hipSetDevice(opts->device));

    // real values: every merged pair matrix real and every character real.  A character computed as exp(-i k.t) at k = pi
    // carries sin(pi t), which rounds to at most 64 pi 2^-53 = 2.2e-14 for the 64 translations allowed: an imaginary part
    // below 1e-13 is that rounding and is dropped, so that the real and the complex kernel apply the same numbers.
    bool values_real = true;
    for (const d2 &v : T.eval)
        if (v.y != 0.0) values_real = false;
    for (int g = 0; g < n_trans; ++g)
        if (std::fabs(R.chr[2 * g + 1]) > 1e-13) values_real = false;
    if (values_real)
        for (int g = 0; g < n_trans; ++g) R.chr[2 * g + 1] = 0.0;

    R.n_pairs = (int)T.pm.size();
    R.fake_pos = fake_pos;
    DevBufs bufs;
    int32_t *pij = nullptr, *eo = nullptr, *eu = nullptr;
    double *pd = nullptr, *sd = nullptr;
    d2 *ev = nullptr;
    QBH_TRY(upload(T.pair_ij, &pij, bufs.pool));
    QBH_TRY(upload(T.eoff, &eo, bufs.pool));
    QBH_TRY(upload(T.eout, &eu, bufs.pool));
    QBH_TRY(upload(T.pdiag, &pd, bufs.pool));
    QBH_TRY(upload(T.sdiag, &sd, bufs.pool));
    QBH_TRY(upload(T.eval, &ev, bufs.pool));
    R.pair_ij = pij; R.eoff = eo; R.eout = eu; R.pdiag = pd; R.sdiag = sd; R.eval = ev;
    SectorDev<QuditReprDev> S;
    int64_t *d_pos = nullptr, nchunks = 0;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who, &d_pos, &nchunks));
    const int64_t dim = S.dim;
    if (dim_out) *dim_out = dim;
    if (row_end < 0) row_end = dim;
    if (row_begin >= row_end || row_end > dim) {
        set_error("%s: bad row range [%lld, %lld) of %lld", who, (long long)row_begin, (long long)row_end, (long long)dim);
        return QBH_EINVAL;
    }
    QuditReprDev hR;                      // the device copy holds the pointer to the counting table (sector_tables)
    QBH_HIP_WHO(who, hipMemcpy(&hR, S.R, sizeof(hR), hipMemcpyDeviceToHost));

    MfQuditRepr t;
    t.R = S.R;
    t.tab = S.tab;
    t.cum = hR.cum;
    t.reps = S.reps;
    t.info = S.info;
    t.chunk_pos = d_pos;
    t.dim = dim;
    t.n_tab = (int)tab.size();
    t.n_cum = n_sites * R.tw;
    t.tables_lds = ((size_t)t.n_tab + (size_t)t.n_cum) * 8 <= kMfQreprLdsCap ? 1 : 0;
    const int64_t bytes = (int64_t)(sizeof(QuditReprDev) + tab.size() * 8 + (size_t)t.n_cum * 8 + T.pair_ij.size() * 4 + T.eoff.size() * 4 +
                        T.eout.size() * 4 + T.pdiag.size() * 8 + T.sdiag.size() * 8 + T.eval.size() * 16) +
                          dim * 9 + (nchunks + 1) * 8;      // tables + representatives + info bytes + directory

    const int64_t nrows = row_end - row_begin;
    const int cgrid = mf_qrepr_grid(t, nrows);
    const size_t lds = mf_qrepr_lds_bytes(t);
    int64_t nnz = 0;
    QBH_TRY(sector_count_entries(who, cgrid, &nnz, [&](unsigned long long *d_part) {
        if (t.tables_lds) {
            const hipError_t ce = hipFuncSetAttribute(reinterpret_cast<const void *>(k_mf_qudit_repr_count<true>),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (ce != hipSuccess) return ce;
            hipLaunchKernelGGL(k_mf_qudit_repr_count<true>, dim3(cgrid), dim3(kMfQreprBlock), lds, 0, t, row_begin, row_end, d_part);
        } else {
            hipLaunchKernelGGL(k_mf_qudit_repr_count<false>, dim3(cgrid), dim3(kMfQreprBlock), 0, 0, t, row_begin, row_end, d_part);
        }
        return hipGetLastError();
    }));

    const int rc = adopt_mf(out, 6, &qbh_csr::mfqr, t, bufs.pool, bytes, values_real, nrows, dim, row_begin, nnz, opts);
    if (rc == QBH_OK) bufs.release();     // the handle owns the tables, the representatives and the directory now
    return rc;
}
