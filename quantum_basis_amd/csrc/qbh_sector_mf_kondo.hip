// qbh_sector_mf_kondo.hip -- qbh_mf_kondo_repr (toolkit and the Kondo family: qbh_sector.hpp; words, ranking, terms: qbh_kondo.hpp)
//
// The sector operator of qbh_gen_kondo_repr applied from its basis, without a stored matrix (MfKondoRepr in qbh_internal.hpp).
// What stays in HBM is the representative list (8 B per row), one info byte per row, the directory of the enumeration (8 B per
// 4096 words) and the tables: no row pointers, no columns, no values.  One lane handles one representative row and follows
// kondo_row up to the point where that would call row_add: it splits the word into (u, d, s), walks kd_row_terms in its own
// order, and for each emitted (u', d', s', code) forms the word c, canonicalises it with the byte-sliced translation tables
// (sector_canonical: n_trans x 3 fields x n_chunks table reads), takes the fermion sign of the translation only when it is
// not the identity, finds the position of the representative b and accumulates kondo_repr_value x[b] as the entries arrive.
// An entry that returns to the row's own orbit simply adds to x[i].  Nothing is staged per row, so the limit of 160 entries
// per row of the stored form does not apply, and the order of the sums of a row does not depend on which rows the launch
// covers: a row shard is bit-identical to the same rows of the whole operator.
//
// The position of b is not looked up in the whole list: kd_rank(b) >> 12 (the inverse of the enumeration's kd_unrank;
// ascending words are ascending ranks) names the chunk of 4096 words that holds b, the directory gives the positions of that
// chunk's first and last representatives, and a bisection of at most 12 steps inside those (at most 32 KB, contiguous) ends at
// what sector_find returns from 31 steps over the whole list.
//
// The translation tables and the two counting tables A and binom of KondoDev are always staged in LDS (qbh_kondo_lds.hpp, which
// also chooses between the two workgroup shapes).  The term arrays, the characters and the permutations are read through the
// device copy of KondoReprDev (uniform over the lanes, cached).
#include "qbh_kondo_lds.hpp"
#include "qbh_mf_row.hpp"

namespace qbh {
namespace {

// The compiler reports 85 VGPRs for every instance of the apply kernel (88 allocated: 5 waves per SIMD, 20 per CU) and 0 bytes
// of scratch, so a CU holds at most five workgroups of 256 lanes or one of 1024: 16 or 20 waves per CU in the small shape.
constexpr int kMfKreprPerCuS = 5;                             // VGPR-limited workgroups of 256 lanes per CU

inline size_t mf_krepr_lds_bytes(const MfKondoRepr &t) { return krepr_lds_bytes(t.n_tab); }
inline bool mf_krepr_large(const MfKondoRepr &t) { return krepr_large(t.n_tab); }
inline int mf_krepr_grid(const MfKondoRepr &t, int64_t nrows) { return krepr_grid(t.n_tab, nrows, kMfKreprPerCuS); }

// the terms of the row of representative a (|S_a| = sa, nonzero norm) in the order of kondo_row: sink(position of b, value)
// for every off-diagonal term entry whose target has nonzero norm; returns the diagonal of the row's own word
template <class Sink>
__device__ __forceinline__ d2 krepr_walk(const KondoReprDev &R, const uint64_t *tab, const uint64_t *A, const uint64_t *binom,
                                         const uint64_t *reps, const uint8_t *info, const int64_t *chunk_pos, int64_t dim, uint64_t a,
                                         double sa, Sink sink)
{
    const int nb = R.k.n_sites;
    const uint64_t mlow = (1ULL << nb) - 1ULL;
    return kd_row_terms(R.k, a & mlow, (a >> nb) & mlow, a >> (2 * nb), [&](uint64_t u2, uint64_t d2w, uint64_t s2, int code) {
        const uint64_t c = u2 | (d2w << nb) | (s2 << (2 * nb));
        int g = 0;
        const uint64_t b = sector_canonical(R, tab, c, &g);
        const int pt = g ? sector_parity(R, g, c) : 0;
        const int64_t lo = sector_dir_find(reps, chunk_pos, dim, b, kd_rank(R.k, A, binom, b & mlow, (b >> nb) & mlow, b >> (2 * nb)));
        const uint8_t cj = info[lo];
        if (cj & 0x80) return;            // zero-norm target: dropped
        sink(lo, kondo_repr_value(R, code, g, pt, cj, sa));
    });
}

// y <- alpha H x + beta y + gamma x on rows [row_begin, row_begin + nrows) of the sector: one lane per row, grid-stride over
// a resident grid, every row gathers (no atomics).  Epilogue and partial sums: qbh_mf_row.hpp.
template <bool REALX, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mf_kondo_repr(MfKondoRepr t, MfVec a)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t kr_lds[];
    __shared__ double red[3 * (BLOCK / 64)];
    const KondoReprDev &R = *static_cast<const KondoReprDev *>(t.R);
    const int tid = threadIdx.x;
    const uint64_t *tab, *A, *binom;
    krepr_stage(t.tab, t.n_tab, R.k, kr_lds, BLOCK, tab, A, binom);
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t lrow = (int64_t)blockIdx.x * BLOCK + tid; lrow < a.nrows; lrow += stride) {
        const int64_t grow = a.row_begin + lrow;
        const uint8_t ci = t.info[grow];
        d2 yo, xi;
        mf_row_load<REALX>(a, lrow, grow, yo, xi);
        d2 sum = {0.0, 0.0};
        d2 dg;
        if (ci & 0x80) {                  // zero norm at this momentum: the decoupled row of row_zero_norm
            dg = d2{R.fake_pos + (double)grow / (double)t.dim, 0.0};
        } else {
            dg = krepr_walk(R, tab, A, binom, t.reps, t.info, t.chunk_pos, t.dim, t.reps[grow], (double)(ci & 0x7f),
                            [&](int64_t lo, d2 v) { mf_gather_add<REALX>(a, sum, v, lo); });
        }
        mf_row_finish(a, lrow, sum, dg.x, xi, yo, acc);      // the diagonal of a word is real by construction (kondo_setup drops Im of a number term)
    }
    mf_block_partials<BLOCK>(acc, red, a.partials);
}

// the contributions the apply kernel makes for rows [row_begin, row_end): one diagonal per row and every off-diagonal term
// entry whose target has nonzero norm, before duplicates merge.  One sum per workgroup.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mf_kondo_repr_count(MfKondoRepr t, int64_t row_begin, int64_t row_end, unsigned long long *part)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t kr_lds[];
    __shared__ unsigned long long red[BLOCK / 64];
    const KondoReprDev &R = *static_cast<const KondoReprDev *>(t.R);
    const uint64_t *tab, *A, *binom;
    krepr_stage(t.tab, t.n_tab, R.k, kr_lds, BLOCK, tab, A, binom);
    unsigned long long c = 0;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * BLOCK + threadIdx.x; row < row_end; row += stride) {
        const uint8_t ci = t.info[row];
        c += 1;
        if (!(ci & 0x80))
            (void)krepr_walk(R, tab, A, binom, t.reps, t.info, t.chunk_pos, t.dim, t.reps[row], (double)(ci & 0x7f),
                             [&](int64_t, d2) { c += 1; });
    }
    mf_block_count<BLOCK>(c, red, part);
}

}  // namespace

int launch_mf_kondo_repr(const MfKondoRepr &t, const MfVec &a, hipStream_t s, int *nparts_out)
{
    const size_t lds = mf_krepr_lds_bytes(t);
    const int g = mf_krepr_grid(t, a.nrows);
    const bool rx = a.xr != nullptr;
    if (mf_krepr_large(t)) {
        if (rx) QBH_HIP(krepr_launch(k_mf_kondo_repr<true, kMfKreprBlockL>, g, kMfKreprBlockL, lds, s, t, a));
        else    QBH_HIP(krepr_launch(k_mf_kondo_repr<false, kMfKreprBlockL>, g, kMfKreprBlockL, lds, s, t, a));
    } else {
        if (rx) QBH_HIP(krepr_launch(k_mf_kondo_repr<true, kMfKreprBlockS>, g, kMfKreprBlockS, lds, s, t, a));
        else    QBH_HIP(krepr_launch(k_mf_kondo_repr<false, kMfKreprBlockS>, g, kMfKreprBlockS, lds, s, t, a));
    }
    if (nparts_out) *nparts_out = g;
    return QBH_OK;
}

}  // namespace qbh

extern "C" int qbh_mf_kondo_repr(qbh_csr **out, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites,
                                 const qbh_z *amp_up, const qbh_z *amp_dn, double U, const double *kz, const double *kxy,
                                 int n_sbonds, const int32_t *sbond_sites, const double *bz, const double *bxy, int n_trans,
                                 const int32_t *perms, const double *chars, double fake_pos, int64_t row_begin, int64_t row_end,
                                 int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    const char *who = "qbh_mf_kondo_repr";
    if (!out) {
        set_error("%s: out is NULL", who);
        return QBH_EINVAL;
    }
    std::vector<KondoReprDev> rr(1);
    KondoReprDev &R = rr[0];
    memset(&R, 0, sizeof(R));
    const int max_row = kondo_setup(who, n_sites, n_elec, two_sz, n_terms, term_sites, amp_up, amp_dn, U, kz, kxy, n_sbonds,
                                    sbond_sites, bz, bxy, R.k, true);     // no row is staged: any row length
    if (max_row <= 0) return max_row;
    std::vector<uint64_t> tab;
    QBH_TRY(kondo_symmetry(R, tab, n_trans, perms, chars, who));
    QBH_TRY(kondo_invariant(who, R.k, n_trans, perms));
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

    // real values: every merged hop amplitude real and every character real (kxy, bxy and the diagonal are real by
    // construction).  A character computed as exp(-i k.t) at k = pi carries sin(pi t), which rounds to at most
    // 64 pi 2^-53 = 2.2e-14 for the 64 translations allowed: an imaginary part below 1e-13 is that rounding and is dropped,
    // so that the real and the complex kernel apply the same numbers.
    bool values_real = true;
    for (int t = 0; t < R.k.n_terms; ++t)
        if (R.k.aup[t][1] != 0.0 || R.k.adn[t][1] != 0.0) values_real = false;
    for (int g = 0; g < n_trans; ++g)
        if (std::fabs(R.chr[2 * g + 1]) > 1e-13) values_real = false;
    if (values_real)
        for (int g = 0; g < n_trans; ++g) R.chr[2 * g + 1] = 0.0;

    R.fake_pos = fake_pos;
    DevBufs bufs;
    SectorDev<KondoReprDev> S;
    int64_t *d_pos = nullptr, nchunks = 0;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who, &d_pos, &nchunks));
    const int64_t dim = S.dim;
    if (dim_out) *dim_out = dim;
    if (row_end < 0) row_end = dim;
    if (row_begin >= row_end || row_end > dim) {
        set_error("%s: bad row range [%lld, %lld) of %lld", who, (long long)row_begin, (long long)row_end, (long long)dim);
        return QBH_EINVAL;
    }

    MfKondoRepr t;
    t.R = S.R;
    t.tab = S.tab;
    t.reps = S.reps;
    t.info = S.info;
    t.chunk_pos = d_pos;
    t.dim = dim;
    t.n_tab = (int)tab.size();
    if (mf_krepr_lds_bytes(t) > kMfKreprLdsMax) {
        set_error("%s: internal: %d table words", who, t.n_tab);
        return QBH_EHIP;
    }
    const int64_t bytes = (int64_t)(sizeof(KondoReprDev) + tab.size() * 8) + dim * 9 + (nchunks + 1) * 8;      // tables + representatives + info bytes + directory

    const int64_t nrows = row_end - row_begin;
    const int cgrid = mf_krepr_grid(t, nrows);
    const size_t lds = mf_krepr_lds_bytes(t);
    int64_t nnz = 0;
    QBH_TRY(sector_count_entries(who, cgrid, &nnz, [&](unsigned long long *d_part) {
        return mf_krepr_large(t)
                   ? krepr_launch(k_mf_kondo_repr_count<kMfKreprBlockL>, cgrid, kMfKreprBlockL, lds, (hipStream_t)0, t, row_begin, row_end, d_part)
                   : krepr_launch(k_mf_kondo_repr_count<kMfKreprBlockS>, cgrid, kMfKreprBlockS, lds, (hipStream_t)0, t, row_begin, row_end, d_part);
    }));

    const int rc = adopt_mf(out, 7, &qbh_csr::mfkr, t, bufs.pool, bytes, values_real, nrows, dim, row_begin, nnz, opts);
    if (rc == QBH_OK) bufs.release();     // the handle owns the tables, the representatives and the directory now
    return rc;
}
