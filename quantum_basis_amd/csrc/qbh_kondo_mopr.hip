// qbh_kondo_mopr.hip -- operators that take a Kondo-lattice vector to another (n_elec, two_sz): c_{q,sigma}, c^dag_{q,sigma}
// and the spin flips S^+-_q of the electrons, of the local spins or of both, in the full sector (qbh_mopr_kondo_dev) and
// between momentum sectors (qbh_mopr_kondo_repr_dev).  Words, ranking and the one-site elements (KondoSiteOp): qbh_kondo.hpp;
// the sector toolkit: qbh_sector.hpp; the staged tables and the two workgroup shapes: qbh_kondo_lds.hpp.
//
// Both kernels gather per TARGET row: one lane per row, grid-stride over a resident grid, the sites walked ascending (the
// electron part of a spin flip before the local-spin part), no atomics, every element of the output written exactly once.
// A row's sum depends on nothing but the row, so two runs are bit-identical.
//   full sector   the lane unranks its target word with the target's counting table, applies KondoSiteOp, ranks the source
//                 word in the SOURCE sector and reads x_old there.  A_old, A_new and binom (3 x 22 x 22 x 8 B = 11,616 B) sit
//                 in LDS.  Rows and ranks are 64-bit.
//   sectors       the row formula at the head of qbh_sector_mopr.hip,
//                     <b, k'| O |a, k> = sum_s w_s sigma(g*) conj(chi_old(g*)) sqrt(|S_a| / |S_b|),   a = g* c,
//                 with the translation tables and the SOURCE's A and binom in LDS and the position of a found through the
//                 directory of the source's enumeration (kd_rank(a) >> 12 names the chunk; at most 12 bisection steps), as
//                 k_mf_kondo_repr finds its columns.  Zero-norm targets receive 0, zero-norm sources are skipped.
// Both entry points: argument checks -> kondo_shape of source and target -> symmetry -> coefficient character -> sector sizes
// -> only then the device is looked for.
#include "qbh_kondo_lds.hpp"

namespace qbh {
namespace {

// ---- full sector ----
// The compiler reports 46 VGPRs and 0 bytes of scratch: eight workgroups of 256 lanes per CU (the wave limit), 93 KB of LDS.
constexpr int kKondoMoprBlock = 256;
constexpr int kKondoMoprPerCu = 8;

__global__ __launch_bounds__(kKondoMoprBlock) void k_mopr_kondo(const KondoDev *Kold, const KondoDev *Knew, KondoSiteOp op,
                                                                const d2 *x_old, d2 *y_new)
{
    __shared__ uint64_t lds[3 * kKondoTabEntries];
    const KondoDev &Ko = *Kold, &Kn = *Knew;
    for (int k = threadIdx.x; k < kKondoTabEntries; k += kKondoMoprBlock) {
        lds[k] = Ko.A[k];
        lds[kKondoTabEntries + k] = Kn.A[k];
        lds[2 * kKondoTabEntries + k] = Kn.binom[k];
    }
    __syncthreads();
    const uint64_t *A_old = lds, *A_new = lds + kKondoTabEntries, *binom = lds + 2 * kKondoTabEntries;
    const int parts = op.parts();
    const uint64_t stride = (uint64_t)gridDim.x * kKondoMoprBlock;
    for (uint64_t row = (uint64_t)blockIdx.x * kKondoMoprBlock + threadIdx.x; row < Kn.total; row += stride) {
        uint64_t bu, bd, bs, ru, rd;
        kd_unrank(Kn, A_new, binom, row, &bu, &bd, &bs, &ru, &rd);
        double ar = 0.0, ai = 0.0;
        for (int s = 0; s < op.n_sites; ++s)
            for (int part = 0; part < parts; ++part) {
                uint64_t cu, cd, cs;
                d2 w;
                if (!op(bu, bd, bs, s, part, cu, cd, cs, w)) continue;
                const d2 x = x_old[kd_rank(Ko, A_old, binom, cu, cd, cs)];
                ar += w.x * x.x - w.y * x.y;
                ai += w.x * x.y + w.y * x.x;
            }
        y_new[row] = d2{ar, ai};
    }
}

// ---- momentum sectors ----
// The compiler reports 60 VGPRs for both shapes and 0 bytes of scratch: the registers admit eight workgroups of 256 lanes per
// CU.  The resident grid counts seven: on the rings this kernel is meant for the tables leave room for seven (12 sites,
// 20,032 B) or five (13 sites, 27,712 B) anyway, so the cap matters on small lattices alone, where an eighth workgroup would
// only share the same gathers among more waves.
constexpr int kKondoMoprReprPerCuS = 7;

struct KondoMoprRepr {
    const KondoReprDev *Ro;               // the SOURCE sector: counting tables, characters, permutations
    const uint64_t *tab;                  // [n_tab] translation tables (the same for both sectors)
    const uint64_t *reps_old, *reps_new;  // representatives, ascending
    const uint8_t *info_old, *info_new;   // |S| | zero-norm << 7
    const int64_t *chunk_pos_old;         // directory of the source's enumeration
    int64_t dim_old, dim_new;
    int n_tab;
};

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mopr_kondo_repr(KondoMoprRepr t, KondoSiteOp op, const d2 *x_old, d2 *y_new)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t km_lds[];
    const KondoReprDev &R = *t.Ro;
    const uint64_t *tab, *A, *binom;
    krepr_stage(t.tab, t.n_tab, R.k, km_lds, BLOCK, tab, A, binom);
    const int nb = R.k.n_sites, parts = op.parts();
    const uint64_t mlow = (1ULL << nb) - 1ULL;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < t.dim_new; i += stride) {
        const uint8_t cb = t.info_new[i];
        double ar = 0.0, ai = 0.0;
        if (!(cb & 0x80)) {
            const uint64_t b = t.reps_new[i];
            const uint64_t bu = b & mlow, bd = (b >> nb) & mlow, bs = b >> (2 * nb);
            const double sb = (double)(cb & 0x7f);
            for (int s = 0; s < nb; ++s)
                for (int part = 0; part < parts; ++part) {
                    uint64_t cu, cd, cs;
                    d2 w;
                    if (!op(bu, bd, bs, s, part, cu, cd, cs, w)) continue;
                    const uint64_t c = cu | (cd << nb) | (cs << (2 * nb));
                    int g = 0;
                    const uint64_t a = sector_canonical(R, tab, c, &g);
                    const int pt = g ? sector_parity(R, g, c) : 0;
                    const int64_t lo = sector_dir_find(t.reps_old, t.chunk_pos_old, t.dim_old, a,
                                                       kd_rank(R.k, A, binom, a & mlow, (a >> nb) & mlow, a >> (2 * nb)));
                    const uint8_t ca = t.info_old[lo];
                    if (ca & 0x80) continue;
                    const double f = (pt ? -1.0 : 1.0) * sqrt((double)(ca & 0x7f) / sb);
                    const double xr = f * R.chr[2 * g], xi = -f * R.chr[2 * g + 1];
                    const double wr = w.x * xr - w.y * xi, wi = w.x * xi + w.y * xr;
                    const d2 x = x_old[lo];
                    ar += wr * x.x - wi * x.y;
                    ai += wr * x.y + wi * x.x;
                }
        }
        y_new[i] = d2{ar, ai};
    }
}

// ---- the host side both entry points share ----
// argument checks and the two shapes; fills the one-site operator
int kondo_mopr_setup(const char *who, int n_sites, int n_elec_old, int two_sz_old, int op, const qbh_z *coef_elec, const qbh_z *coef_spin,
                     const qbh_z *d_vec_old, qbh_z *d_vec_new, KondoDev &Ko, KondoDev &Kn, KondoSiteOp &O)
{
    if (op < 0 || op >= kKondoMoprOps) {
        set_error("%s: op = %d outside [0, %d]", who, op, kKondoMoprOps - 1);
        return QBH_EINVAL;
    }
    if (op < 4 && (!coef_elec || coef_spin)) {
        set_error("%s: op %d (c / c^dag) takes coef_elec alone: coef_spin must be NULL", who, op);
        return QBH_EINVAL;
    }
    if (op >= 4 && !coef_elec && !coef_spin) {
        set_error("%s: op %d (spin flip) needs coef_elec, coef_spin or both", who, op);
        return QBH_EINVAL;
    }
    if (!d_vec_old || !d_vec_new) {
        set_error("%s: invalid argument (a vector is NULL)", who);
        return QBH_EINVAL;
    }
    QBH_TRY(kondo_shape(who, n_sites, n_elec_old, two_sz_old, Ko));
    int n_elec_new = 0, two_sz_new = 0;
    kondo_mopr_target(op, n_elec_old, two_sz_old, &n_elec_new, &two_sz_new);
    if (n_elec_new < 0 || n_elec_new > 2 * n_sites || kondo_shape(who, n_sites, n_elec_new, two_sz_new, Kn) != QBH_OK) {
        set_error("%s: the target sector does not exist (op %d from n_elec = %d, two_sz = %d on %d sites leads to n_elec = %d, two_sz = %d)",
                  who, op, n_elec_old, two_sz_old, n_sites, n_elec_new, two_sz_new);
        return QBH_EINVAL;
    }
    memset(&O, 0, sizeof(O));
    O.n_sites = n_sites;
    O.op = op;
    for (int s = 0; s < n_sites; ++s) {
        if (coef_elec) {
            O.ce_re[s] = coef_elec[s].re;
            O.ce_im[s] = coef_elec[s].im;
        }
        if (coef_spin) {
            O.cs_re[s] = coef_spin[s].re;
            O.cs_im[s] = coef_spin[s].im;
        }
    }
    return QBH_OK;
}

int kondo_mopr_words(const char *who, const KondoDev &K)
{
    if (K.total >= (1ULL << 40)) {
        set_error("%s: sector too large (%llu words; below 2^40 are supported)", who, (unsigned long long)K.total);
        return QBH_EUNSUPP;
    }
    return QBH_OK;
}

int kondo_mopr_device()
{
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    return QBH_OK;
}

}  // namespace
}  // namespace qbh

extern "C" int qbh_mopr_kondo_dev(int n_sites, int n_elec_old, int two_sz_old, int op, const qbh_z *coef_elec, const qbh_z *coef_spin,
                                  const qbh_z *d_vec_old, qbh_z *d_vec_new, int64_t *dim_old_out, int64_t *dim_new_out, void *stream)
{
    using namespace qbh;
    const char *who = "qbh_mopr_kondo_dev";
    std::vector<KondoDev> kk(2);
    KondoSiteOp O;
    QBH_TRY(kondo_mopr_setup(who, n_sites, n_elec_old, two_sz_old, op, coef_elec, coef_spin, d_vec_old, d_vec_new, kk[0], kk[1], O));
    QBH_TRY(kondo_mopr_words(who, kk[0]));
    QBH_TRY(kondo_mopr_words(who, kk[1]));
    if (dim_old_out) *dim_old_out = (int64_t)kk[0].total;
    if (dim_new_out) *dim_new_out = (int64_t)kk[1].total;
    QBH_TRY(kondo_mopr_device());                          // every refusal above comes before the device is looked for
    DevBufs bufs;
    KondoDev *d_K = nullptr;
    QBH_TRY(upload(kk, &d_K, bufs.pool));
    const int64_t dim_new = (int64_t)kk[1].total;
    const int64_t nblk = (dim_new + kKondoMoprBlock - 1) / kKondoMoprBlock;
    const int grid = (int)std::min<int64_t>(nblk, (int64_t)device_cu_count() * kKondoMoprPerCu);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mopr_kondo, dim3(grid), dim3(kKondoMoprBlock), 0, st, d_K, d_K + 1, O, reinterpret_cast<const d2 *>(d_vec_old),
                       reinterpret_cast<d2 *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipStreamSynchronize(st));
    return QBH_OK;
}

extern "C" int qbh_mopr_kondo_repr_dev(int n_sites, int n_elec_old, int two_sz_old, int op, int n_trans, const int32_t *perms,
                                       const double *chars_old, const qbh_z *coef_elec, const qbh_z *coef_spin, const qbh_z *d_vec_old,
                                       qbh_z *d_vec_new, int64_t *dim_old_out, int64_t *dim_new_out, void *stream)
{
    using namespace qbh;
    const char *who = "qbh_mopr_kondo_repr_dev";
    std::vector<KondoReprDev> rr(2);
    memset(rr.data(), 0, 2 * sizeof(KondoReprDev));
    KondoReprDev &Ro = rr[0], &Rn = rr[1];
    KondoSiteOp O;
    QBH_TRY(kondo_mopr_setup(who, n_sites, n_elec_old, two_sz_old, op, coef_elec, coef_spin, d_vec_old, d_vec_new, Ro.k, Rn.k, O));
    std::vector<uint64_t> tab, tab_n;
    QBH_TRY(kondo_symmetry(Ro, tab, n_trans, perms, chars_old, who));
    const qbh_z *sets[2];
    int n_sets = 0;
    if (coef_elec) sets[n_sets++] = coef_elec;
    if (coef_spin) sets[n_sets++] = coef_spin;
    std::vector<std::complex<double>> eta((size_t)n_trans);
    QBH_TRY(coef_character(who, n_sites, n_trans, perms, sets, n_sets, eta.data()));
    std::vector<double> chars_new((size_t)2 * n_trans);
    for (int g = 0; g < n_trans; ++g) {
        const std::complex<double> chi = std::complex<double>(chars_old[2 * g], chars_old[2 * g + 1]) * eta[(size_t)g];
        chars_new[2 * g] = chi.real();
        chars_new[2 * g + 1] = chi.imag();
    }
    QBH_TRY(kondo_symmetry(Rn, tab_n, n_trans, perms, chars_new.data(), who));     // the same tables: they depend on perms alone
    QBH_TRY(kondo_mopr_words(who, Ro.k));
    QBH_TRY(kondo_mopr_words(who, Rn.k));
    QBH_TRY(kondo_mopr_device());                          // every refusal above comes before the device is looked for

    DevBufs bufs;
    SectorDev<KondoReprDev> So, Sn;
    int64_t *d_pos = nullptr, nchunks = 0;
    QBH_TRY(sector_enumerate(Ro, tab, bufs.pool, So, who, &d_pos, &nchunks));
    QBH_TRY(sector_enumerate(Rn, tab_n, bufs.pool, Sn, who));
    KondoMoprRepr t;
    t.Ro = So.R;
    t.tab = So.tab;
    t.reps_old = So.reps;
    t.info_old = So.info;
    t.chunk_pos_old = d_pos;
    t.dim_old = So.dim;
    t.reps_new = Sn.reps;
    t.info_new = Sn.info;
    t.dim_new = Sn.dim;
    t.n_tab = (int)tab.size();
    const size_t lds = krepr_lds_bytes(t.n_tab);
    if (lds > kMfKreprLdsMax) {
        set_error("%s: internal: %d table words", who, t.n_tab);
        return QBH_EHIP;
    }
    const int grid = krepr_grid(t.n_tab, t.dim_new, kKondoMoprReprPerCuS);
    hipStream_t st = (hipStream_t)stream;
    const d2 *x = reinterpret_cast<const d2 *>(d_vec_old);
    d2 *y = reinterpret_cast<d2 *>(d_vec_new);
    if (krepr_large(t.n_tab)) QBH_HIP_WHO(who, krepr_launch(k_mopr_kondo_repr<kMfKreprBlockL>, grid, kMfKreprBlockL, lds, st, t, O, x, y));
    else                      QBH_HIP_WHO(who, krepr_launch(k_mopr_kondo_repr<kMfKreprBlockS>, grid, kMfKreprBlockS, lds, st, t, O, x, y));
    QBH_HIP_WHO(who, hipStreamSynchronize(st));
    if (dim_old_out) *dim_old_out = So.dim;
    if (dim_new_out) *dim_new_out = Sn.dim;
    return QBH_OK;
}
