// qbh_sector_mopr.hip -- operators that act between momentum sectors (moprXvec_repr, src/model.cc:1715-1846): S^z_q and
// S^-+_q of spin-1/2 sites, N_q / S^z_q and c_q / c^dag_q of the Hubbard family, O_q of d-level sites, the diagonal
// operators of the Kondo lattice (toolkit and families: qbh_sector.hpp).
//
// All of them are O = sum_s c_s O_s with c_{g(s)} = eta(g) c_s, so O T_g = eta(g) T_g O and O takes the sector with
// characters chi to the one with chi' = chi eta.  The vectors are indexed like the rows of the sector operators (all
// representatives, ascending).  Two kernels serve them:
//   diagonal O_s        O |a, k> = z_a |a, k'>, z_a evaluated on the representative itself (the stabiliser, hence the
//                       normalisation, does not depend on the momentum; fermion signs sit inside T_g on both sides)
//   one-site moves      gathered per TARGET representative b with the row formula of the sector operators,
//                         <b, k'| O |a, k> = sum_s c_s <b|O_s|c> sigma(g*) conj(chi(g*)) sqrt(|S_a| / |S_b|),   a = g* c,
//                       chi the SOURCE characters: no atomics, every element of the output written exactly once
// Representatives whose norm vanishes at the target momentum get 0, sources whose norm vanishes are skipped.
// Every entry point: argument checks -> symmetry -> character check where the target characters follow from the
// coefficients -> sector sizes -> only then the device is looked for -> enumerate -> one kernel -> synchronise.
#include "qbh_sector.hpp"

namespace qbh {
namespace {

// ---- z_a of the diagonal operators: the coefficient tables and the sum over the sites of a word ----
struct SpinSzSum {                        // sum_s c_s S^z_s, bit set = spin down
    int n_sites;
    double re[64], im[64];
    __device__ __forceinline__ void operator()(uint64_t s, double &zr, double &zi) const
    {
        for (int site = 0; site < n_sites; ++site) {
            const double sz = ((s >> site) & 1ULL) ? -0.5 : 0.5;
            zr += sz * re[site];
            zi += sz * im[site];
        }
    }
};

struct HubCoef { double up_re[32], up_im[32], dn_re[32], dn_im[32]; };
struct HubDensitySum {                    // sum_s ( c_up[s] n_{s,up} + c_dn[s] n_{s,dn} ): the up particles, then the down particles
    int n_sites;
    HubCoef cf;
    __device__ __forceinline__ void operator()(uint64_t a, double &zr, double &zi) const
    {
        uint64_t u = a & ((1ULL << n_sites) - 1ULL), d = a >> n_sites;
        while (u) {
            const int s = __ffsll((long long)u) - 1;
            u &= u - 1;
            zr += cf.up_re[s];
            zi += cf.up_im[s];
        }
        while (d) {
            const int s = __ffsll((long long)d) - 1;
            d &= d - 1;
            zr += cf.dn_re[s];
            zi += cf.dn_im[s];
        }
    }
};

struct KondoDiagSum {                     // sum_s ( c_up[s] n_{s,up} + c_dn[s] n_{s,dn} + c_sp[s] S^z_s ), site by site
    int n_sites;
    double up_re[kKondoMaxSites], up_im[kKondoMaxSites], dn_re[kKondoMaxSites], dn_im[kKondoMaxSites], sp_re[kKondoMaxSites],
        sp_im[kKondoMaxSites];
    __device__ __forceinline__ void operator()(uint64_t a, double &zr, double &zi) const
    {
        const uint64_t mlow = (1ULL << n_sites) - 1ULL;
        const uint64_t u = a & mlow, d = (a >> n_sites) & mlow, sp = a >> (2 * n_sites);
        for (int s = 0; s < n_sites; ++s) {
            const double nu = (double)((u >> s) & 1ULL), nd = (double)((d >> s) & 1ULL);
            const double sz = ((sp >> s) & 1ULL) ? -0.5 : 0.5;
            zr += nu * up_re[s] + nd * dn_re[s] + sz * sp_re[s];
            zi += nu * up_im[s] + nd * dn_im[s] + sz * sp_im[s];
        }
    }
};

// y_new[i] = z(reps[i]) * x_old[i]; info_new[] comes from the enumeration with the TARGET characters
template <class Z>
__global__ __launch_bounds__(256) void k_sector_apply_diag(const uint64_t *reps, const uint8_t *info_new, int64_t dim, Z z, const d2 *x_old,
                                                           d2 *y_new)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += stride) {
        d2 y = {0.0, 0.0};
        if (!(info_new[i] & 0x80)) {
            double zr = 0.0, zi = 0.0;
            z(reps[i], zr, zi);
            const d2 x = x_old[i];
            y = d2{zr * x.x - zi * x.y, zr * x.y + zi * x.x};
        }
        y_new[i] = y;
    }
}

// ---- <b|O_s|c> of the one-site moves: for target word b and site s, the source word c and w = c_s <b|O_s|c>, or false ----
struct SpinFlip {                         // S^- (lower: the target's spin s is down, bit 1) / S^+; the element is 1
    int n_sites, lower;
    double re[64], im[64];
    __device__ __forceinline__ bool operator()(uint64_t b, int s, uint64_t &c, d2 &w) const
    {
        const bool down = (b >> s) & 1ULL;
        if (lower ? !down : down) return false;
        c = b ^ (1ULL << s);
        w = d2{re[s], im[s]};
        return true;
    }
};

// c_{s,sigma} (create = 0) / c^dag_{s,sigma} (create = 1).  Either way b and c differ in the particle (s, sigma) alone, and
// the element is (-1)^(operators left of (s, sigma) in the operator string "all up ascending, then all down ascending"):
// the particles of the species below s, and for the down species the whole up block, which b and c share.
struct HubFermion {
    int n_sites, species, create;
    double re[32], im[32];
    __device__ __forceinline__ bool operator()(uint64_t b, int s, uint64_t &c, d2 &w) const
    {
        const uint64_t bu = b & ((1ULL << n_sites) - 1ULL), bd = b >> n_sites;
        const uint64_t occ = species ? bd : bu;
        const bool has = (occ >> s) & 1ULL;
        if ((create ? !has : has) || (re[s] == 0.0 && im[s] == 0.0)) return false;
        const int par = ((species ? __popcll(bu) : 0) + __popcll(occ & ((1ULL << s) - 1ULL))) & 1;
        c = b ^ (1ULL << (species ? s + n_sites : s));
        w = par ? d2{-re[s], -im[s]} : d2{re[s], im[s]};
        return true;
    }
};

struct QuditShift {                       // the level of site s raised by dq, times local[l' = l + dq][l]
    int n_sites, d, bits, dq;
    QuditMopr cf;
    __device__ __forceinline__ bool operator()(uint64_t b, int s, uint64_t &c, d2 &w) const
    {
        const int l = qd_level(b, bits, s), ls = l - dq;
        if (ls < 0 || ls >= d) return false;
        const double lr = cf.la[l], li = cf.lb[l];
        if ((lr == 0.0 && li == 0.0) || (cf.ca[s] == 0.0 && cf.cb[s] == 0.0)) return false;
        const uint64_t field = (1ULL << bits) - 1ULL;
        c = (b & ~(field << (s * bits))) | ((uint64_t)ls << (s * bits));
        w = d2{cf.ca[s] * lr - cf.cb[s] * li, cf.ca[s] * li + cf.cb[s] * lr};
        return true;
    }
};

// one lane per target representative; Rold carries the characters of the SOURCE sector (see the head of the file)
template <class Dev, class Op>
__global__ __launch_bounds__(256) void k_sector_apply_gather(const Dev *Rold, const uint64_t *tab, const uint64_t *reps_old,
                                                             const uint8_t *info_old, int64_t dim_old, const uint64_t *reps_new,
                                                             const uint8_t *info_new, int64_t dim_new, Op op, const d2 *x_old, d2 *y_new)
{
    const Dev &R = *Rold;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim_new; i += stride) {
        const uint8_t cb = info_new[i];
        double ar = 0.0, ai = 0.0;
        if (!(cb & 0x80)) {
            const uint64_t b = reps_new[i];
            const double sb = (double)(cb & 0x7f);
            for (int s = 0; s < op.n_sites; ++s) {
                uint64_t c;
                d2 w;
                if (!op(b, s, c, w)) continue;
                int g = 0;
                const uint64_t a = sector_canonical(R, tab, c, &g);
                const int pt = g ? sector_parity(R, g, c) : 0;
                const int64_t lo = sector_find(reps_old, dim_old, a);
                const uint8_t ca = info_old[lo];
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

// ---- the host side every entry point shares ----
int need_device()
{
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    return QBH_OK;
}

template <class Dev>
int sector_fits(const Dev &R, const char *who)
{
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    return sector_words(R, ctab, &nstates, who);
}

template <class Dev, class Z>
int sector_apply_diag(const char *who, const Dev &R, const std::vector<uint64_t> &tab, const Z &z, const qbh_z *d_vec_old,
                      qbh_z *d_vec_new, int64_t *dim_out)
{
    QBH_TRY(sector_fits(R, who));                          // every refusal comes before the device is looked for
    QBH_TRY(need_device());
    DevBufs bufs;
    SectorDev<Dev> S;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who));
    hipLaunchKernelGGL(k_sector_apply_diag<Z>, dim3(blas_grid(S.dim)), dim3(256), 0, 0, S.reps, S.info, S.dim, z,
                       reinterpret_cast<const d2 *>(d_vec_old), reinterpret_cast<d2 *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    if (dim_out) *dim_out = S.dim;
    return QBH_OK;
}

template <class Dev, class Op>
int sector_apply_gather(const char *who, const Dev &Ro, const std::vector<uint64_t> &tab_o, const Dev &Rn,
                        const std::vector<uint64_t> &tab_n, const Op &op, const qbh_z *d_vec_old, qbh_z *d_vec_new,
                        int64_t *dim_old_out, int64_t *dim_new_out, hipStream_t st)
{
    QBH_TRY(sector_fits(Ro, who));                         // every refusal comes before the device is looked for
    QBH_TRY(sector_fits(Rn, who));
    QBH_TRY(need_device());
    DevBufs bufs;
    SectorDev<Dev> So, Sn;
    QBH_TRY(sector_enumerate(Ro, tab_o, bufs.pool, So, who));
    QBH_TRY(sector_enumerate(Rn, tab_n, bufs.pool, Sn, who));
    hipLaunchKernelGGL((k_sector_apply_gather<Dev, Op>), dim3(blas_grid(Sn.dim)), dim3(256), 0, st, So.R, So.tab, So.reps, So.info, So.dim,
                       Sn.reps, Sn.info, Sn.dim, op, reinterpret_cast<const d2 *>(d_vec_old), reinterpret_cast<d2 *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipStreamSynchronize(st));
    if (dim_old_out) *dim_old_out = So.dim;
    if (dim_new_out) *dim_new_out = Sn.dim;
    return QBH_OK;
}

}  // namespace
}  // namespace qbh

// S^z_q of spin-1/2 sites, with the characters of the TARGET momentum
extern "C" int qbh_mopr_sz_repr_dev(int n_sites, int n_dn, int n_trans, const int32_t *perms, const double *chars_new,
                                    const qbh_z *coef, const qbh_z *d_vec_old, qbh_z *d_vec_new, int64_t *dim_out)
{
    using namespace qbh;
    const char *who = "qbh_mopr_sz_repr_dev";
    if (!perms || !chars_new || !coef || !d_vec_old || !d_vec_new || n_sites <= 0 || n_sites > 62 || n_dn < 0 || n_dn > n_sites ||
        n_dn > 33 || n_trans < 1 || n_trans > kReprMaxTrans) {
        set_error("qbh_mopr_sz_repr_dev: invalid argument");
        return QBH_EINVAL;
    }
    std::vector<ReprDev> rr(1);
    std::vector<uint64_t> tab;
    QBH_TRY(repr_symmetry(rr[0], tab, n_sites, n_dn, n_trans, perms, chars_new, who));
    SpinSzSum z{};
    z.n_sites = n_sites;
    for (int s = 0; s < n_sites; ++s) {
        z.re[s] = coef[s].re;
        z.im[s] = coef[s].im;
    }
    return sector_apply_diag(who, rr[0], tab, z, d_vec_old, d_vec_new, dim_out);
}

// S^-_q (kind -1: n_dn -> n_dn + 1) and S^+_q (kind +1: n_dn -> n_dn - 1) of spin-1/2 sites
extern "C" int qbh_mopr_flip_repr_dev(int n_sites, int n_dn_old, int kind, int n_trans, const int32_t *perms, const double *chars_old,
                                      const double *chars_new, const qbh_z *coef, const qbh_z *d_vec_old, qbh_z *d_vec_new,
                                      int64_t *dim_old_out, int64_t *dim_new_out)
{
    using namespace qbh;
    const char *who = "qbh_mopr_flip_repr_dev";
    const int n_new = n_dn_old - kind;
    if (!perms || !chars_old || !chars_new || !coef || !d_vec_old || !d_vec_new || (kind != -1 && kind != 1) || n_sites <= 0 ||
        n_sites > 62 || n_dn_old < 0 || n_dn_old > n_sites || n_new < 0 || n_new > n_sites || n_dn_old > 33 || n_new > 33 || n_trans < 1 ||
        n_trans > kReprMaxTrans) {
        set_error("qbh_mopr_flip_repr_dev: invalid argument");
        return QBH_EINVAL;
    }
    std::vector<ReprDev> rr(2);
    std::vector<uint64_t> tab_o, tab_n;
    QBH_TRY(repr_symmetry(rr[0], tab_o, n_sites, n_dn_old, n_trans, perms, chars_old, who));
    QBH_TRY(repr_symmetry(rr[1], tab_n, n_sites, n_new, n_trans, perms, chars_new, who));
    SpinFlip op{};
    op.n_sites = n_sites;
    op.lower = kind < 0 ? 1 : 0;
    for (int s = 0; s < n_sites; ++s) {
        op.re[s] = coef[s].re;
        op.im[s] = coef[s].im;
    }
    return sector_apply_gather(who, rr[0], tab_o, rr[1], tab_n, op, d_vec_old, d_vec_new, dim_old_out, dim_new_out, nullptr);
}

// O_q = sum_s c_s O_s of d-level sites, O = local[l'][l] raising the level by dq; the target characters chi_old * eta follow
// from coef
extern "C" int qbh_mopr_qudit_repr_dev(int n_sites, int d, int total_old, int dq, int n_trans, const int32_t *perms,
                                       const double *chars_old, const qbh_z *coef, const qbh_z *local, const qbh_z *d_vec_old,
                                       qbh_z *d_vec_new, int64_t *dim_old_out, int64_t *dim_new_out, void *stream)
{
    using namespace qbh;
    const char *who = "qbh_mopr_qudit_repr_dev";
    QBH_TRY(qudit_check_shape(who, n_sites, d));
    const int total_new = total_old + dq;
    if (!perms || !chars_old || !coef || !local || !d_vec_old || !d_vec_new || total_old < 0 || total_old > n_sites * (d - 1) ||
        total_new < 0 || total_new > n_sites * (d - 1) || n_trans < 1 || n_trans > kReprMaxTrans) {
        set_error("%s: invalid argument (charge %d -> %d of at most %d, 1 .. %d translations)", who, total_old, total_new,
                  n_sites * (d - 1), kReprMaxTrans);
        return QBH_EINVAL;
    }
    QuditShift op{};
    op.n_sites = n_sites;
    op.d = d;
    op.bits = bits_per_level(d);
    op.dq = dq;
    for (int lp = 0; lp < d; ++lp)
        for (int l = 0; l < d; ++l) {
            const qbh_z z = local[lp * d + l];
            if (z.re == 0.0 && z.im == 0.0) continue;
            if (lp != l + dq) {
                set_error("%s: local[%d][%d] is nonzero but does not change the level by dq = %d", who, lp, l, dq);
                return QBH_EINVAL;
            }
            op.cf.la[lp] = z.re;
            op.cf.lb[lp] = z.im;
        }
    for (int s = 0; s < n_sites; ++s) {
        op.cf.ca[s] = coef[s].re;
        op.cf.cb[s] = coef[s].im;
    }
    QuditReprDev Ro, Rn;
    std::vector<uint64_t> tab_o, tab_n;
    QBH_TRY(qrepr_symmetry(Ro, tab_o, n_sites, d, total_old, n_trans, perms, chars_old, who));
    std::vector<std::complex<double>> eta((size_t)n_trans);
    QBH_TRY(coef_character(who, n_sites, n_trans, perms, &coef, 1, eta.data()));
    std::vector<double> chars_new((size_t)2 * n_trans);
    for (int g = 0; g < n_trans; ++g) {
        const std::complex<double> chi = std::complex<double>(chars_old[2 * g], chars_old[2 * g + 1]) * eta[(size_t)g];
        chars_new[2 * g] = chi.real();
        chars_new[2 * g + 1] = chi.imag();
    }
    QBH_TRY(qrepr_symmetry(Rn, tab_n, n_sites, d, total_new, n_trans, perms, chars_new.data(), who));
    return sector_apply_gather(who, Ro, tab_o, Rn, tab_n, op, d_vec_old, d_vec_new, dim_old_out, dim_new_out, (hipStream_t)stream);
}

// N_q and the two S^z_q of a Kondo lattice, with the characters of the TARGET momentum
extern "C" int qbh_mopr_diag_kondo_repr_dev(int n_sites, int n_elec, int two_sz, int n_trans, const int32_t *perms,
                                            const double *chars_new, const qbh_z *coef_up, const qbh_z *coef_dn, const qbh_z *coef_spin,
                                            const qbh_z *d_vec_old, qbh_z *d_vec_new, int64_t *dim_out)
{
    using namespace qbh;
    const char *who = "qbh_mopr_diag_kondo_repr_dev";
    if (!coef_up || !coef_dn || !coef_spin || !d_vec_old || !d_vec_new) {
        set_error("%s: invalid argument", who);
        return QBH_EINVAL;
    }
    std::vector<KondoReprDev> rr(1);
    KondoReprDev &R = rr[0];
    memset(&R, 0, sizeof(R));
    QBH_TRY(kondo_shape(who, n_sites, n_elec, two_sz, R.k));
    std::vector<uint64_t> tab;
    QBH_TRY(kondo_symmetry(R, tab, n_trans, perms, chars_new, who));
    const qbh_z *sets[3] = {coef_up, coef_dn, coef_spin};
    QBH_TRY(coef_character(who, n_sites, n_trans, perms, sets, 3, nullptr));
    KondoDiagSum z{};
    z.n_sites = n_sites;
    for (int s = 0; s < n_sites; ++s) {
        z.up_re[s] = coef_up[s].re;
        z.up_im[s] = coef_up[s].im;
        z.dn_re[s] = coef_dn[s].re;
        z.dn_im[s] = coef_dn[s].im;
        z.sp_re[s] = coef_spin[s].re;
        z.sp_im[s] = coef_spin[s].im;
    }
    return sector_apply_diag(who, R, tab, z, d_vec_old, d_vec_new, dim_out);
}

// N_q / S^z_q of the Hubbard family, with the characters of the TARGET momentum
extern "C" int qbh_mopr_diag_hubrepr_dev(int n_sites, int n_up, int n_dn, int n_trans, const int32_t *perms, const double *chars_new,
                                         const qbh_z *coef_up, const qbh_z *coef_dn, const qbh_z *d_vec_old, qbh_z *d_vec_new,
                                         int64_t *dim_out)
{
    using namespace qbh;
    const char *who = "qbh_mopr_diag_hubrepr_dev";
    if (!perms || !chars_new || !coef_up || !coef_dn || !d_vec_old || !d_vec_new || n_sites <= 0 || n_sites > 31 || n_up < 0 ||
        n_up > n_sites || n_dn < 0 || n_dn > n_sites || n_trans < 1 || n_trans > kReprMaxTrans) {
        set_error("qbh_mopr_diag_hubrepr_dev: invalid argument");
        return QBH_EINVAL;
    }
    std::vector<HubReprDev> rr(1);
    std::vector<uint64_t> tab;
    QBH_TRY(hubrepr_symmetry(rr[0], tab, n_sites, n_up, n_dn, n_trans, perms, chars_new, who));
    const qbh_z *sets[2] = {coef_up, coef_dn};
    QBH_TRY(coef_character(who, n_sites, n_trans, perms, sets, 2, nullptr));
    HubDensitySum z{};
    z.n_sites = n_sites;
    for (int s = 0; s < n_sites; ++s) {
        z.cf.up_re[s] = coef_up[s].re;
        z.cf.up_im[s] = coef_up[s].im;
        z.cf.dn_re[s] = coef_dn[s].re;
        z.cf.dn_im[s] = coef_dn[s].im;
    }
    return sector_apply_diag(who, rr[0], tab, z, d_vec_old, d_vec_new, dim_out);
}

// c_{q,sigma} (kind -1) / c^dag_{q,sigma} (kind +1) of the Hubbard family, the operators of the single-particle spectral function
extern "C" int qbh_mopr_c_hubrepr_dev(int n_sites, int n_up_old, int n_dn_old, int species, int kind, int n_trans, const int32_t *perms,
                                      const double *chars_old, const double *chars_new, const qbh_z *coef, const qbh_z *d_vec_old,
                                      qbh_z *d_vec_new, int64_t *dim_old_out, int64_t *dim_new_out)
{
    using namespace qbh;
    const char *who = "qbh_mopr_c_hubrepr_dev";
    if (!perms || !chars_old || !chars_new || !coef || !d_vec_old || !d_vec_new || n_sites <= 0 || n_sites > 31 || n_up_old < 0 ||
        n_up_old > n_sites || n_dn_old < 0 || n_dn_old > n_sites || n_trans < 1 || n_trans > kReprMaxTrans ||
        (species != 0 && species != 1) || (kind != 1 && kind != -1)) {
        set_error("qbh_mopr_c_hubrepr_dev: invalid argument (species 0 up / 1 down, kind -1 annihilate / +1 create)");
        return QBH_EINVAL;
    }
    const int n_up_new = n_up_old + (species == 0 ? kind : 0), n_dn_new = n_dn_old + (species == 1 ? kind : 0);
    if (n_up_new < 0 || n_up_new > n_sites || n_dn_new < 0 || n_dn_new > n_sites) {
        set_error("qbh_mopr_c_hubrepr_dev: the target sector does not exist");
        return QBH_EINVAL;
    }
    std::vector<HubReprDev> rr(2);
    std::vector<uint64_t> tab_o, tab_n;
    QBH_TRY(hubrepr_symmetry(rr[0], tab_o, n_sites, n_up_old, n_dn_old, n_trans, perms, chars_old, who));
    QBH_TRY(hubrepr_symmetry(rr[1], tab_n, n_sites, n_up_new, n_dn_new, n_trans, perms, chars_new, who));
    HubFermion op{};
    op.n_sites = n_sites;
    op.species = species;
    op.create = kind > 0 ? 1 : 0;
    for (int s = 0; s < n_sites; ++s) {
        op.re[s] = coef[s].re;
        op.im[s] = coef[s].im;
    }
    return sector_apply_gather(who, rr[0], tab_o, rr[1], tab_n, op, d_vec_old, d_vec_new, dim_old_out, dim_new_out, nullptr);
}
