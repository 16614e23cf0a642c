// qbh_sector.hip -- the stored operators of momentum sectors: qbh_gen_heisenberg_repr, qbh_gen_hubbard_repr,
// qbh_gen_qudit_repr, qbh_gen_kondo_repr and their _cuts forms (toolkit and families: qbh_sector.hpp).
#include "qbh_sector.hpp"

// ---- the entry points: validate -> symmetry -> the family's terms -> sector_enumerate -> the rows, or the operator's kernel ----
static int gen_heisenberg_repr_impl(qbh_csr **out, int n_sites, int n_dn, int n_bonds, const int32_t *bonds, double J,
                                       int n_trans, const int32_t *perms, const double *chars, double fake_pos,
                                       int shard, int n_shards, const int64_t *row_cuts, int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    const char *who = "qbh_gen_heisenberg_repr";
    if (!out || !bonds || !perms || !chars || n_sites <= 0 || n_sites > 62 || n_dn < 0 || n_dn > n_sites || n_dn > 33 ||
        n_bonds <= 0 || n_trans < 1 || n_trans > kReprMaxTrans || n_shards < 1 || shard < 0 || shard >= n_shards) {
        set_error("qbh_gen_heisenberg_repr: invalid argument (<= 62 sites, <= 64 translations)");
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP(hipSetDevice(opts->device));
    std::vector<ReprDev> rr(1);
    ReprDev &R = rr[0];
    std::vector<uint64_t> tab;
    QBH_TRY(repr_symmetry(R, tab, n_sites, n_dn, n_trans, perms, chars, who));
    std::map<std::pair<int, int>, double> bmap;
    QBH_TRY(merge_bonds(n_sites, n_bonds, bonds, bmap));
    if ((int)bmap.size() + 1 > kReprMaxRow || (int)bmap.size() > kMaxBonds) {
        set_error("qbh_gen_heisenberg_repr: too many distinct bonds");
        return QBH_EUNSUPP;
    }
    for (const auto &bw : bmap) {
        R.h.sa[R.h.n_bonds] = bw.first.first;
        R.h.sb[R.h.n_bonds] = bw.first.second;
        R.h.offd[R.h.n_bonds] = 0.5 * J * bw.second;
        R.h.diag[R.h.n_bonds] = 0.25 * J * bw.second;
        R.h.n_bonds++;
    }
    R.fake_pos = fake_pos;
    DevBufs bufs;
    SectorDev<ReprDev> S;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who));
    return assemble_sector_rows(who, bufs.pool, S.R, S.tab, S.reps, S.info, S.dim, shard, n_shards, row_cuts, opts, out, dim_out);
}

static int gen_hubbard_repr_impl(qbh_csr **out, int n_sites, int n_up, int n_dn, int n_terms, const int32_t *term_sites,
                                    const qbh_z *amp_up, const qbh_z *amp_dn, double U, int n_pairs, const int32_t *pair_sites,
                                    const double *pair_v, int n_exch, const int32_t *exch_sites, const double *exch_amp,
                                    int no_double, int n_trans, const int32_t *perms, const double *chars, double fake_pos,
                                    int shard, int n_shards, const int64_t *row_cuts, int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    const char *who = "qbh_gen_hubbard_repr";
    if (n_exch < 0 || n_exch > kHubReprMaxPairs || (n_exch > 0 && (!exch_sites || !exch_amp))) {
        set_error("qbh_gen_hubbard_repr: invalid spin-exchange term list");
        return QBH_EINVAL;
    }
    if (!out || (n_terms > 0 && (!term_sites || !amp_up || !amp_dn)) || !perms || !chars || n_sites <= 0 || n_sites > 31 || n_up < 0 ||
        n_up > n_sites || n_dn < 0 || n_dn > n_sites || n_terms < 0 || n_pairs < 0 || n_pairs > kHubReprMaxPairs ||
        (n_pairs > 0 && (!pair_sites || !pair_v)) || n_trans < 1 || n_trans > kReprMaxTrans || n_shards < 1 || shard < 0 ||
        shard >= n_shards) {
        set_error("qbh_gen_hubbard_repr: invalid argument (<= 31 sites, <= 64 translations)");
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP(hipSetDevice(opts->device));
    std::vector<HubReprDev> rr(1);
    HubReprDev &R = rr[0];
    std::vector<uint64_t> tab;
    QBH_TRY(hubrepr_symmetry(R, tab, n_sites, n_up, n_dn, n_trans, perms, chars, who));
    TermMap tmap;
    QBH_TRY(merge_terms(n_sites, n_terms, term_sites, amp_up, amp_dn, n_exch, who, tmap));
    for (const auto &kv : tmap) {
        R.ti[R.n_terms] = (int8_t)kv.first.first;
        R.tj[R.n_terms] = (int8_t)kv.first.second;
        R.aup[R.n_terms][0] = kv.second[0];
        R.aup[R.n_terms][1] = kv.second[1];
        R.adn[R.n_terms][0] = kv.second[2];
        R.adn[R.n_terms][1] = kv.second[3];
        R.n_terms++;
    }
    R.U = U;
    R.fake_pos = fake_pos;
    for (int p = 0; p < n_pairs; ++p) {
        const int i = pair_sites[2 * p], j = pair_sites[2 * p + 1];
        if (i < 0 || i >= n_sites || j < 0 || j >= n_sites) {
            set_error("qbh_gen_hubbard_repr: density-density term %d acts on a site outside the lattice", p);
            return QBH_EINVAL;
        }
        R.pi[p] = (int8_t)i;
        R.pj[p] = (int8_t)j;
        for (int c = 0; c < 4; ++c) R.pv[p][c] = pair_v[4 * p + c];
    }
    R.n_pairs = n_pairs;
    for (int e = 0; e < n_exch; ++e) {
        const int i = exch_sites[2 * e], j = exch_sites[2 * e + 1];
        if (i < 0 || i >= n_sites || j < 0 || j >= n_sites || i == j) {
            set_error("qbh_gen_hubbard_repr: spin-exchange term %d needs two different sites of the lattice", e);
            return QBH_EINVAL;
        }
        R.xi[e] = (int8_t)i;
        R.xj[e] = (int8_t)j;
        R.xa[e] = exch_amp[e];
    }
    R.n_exch = n_exch;
    R.no_double = no_double ? 1 : 0;
    DevBufs bufs;
    SectorDev<HubReprDev> S;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who));
    return assemble_sector_rows(who, bufs.pool, S.R, S.tab, S.reps, S.info, S.dim, shard, n_shards, row_cuts, opts, out, dim_out);
}

static int gen_qudit_repr_impl(qbh_csr **out, int n_sites, int d, int total, int n_pairs, const int32_t *pair_sites,
                               const qbh_z *pair_mat, int n_single, const int32_t *single_sites, const double *single_diag,
                               int n_trans, const int32_t *perms, const double *chars, double fake_pos, int shard, int n_shards,
                               const int64_t *row_cuts, int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    const char *who = "qbh_gen_qudit_repr";
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
    if (!perms || !chars || n_trans < 1 || n_trans > kReprMaxTrans || n_shards < 1 || shard < 0 || shard >= n_shards) {
        set_error("%s: invalid symmetry or shard argument (1 .. %d translations)", who, kReprMaxTrans);
        return QBH_EINVAL;
    }
    QuditTerms T;
    QBH_TRY(qudit_merge_terms(who, n_sites, d, n_pairs, pair_sites, pair_mat, n_single, single_sites, single_diag, T));
    QuditReprDev R;
    std::vector<uint64_t> tab;
    QBH_TRY(qrepr_symmetry(R, tab, n_sites, d, total, n_trans, perms, chars, who));
    QBH_TRY(qrepr_invariant(T, n_sites, d, n_trans, perms, who));
    if (T.max_row > kQuditReprMaxRow) {
        set_error("%s: a row may hold %d entries; at most %d are supported", who, T.max_row, kQuditReprMaxRow);
        return QBH_EUNSUPP;
    }
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));       // every refusal comes before the device is looked for
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP_WHO(who, hipSetDevice(opts->device));
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
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who));
    return assemble_sector_rows(who, bufs.pool, S.R, S.tab, S.reps, S.info, S.dim, shard, n_shards, row_cuts, opts, out, dim_out);
}

extern "C" int qbh_gen_qudit_repr(qbh_csr **out, int n_sites, int d, int total, int n_pairs, const int32_t *pair_sites,
                                  const qbh_z *pair_mat, int n_single, const int32_t *single_sites, const double *single_diag,
                                  int n_trans, const int32_t *perms, const double *chars, double fake_pos, int shard, int n_shards,
                                  int64_t *dim_out, const qbh_opts *opts)
{
    return gen_qudit_repr_impl(out, n_sites, d, total, n_pairs, pair_sites, pair_mat, n_single, single_sites, single_diag, n_trans,
                               perms, chars, fake_pos, shard, n_shards, nullptr, dim_out, opts);
}

extern "C" int qbh_gen_qudit_repr_cuts(qbh_csr **out, int n_sites, int d, int total, int n_pairs, const int32_t *pair_sites,
                                       const qbh_z *pair_mat, int n_single, const int32_t *single_sites, const double *single_diag,
                                       int n_trans, const int32_t *perms, const double *chars, double fake_pos, int shard,
                                       int n_shards, const int64_t *row_cuts, int64_t *dim_out, const qbh_opts *opts)
{
    return gen_qudit_repr_impl(out, n_sites, d, total, n_pairs, pair_sites, pair_mat, n_single, single_sites, single_diag, n_trans,
                               perms, chars, fake_pos, shard, n_shards, row_cuts, dim_out, opts);
}

static int gen_kondo_repr_impl(qbh_csr **out, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites,
                               const qbh_z *amp_up, const qbh_z *amp_dn, double U, const double *kz, const double *kxy, int n_sbonds,
                               const int32_t *sbond_sites, const double *bz, const double *bxy, int n_trans, const int32_t *perms,
                               const double *chars, double fake_pos, int shard, int n_shards, const int64_t *row_cuts,
                               int64_t *dim_out, const qbh_opts *opts)
{
    using namespace qbh;
    const char *who = "qbh_gen_kondo_repr";
    if (!out || n_shards < 1 || shard < 0 || shard >= n_shards) {
        set_error("%s: invalid output or shard argument", who);
        return QBH_EINVAL;
    }
    std::vector<KondoReprDev> rr(1);
    KondoReprDev &R = rr[0];
    memset(&R, 0, sizeof(R));
    const int max_row = kondo_setup(who, n_sites, n_elec, two_sz, n_terms, term_sites, amp_up, amp_dn, U, kz, kxy, n_sbonds,
                                    sbond_sites, bz, bxy, R.k);
    if (max_row <= 0) return max_row;
    std::vector<uint64_t> tab;
    QBH_TRY(kondo_symmetry(R, tab, n_trans, perms, chars, who));
    QBH_TRY(kondo_invariant(who, R.k, n_trans, perms));
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));       // every refusal comes before the device is looked for
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP_WHO(who, hipSetDevice(opts->device));
    R.fake_pos = fake_pos;
    DevBufs bufs;
    SectorDev<KondoReprDev> S;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who));
    return assemble_sector_rows(who, bufs.pool, S.R, S.tab, S.reps, S.info, S.dim, shard, n_shards, row_cuts, opts, out, dim_out);
}

extern "C" int qbh_gen_kondo_repr(qbh_csr **out, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites,
                                  const qbh_z *amp_up, const qbh_z *amp_dn, double U, const double *kz, const double *kxy,
                                  int n_sbonds, const int32_t *sbond_sites, const double *bz, const double *bxy, int n_trans,
                                  const int32_t *perms, const double *chars, double fake_pos, int shard, int n_shards,
                                  int64_t *dim_out, const qbh_opts *opts)
{
    return gen_kondo_repr_impl(out, n_sites, n_elec, two_sz, n_terms, term_sites, amp_up, amp_dn, U, kz, kxy, n_sbonds, sbond_sites, bz,
                               bxy, n_trans, perms, chars, fake_pos, shard, n_shards, nullptr, dim_out, opts);
}

extern "C" int qbh_gen_kondo_repr_cuts(qbh_csr **out, int n_sites, int n_elec, int two_sz, int n_terms, const int32_t *term_sites,
                                       const qbh_z *amp_up, const qbh_z *amp_dn, double U, const double *kz, const double *kxy,
                                       int n_sbonds, const int32_t *sbond_sites, const double *bz, const double *bxy, int n_trans,
                                       const int32_t *perms, const double *chars, double fake_pos, int shard, int n_shards,
                                       const int64_t *row_cuts, int64_t *dim_out, const qbh_opts *opts)
{
    return gen_kondo_repr_impl(out, n_sites, n_elec, two_sz, n_terms, term_sites, amp_up, amp_dn, U, kz, kxy, n_sbonds, sbond_sites, bz,
                               bxy, n_trans, perms, chars, fake_pos, shard, n_shards, row_cuts, dim_out, opts);
}

// ---- public entry points of the sector generators: uniform row blocks, or the caller's row cuts ----
extern "C" int qbh_gen_heisenberg_repr(qbh_csr **out, int n_sites, int n_dn, int n_bonds, const int32_t *bonds, double J,
                                       int n_trans, const int32_t *perms, const double *chars, double fake_pos,
                                       int shard, int n_shards, int64_t *dim_out, const qbh_opts *opts)
{
    return gen_heisenberg_repr_impl(out, n_sites, n_dn, n_bonds, bonds, J, n_trans, perms, chars, fake_pos, shard, n_shards, nullptr,
                                    dim_out, opts);
}
extern "C" int qbh_gen_heisenberg_repr_cuts(qbh_csr **out, int n_sites, int n_dn, int n_bonds, const int32_t *bonds, double J,
                                            int n_trans, const int32_t *perms, const double *chars, double fake_pos,
                                            int shard, int n_shards, const int64_t *row_cuts, int64_t *dim_out, const qbh_opts *opts)
{
    return gen_heisenberg_repr_impl(out, n_sites, n_dn, n_bonds, bonds, J, n_trans, perms, chars, fake_pos, shard, n_shards, row_cuts,
                                    dim_out, opts);
}
extern "C" int qbh_gen_hubbard_repr(qbh_csr **out, int n_sites, int n_up, int n_dn, int n_terms, const int32_t *term_sites,
                                    const qbh_z *amp_up, const qbh_z *amp_dn, double U, int n_pairs, const int32_t *pair_sites,
                                    const double *pair_v, int n_exch, const int32_t *exch_sites, const double *exch_amp,
                                    int no_double, int n_trans, const int32_t *perms, const double *chars, double fake_pos,
                                    int shard, int n_shards, int64_t *dim_out, const qbh_opts *opts)
{
    return gen_hubbard_repr_impl(out, n_sites, n_up, n_dn, n_terms, term_sites, amp_up, amp_dn, U, n_pairs, pair_sites, pair_v, n_exch,
                                 exch_sites, exch_amp, no_double, n_trans, perms, chars, fake_pos, shard, n_shards, nullptr, dim_out, opts);
}
extern "C" int qbh_gen_hubbard_repr_cuts(qbh_csr **out, int n_sites, int n_up, int n_dn, int n_terms, const int32_t *term_sites,
                                         const qbh_z *amp_up, const qbh_z *amp_dn, double U, int n_pairs, const int32_t *pair_sites,
                                         const double *pair_v, int n_exch, const int32_t *exch_sites, const double *exch_amp,
                                         int no_double, int n_trans, const int32_t *perms, const double *chars, double fake_pos,
                                         int shard, int n_shards, const int64_t *row_cuts, int64_t *dim_out, const qbh_opts *opts)
{
    return gen_hubbard_repr_impl(out, n_sites, n_up, n_dn, n_terms, term_sites, amp_up, amp_dn, U, n_pairs, pair_sites, pair_v, n_exch,
                                 exch_sites, exch_amp, no_double, n_trans, perms, chars, fake_pos, shard, n_shards, row_cuts, dim_out, opts);
}
