// qbh_gen.hip -- measurement harness: assemble the benchmark Hamiltonians directly in HBM.
//
// The reference builds its CSR on the host (model::generate_Ham_sparse_full,
// src/model.cc:619-685: brute-force basis enumeration, forward_list LIL, ~48 B/nnz) and
// cannot reach dim >= 1e8.  These generators produce the same operators (same model
// definitions as examples/trans_absent/latt_square/square_Fermi_Hubbard.cc and
// latt_kagome/kagome_Heisenberg_spin_half.cc) in a locality-friendly basis order; spectra
// are invariant under the basis permutation / sign gauge, and tests/ check the device CSR
// entry-by-entry against an independent numpy assembly at small sizes.
//
// Conventions (documented in include/qbhip.h):
//   Hubbard   index = rank(up) * C(L, n_dn) + rank(dn), ranks colexicographic (= ascending
//             bit pattern); operator order: all up, then all down -> hop signs factorise.
//   Heisenberg index = colex rank of the down-spin bit pattern.
#include "qbh_gen_util.hpp"

namespace qbh {
namespace {

// ------------------------------------------------------------------ Hubbard ----

struct HopTable {              // per configuration: sorted (target rank, amplitude) lists
    std::vector<uint32_t> cfg;
    std::vector<int32_t> ptr, tgt, nlo;
    std::vector<double> val;
};

// bonds: unique (a,b) -> weight w.  amplitude of c+_b c_a on |cfg> is -t*w*(-1)^(# set bits between)
void build_hops(int L, int n, const std::map<std::pair<int, int>, double> &bonds, double t, HopTable &H)
{
    enumerate_configs(L, n, H.cfg);
    const size_t N = H.cfg.size();
    H.ptr.assign(N + 1, 0);
    H.nlo.assign(N, 0);
    H.tgt.clear();
    H.val.clear();
    for (size_t i = 0; i < N; ++i) {
        const uint32_t c = H.cfg[i];
        std::map<int32_t, double> row;
        for (const auto &bw : bonds) {
            const int s0 = bw.first.first, s1 = bw.first.second;
            for (int dir = 0; dir < 2; ++dir) {
                const int a = dir ? s1 : s0, b = dir ? s0 : s1;       // particle moves a -> b
                if (!((c >> a) & 1u) || ((c >> b) & 1u)) continue;
                const uint32_t nc = (c ^ (1u << a)) | (1u << b);
                const int lo = std::min(a, b), hi = std::max(a, b);
                const uint32_t between = (uint32_t)(((1ULL << hi) - 1ULL) & ~((1ULL << (lo + 1)) - 1ULL));
                const double sign = (__builtin_popcount(c & between) & 1) ? -1.0 : 1.0;
                const int32_t j = (int32_t)(std::lower_bound(H.cfg.begin(), H.cfg.end(), nc) - H.cfg.begin());
                row[j] += -t * bw.second * sign;
            }
        }
        for (const auto &e : row) {
            if (std::fabs(e.second) < QBH_SPARSE_PRECISION) continue;    // lil_mat::add drop rule
            H.tgt.push_back(e.first);
            H.val.push_back(e.second);
            if (e.first < (int32_t)i) H.nlo[i]++;
        }
        H.ptr[i + 1] = (int32_t)H.tgt.size();
    }
}

// Recursive spectral bisection of the hop graph of one species into `parts` parts of sizes (q + 1) N / parts - q N / parts (the
// major-index ranges of dist.kron_row_cuts): at every level the Fiedler vector of the sub-graph by power iteration on c I - L
// with the constant vector projected out (600 sweeps; plain double arithmetic in a fixed order: every rank computes the same
// numbers), nodes sorted by it and cut at the size the left ranks own.  Inside a part the nodes keep their ascending order.
// inv[new index] = old index.
void partition_majors(const HopTable &H, int parts, std::vector<int32_t> &inv)
{
    const int64_t N = (int64_t)H.cfg.size();
    std::vector<int64_t> cu((size_t)parts + 1);
    for (int q = 0; q <= parts; ++q) cu[(size_t)q] = (int64_t)q * N / parts;
    std::vector<int32_t> order((size_t)N), pos((size_t)N, -1);
    for (int64_t i = 0; i < N; ++i) order[(size_t)i] = (int32_t)i;
    struct Job { int64_t lo, hi; int q0, q1; };
    std::vector<Job> stack{{0, N, 0, parts}};
    std::vector<double> f, g;
    while (!stack.empty()) {
        const Job j = stack.back();
        stack.pop_back();
        if (j.q1 - j.q0 <= 1) {
            std::sort(order.begin() + j.lo, order.begin() + j.hi);        // ascending patterns inside a part
            continue;
        }
        const int64_t n = j.hi - j.lo;
        for (int64_t i = 0; i < n; ++i) pos[(size_t)order[(size_t)(j.lo + i)]] = (int32_t)i;
        f.assign((size_t)n, 0.0);
        g.assign((size_t)n, 0.0);
        uint64_t lcg = 88172645463325252ULL;
        double cmax = 1.0;
        for (int64_t i = 0; i < n; ++i) {
            lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
            f[(size_t)i] = (double)(lcg >> 11) / 9007199254740992.0 - 0.5;
            const int32_t u = order[(size_t)(j.lo + i)];
            cmax = std::max(cmax, 2.0 * (double)(H.ptr[u + 1] - H.ptr[u]));
        }
        for (int sweep = 0; sweep < 600; ++sweep) {
            double mean = 0.0;
            for (int64_t i = 0; i < n; ++i) mean += f[(size_t)i];
            mean /= (double)n;
            double nrm = 0.0;
            for (int64_t i = 0; i < n; ++i) {
                const int32_t u = order[(size_t)(j.lo + i)];
                double deg = 0.0, sum = 0.0;
                for (int32_t e = H.ptr[u]; e < H.ptr[u + 1]; ++e) {
                    const int32_t p = pos[(size_t)H.tgt[(size_t)e]];
                    if (p >= 0 && H.tgt[(size_t)e] != u) {
                        deg += 1.0;
                        sum += f[(size_t)p] - mean;
                    }
                }
                const double v = (cmax - deg) * (f[(size_t)i] - mean) + sum;       // (c I - L)(f - mean)
                g[(size_t)i] = v;
                nrm += v * v;
            }
            nrm = std::sqrt(nrm);
            if (!(nrm > 0.0)) break;
            for (int64_t i = 0; i < n; ++i) f[(size_t)i] = g[(size_t)i] / nrm;
        }
        for (int64_t i = 0; i < n; ++i) pos[(size_t)order[(size_t)(j.lo + i)]] = -1;
        std::vector<std::pair<double, int32_t>> key((size_t)n);
        for (int64_t i = 0; i < n; ++i) key[(size_t)i] = {f[(size_t)i], order[(size_t)(j.lo + i)]};
        std::sort(key.begin(), key.end());
        for (int64_t i = 0; i < n; ++i) order[(size_t)(j.lo + i)] = key[(size_t)i].second;
        const int qm = j.q0 + (j.q1 - j.q0) / 2;
        const int64_t mid = j.lo + (cu[(size_t)qm] - cu[(size_t)j.q0]);
        stack.push_back({j.lo, mid, j.q0, qm});
        stack.push_back({mid, j.hi, qm, j.q1});
    }
    inv = order;
}

// the hop table with its configurations re-labelled: new index i holds old configuration inv[i]; every list sorted by new target
void permute_hops(HopTable &H, const std::vector<int32_t> &inv)
{
    const size_t N = H.cfg.size();
    std::vector<int32_t> fwd(N);
    for (size_t i = 0; i < N; ++i) fwd[(size_t)inv[i]] = (int32_t)i;
    HopTable P;
    P.cfg.resize(N);
    P.ptr.assign(N + 1, 0);
    P.nlo.assign(N, 0);
    P.tgt.reserve(H.tgt.size());
    P.val.reserve(H.val.size());
    std::vector<std::pair<int32_t, double>> row;
    for (size_t i = 0; i < N; ++i) {
        const int32_t o = inv[i];
        P.cfg[i] = H.cfg[(size_t)o];
        row.clear();
        for (int32_t e = H.ptr[o]; e < H.ptr[o + 1]; ++e) row.emplace_back(fwd[(size_t)H.tgt[(size_t)e]], H.val[(size_t)e]);
        std::sort(row.begin(), row.end());
        for (const auto &e : row) {
            P.tgt.push_back(e.first);
            P.val.push_back(e.second);
            if (e.first < (int32_t)i) P.nlo[i]++;
        }
        P.ptr[i + 1] = (int32_t)P.tgt.size();
    }
    H = std::move(P);
}

struct HubDev {
    const uint32_t *cfg_u, *cfg_d;
    const int32_t *ptr_u, *tgt_u, *nlo_u, *ptr_d, *tgt_d, *nlo_d;
    const double *val_u, *val_d;
    const int64_t *base_u;   // [Nu+1] nnz before the first row of up-block u
    const int64_t *pre_d;    // [Nd+1] dn hops before dn config d
    int64_t Nu, Nd;
    double U;
};

__device__ __forceinline__ int64_t hub_rowptr(const HubDev &h, int64_t row)
{
    if (row >= h.Nu * h.Nd) return h.base_u[h.Nu];
    const int64_t u = row / h.Nd, d = row - u * h.Nd;
    const int64_t nu = h.ptr_u[u + 1] - h.ptr_u[u];
    return h.base_u[u] + d * (1 + nu) + h.pre_d[d];
}

// 32 lanes per row: lane l writes entry l, l+32, ... of the row (coalesced 20 B/entry).
__global__ __launch_bounds__(256) void k_gen_hubbard(HubDev h, int64_t row_begin, int64_t row_end,
                                                     int64_t *ia, int32_t *ja, d2 *val)
{
    const int64_t grp = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 5;
    const int sub = threadIdx.x & 31;
    const int64_t ngrp = ((int64_t)gridDim.x * 256) >> 5;
    const int64_t p_begin = hub_rowptr(h, row_begin);
    for (int64_t row = row_begin + grp; row < row_end; row += ngrp) {
        const int64_t u = row / h.Nd, d = row - u * h.Nd;
        const int pu = h.ptr_u[u], nu = h.ptr_u[u + 1] - pu, lo_u = h.nlo_u[u];
        const int pd = h.ptr_d[d], nd = h.ptr_d[d + 1] - pd, lo_d = h.nlo_d[d];
        const int64_t p0 = h.base_u[u] + d * (1 + nu) + h.pre_d[d] - p_begin;
        if (sub == 0) ia[row - row_begin] = p0;
        const int n = 1 + nu + nd;
        for (int l = sub; l < n; l += 32) {
            int32_t col;
            d2 v = {0.0, 0.0};
            if (l < lo_u) {                                   // up hops to lower up-blocks
                col = (int32_t)((int64_t)h.tgt_u[pu + l] * h.Nd + d);
                v.x = h.val_u[pu + l];
            } else if (l < lo_u + lo_d) {                     // dn hops below the diagonal
                const int q = l - lo_u;
                col = (int32_t)(u * h.Nd + h.tgt_d[pd + q]);
                v.x = h.val_d[pd + q];
            } else if (l == lo_u + lo_d) {                    // diagonal (always stored)
                col = (int32_t)row;
                v.x = h.U * (double)__popc(h.cfg_u[u] & h.cfg_d[d]);
            } else if (l < lo_u + 1 + nd) {                   // dn hops above the diagonal
                const int q = l - lo_u - 1;
                col = (int32_t)(u * h.Nd + h.tgt_d[pd + q]);
                v.x = h.val_d[pd + q];
            } else {                                          // up hops to higher up-blocks
                const int q = l - 1 - nd;
                col = (int32_t)((int64_t)h.tgt_u[pu + q] * h.Nd + d);
                v.x = h.val_u[pu + q];
            }
            ja[p0 + l] = col;
            val[p0 + l] = v;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ia[row_end - row_begin] = hub_rowptr(h, row_end) - p_begin;
}

// lil_mat::add drop rule, as in build_hops: a bond whose off-diagonal amplitude is below the sparse precision adds to the
// diagonal only.  The count and the fill pass ask the same question.
__device__ __forceinline__ bool heis_stores(const HeisDev &h, int bnd) { return fabs(h.offd[bnd]) >= QBH_SPARSE_PRECISION; }

__global__ __launch_bounds__(256) void k_heis_count(const HeisDev *hp, int64_t row_begin, int64_t row_end,
                                                    int32_t *cnt)
{
    const HeisDev &h = *hp;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; row < row_end; row += stride) {
        const uint64_t s = heis_unrank(h, (uint64_t)row);
        int c = 1;
        for (int bnd = 0; bnd < h.n_bonds; ++bnd)
            if (heis_stores(h, bnd)) c += (int)(((s >> h.sa[bnd]) ^ (s >> h.sb[bnd])) & 1ULL);
        cnt[row - row_begin] = c;
    }
}

__global__ __launch_bounds__(256) void k_heis_fill(const HeisDev *hp, int64_t row_begin, int64_t row_end,
                                                   const int64_t *ia, int32_t *ja, d2 *val)
{
    const HeisDev &h = *hp;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; row < row_end; row += stride) {
        const uint64_t s = heis_unrank(h, (uint64_t)row);
        int32_t cols[kMaxBonds + 1];
        double vals[kMaxBonds + 1];
        int n = 0;
        double dg = 0.0;
        for (int bnd = 0; bnd < h.n_bonds; ++bnd) {
            const uint64_t ma = 1ULL << h.sa[bnd], mb = 1ULL << h.sb[bnd];
            const bool differ = (((s >> h.sa[bnd]) ^ (s >> h.sb[bnd])) & 1ULL) != 0;
            if (differ) {
                dg -= h.diag[bnd];
                if (!heis_stores(h, bnd)) continue;
                const int32_t c = (int32_t)heis_rank(h, s ^ ma ^ mb);
                int q = n++;                               // insertion sort by column
                while (q > 0 && cols[q - 1] > c) {
                    cols[q] = cols[q - 1];
                    vals[q] = vals[q - 1];
                    --q;
                }
                cols[q] = c;
                vals[q] = h.offd[bnd];
            } else {
                dg += h.diag[bnd];
            }
        }
        {
            const int32_t c = (int32_t)row;
            int q = n++;
            while (q > 0 && cols[q - 1] > c) {
                cols[q] = cols[q - 1];
                vals[q] = vals[q - 1];
                --q;
            }
            cols[q] = c;
            vals[q] = dg;
        }
        const int64_t p0 = ia[row - row_begin];
        for (int q = 0; q < n; ++q) {
            ja[p0 + q] = cols[q];
            val[p0 + q] = d2{vals[q], 0.0};
        }
    }
}

}  // namespace
}  // namespace qbh

using qbh::d2;

extern "C" int qbh_gen_hubbard(qbh_csr **out, int n_sites, int n_up, int n_dn, int n_bonds, const int32_t *bonds,
                               double t, double U, int64_t row_begin, int64_t row_end, const qbh_opts *opts)
{
    using namespace qbh;
    if (!out || !bonds || n_sites <= 0 || n_sites > 31 || n_up < 0 || n_dn < 0 || n_up > n_sites ||
        n_dn > n_sites || n_bonds <= 0) {
        set_error("qbh_gen_hubbard: invalid lattice / filling");
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP(hipSetDevice(opts->device));
    std::map<std::pair<int, int>, double> bmap;
    QBH_TRY(merge_bonds(n_sites, n_bonds, bonds, bmap));
    HopTable hu, hd;
    build_hops(n_sites, n_up, bmap, t, hu);
    build_hops(n_sites, n_dn, bmap, t, hd);
    const int64_t Nu = (int64_t)hu.cfg.size(), Nd = (int64_t)hd.cfg.size(), dim = Nu * Nd;
    if (dim >= 2147483647LL) {
        set_error("qbh_gen_hubbard: dim %lld exceeds int32 columns", (long long)dim);
        return QBH_EUNSUPP;
    }
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("qbh_gen_hubbard: bad row range");
        return QBH_EINVAL;
    }
    // qbh_opts.major_partition: the up configurations in the order of a recursive spectral bisection into that many parts
    std::vector<int32_t> major_inv;                    // [new major index] -> the generator's (ascending pattern) index
    const int n_parts = (opts && opts->major_partition > 1 && (int64_t)opts->major_partition <= Nu) ? opts->major_partition : 0;
    if (n_parts > 1) {
        partition_majors(hu, n_parts, major_inv);
        permute_hops(hu, major_inv);
    }
    std::vector<int64_t> pre_d((size_t)Nd + 1, 0), base_u((size_t)Nu + 1, 0);
    for (int64_t d = 0; d < Nd; ++d) pre_d[d + 1] = pre_d[d] + (hd.ptr[d + 1] - hd.ptr[d]);
    for (int64_t u = 0; u < Nu; ++u)
        base_u[u + 1] = base_u[u] + Nd * (1 + (hu.ptr[u + 1] - hu.ptr[u])) + pre_d[Nd];

    std::vector<void *> pool;
    HubDev h{};
    uint32_t *c1, *c2;
    int32_t *i1, *i2, *i3, *i4, *i5, *i6;
    double *v1, *v2;
    int64_t *b1, *b2;
    int rc = QBH_OK;
#define UP(vec, ptr) if (rc == QBH_OK) rc = upload(vec, &ptr, pool)
    UP(hu.cfg, c1); UP(hd.cfg, c2); UP(hu.ptr, i1); UP(hu.tgt, i2); UP(hu.nlo, i3);
    UP(hd.ptr, i4); UP(hd.tgt, i5); UP(hd.nlo, i6); UP(hu.val, v1); UP(hd.val, v2);
    UP(base_u, b1); UP(pre_d, b2);
#undef UP
    if (rc != QBH_OK) {
        free_pool(pool);
        return rc;
    }
    h.cfg_u = c1; h.cfg_d = c2; h.ptr_u = i1; h.tgt_u = i2; h.nlo_u = i3;
    h.ptr_d = i4; h.tgt_d = i5; h.nlo_d = i6; h.val_u = v1; h.val_d = v2;
    h.base_u = b1; h.pre_d = b2; h.Nu = Nu; h.Nd = Nd; h.U = U;

    auto rowptr = [&](int64_t row) -> int64_t {
        if (row >= dim) return base_u[Nu];
        const int64_t u = row / Nd, d = row - u * Nd;
        return base_u[u] + d * (1 + (hu.ptr[u + 1] - hu.ptr[u])) + pre_d[d];
    };
    const int64_t nrows = row_end - row_begin;
    const int64_t nnz = rowptr(row_end) - rowptr(row_begin);
    int64_t *d_ia = nullptr;
    int32_t *d_ja = nullptr;
    d2 *d_val = nullptr;
    hipError_t e = qbh::dev_alloc(&d_ia, (size_t)(nrows + 1) * sizeof(int64_t));
    if (e == hipSuccess) e = qbh::dev_alloc(&d_ja, (size_t)nnz * sizeof(int32_t));
    if (e == hipSuccess) e = qbh::dev_alloc(&d_val, (size_t)nnz * sizeof(d2));
    if (e == hipSuccess) {
        const int64_t groups = nrows;
        int64_t grid = (groups * 32 + 255) / 256;
        if (grid > 256 * 64) grid = 256 * 64;
        hipLaunchKernelGGL(k_gen_hubbard, dim3((unsigned)grid), dim3(256), 0, 0, h, row_begin, row_end, d_ia, d_ja,
                           d_val);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    free_pool(pool);
    if (e != hipSuccess) {
        set_error("qbh_gen_hubbard: %s", hipGetErrorString(e));
        (void)hipGetLastError();      // reported: not left sticky for the next call
        if (d_ia) (void)hipFree(d_ia);
        if (d_ja) (void)hipFree(d_ja);
        if (d_val) (void)hipFree(d_val);
        return e == hipErrorOutOfMemory ? QBH_ENOMEM : QBH_EHIP;
    }
    // ownership passes with the call: on failure the arrays have already been released.  The basis is the product
    // (up configuration) x (down configuration): announce the minor size for the Kronecker split (qbh_opts.kron_split)
    qbh_opts o2;
    if (opts) o2 = *opts;
    else opts_builtin(&o2);
    o2.basis_detect = 0;
    if (o2.basis_kind == QBH_BASIS_REF_FERMION2) o2.basis_kind = QBH_BASIS_NONE;      // the generator's order is species-major already: a host's hint about ITS arrays does not describe it
    if (o2.kron_minor == 0) o2.kron_minor = Nd;        // index = up * Nd + down; kron_build checks that a shard is made of whole up blocks
    const int crc = qbh_csr_create_device(out, nrows, dim, row_begin, nnz, d_ia, d_ja, reinterpret_cast<qbh_z *>(d_val), 1, &o2);
    if (crc == QBH_OK && n_parts > 1) {               // the map stays with the handle: qbh_vec_randomize, qbh_csr_major_order
        qbh_csr *A = *out;
        if (qbh::dev_alloc(&A->d_major_inv, (size_t)Nu * sizeof(int32_t)) != hipSuccess ||
            hipMemcpy(A->d_major_inv, major_inv.data(), (size_t)Nu * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            qbh_csr_destroy(A);
            *out = nullptr;
            set_error("qbh_gen_hubbard: no room for the major-index map");
            return QBH_ENOMEM;
        }
        A->major_n = Nu;
        A->major_S = Nd;
        A->major_parts = n_parts;
    }
    return crc;
}

extern "C" int qbh_mf_hubbard(qbh_csr **out, int n_sites, int n_up, int n_dn, int n_bonds, const int32_t *bonds, double t,
                              double U, int64_t row_begin, int64_t row_end, const qbh_opts *opts)
{
    using namespace qbh;
    if (!out || !bonds || n_sites <= 0 || n_sites > 31 || n_up < 0 || n_dn < 0 || n_up > n_sites || n_dn > n_sites ||
        n_bonds <= 0) {
        set_error("qbh_mf_hubbard: invalid lattice / filling");
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP(hipSetDevice(opts->device));
    std::map<std::pair<int, int>, double> bmap;
    QBH_TRY(merge_bonds(n_sites, n_bonds, bonds, bmap));
    HopTable hu, hd;
    build_hops(n_sites, n_up, bmap, t, hu);
    build_hops(n_sites, n_dn, bmap, t, hd);
    const int64_t Nu = (int64_t)hu.cfg.size(), Nd = (int64_t)hd.cfg.size(), dim = Nu * Nd;
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("qbh_mf_hubbard: bad row range");
        return QBH_EINVAL;
    }
    // nnz of the equivalent CSR shard (closed form, as in qbh_gen_hubbard)
    std::vector<int64_t> pre_d((size_t)Nd + 1, 0), base_u((size_t)Nu + 1, 0);
    for (int64_t d = 0; d < Nd; ++d) pre_d[d + 1] = pre_d[d] + (hd.ptr[d + 1] - hd.ptr[d]);
    for (int64_t u = 0; u < Nu; ++u) base_u[u + 1] = base_u[u] + Nd * (1 + (hu.ptr[u + 1] - hu.ptr[u])) + pre_d[Nd];
    auto rowptr = [&](int64_t row) -> int64_t {
        if (row >= dim) return base_u[Nu];
        const int64_t u = row / Nd, d = row - u * Nd;
        return base_u[u] + d * (1 + (hu.ptr[u + 1] - hu.ptr[u])) + pre_d[d];
    };
    if (Nu >= (1 << 24) || Nd >= (1 << 24)) {              // before anything is allocated
        set_error("qbh_mf_hubbard: more than 2^24 configurations per species");
        return QBH_EUNSUPP;
    }
    MfHubbard m;
    m.Nu = Nu;
    m.Nd = Nd;
    m.U = U;
    auto tables = [&]() {                    // the device arrays placed so far
        std::vector<void *> own;
        for (void *q : {(void *)m.cfg_u, (void *)m.cfg_d, (void *)m.tgt_u, (void *)m.tgt_d, (void *)m.val_u, (void *)m.val_d, (void *)m.pk_d})
            if (q) own.push_back(q);
        return own;
    };
    auto build = [&]() -> int {
    QBH_HIP(qbh::dev_alloc(&m.cfg_u, (size_t)Nu * sizeof(uint32_t)));
    QBH_HIP(qbh::dev_alloc(&m.cfg_d, (size_t)Nd * sizeof(uint32_t)));
    QBH_HIP(hipMemcpy(m.cfg_u, hu.cfg.data(), (size_t)Nu * sizeof(uint32_t), hipMemcpyHostToDevice));
    QBH_HIP(hipMemcpy(m.cfg_d, hd.cfg.data(), (size_t)Nd * sizeof(uint32_t), hipMemcpyHostToDevice));
    HopTableView vu{Nu, hu.ptr.data(), hu.tgt.data(), hu.val.data()}, vd{Nd, hd.ptr.data(), hd.tgt.data(), hd.val.data()};
    std::vector<double> amp(1, 0.0);
    QBH_TRY(upload_ell(vu, amp, &m.wu, &m.tgt_u, &m.val_u));
    QBH_TRY(upload_ell(vd, amp, &m.wd, &m.tgt_d, &m.val_d));
    for (size_t c = 0; c < amp.size(); ++c) m.amp[c] = amp[c];
    {   // packed copy of the down-species table for the row-staged kernel
        std::vector<uint32_t> pk((size_t)m.wd * Nd, 0u);
        for (int64_t d = 0; d < Nd; ++d)
            for (int k = 0; k < m.wd; ++k) pk[((size_t)(k / 4) * Nd + d) * 4 + (k & 3)] = (uint32_t)d;     // padding: self, code 0
        for (int64_t d = 0; d < Nd; ++d)
            for (int q = hd.ptr[d]; q < hd.ptr[d + 1]; ++q) {
                const int k = q - hd.ptr[d];
                int code = 0;
                for (size_t c = 0; c < amp.size(); ++c)
                    if (amp[c] == hd.val[q]) code = (int)c;
                pk[((size_t)(k / 4) * Nd + d) * 4 + (k & 3)] = (uint32_t)hd.tgt[q] | ((uint32_t)code << 24);
            }
        QBH_HIP(qbh::dev_alloc(&m.pk_d, pk.size() * sizeof(uint32_t)));
        QBH_HIP(hipMemcpy(m.pk_d, pk.data(), pk.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return QBH_OK;
    };
    int rc = build();
    if (rc == QBH_OK)                        // t and U are real
        rc = adopt_mf(out, 1, &qbh_csr::mf, m, tables(), (m.Nu * m.wu + m.Nd * m.wd) * 5 + m.Nd * m.wd * 4 + (m.Nu + m.Nd) * 4, true,
                      row_end - row_begin, dim, row_begin, rowptr(row_end) - rowptr(row_begin), opts);
    if (rc != QBH_OK)                        // the handle takes the tables only when adoption succeeds
        for (void *q : tables()) (void)hipFree(q);
    return rc;
}

extern "C" int qbh_gen_heisenberg(qbh_csr **out, int n_sites, int n_dn, int n_bonds, const int32_t *bonds, double J,
                                  int64_t row_begin, int64_t row_end, const qbh_opts *opts)
{
    using namespace qbh;
    if (!out || !bonds || n_sites <= 0 || n_sites > 63 || n_dn < 0 || n_dn > n_sites || n_dn > 33 || n_bonds <= 0) {
        set_error("qbh_gen_heisenberg: invalid lattice / magnetisation");
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP(hipSetDevice(opts->device));
    std::map<std::pair<int, int>, double> bmap;
    QBH_TRY(merge_bonds(n_sites, n_bonds, bonds, bmap));
    if ((int)bmap.size() > kMaxBonds) {
        set_error("qbh_gen_heisenberg: more than %d distinct bonds", kMaxBonds);
        return QBH_EUNSUPP;
    }
    std::vector<HeisDev> hh(1);
    HeisDev &h = hh[0];
    memset(&h, 0, sizeof(h));
    for (int p = 0; p <= 64; ++p)
        for (int k = 0; k <= 33; ++k) h.binom[p][k] = binom_u64(p, k);
    h.n_sites = n_sites;
    h.n_dn = n_dn;
    h.n_bonds = 0;
    for (const auto &bw : bmap) {
        h.sa[h.n_bonds] = bw.first.first;
        h.sb[h.n_bonds] = bw.first.second;
        h.offd[h.n_bonds] = 0.5 * J * bw.second;
        h.diag[h.n_bonds] = 0.25 * J * bw.second;
        h.n_bonds++;
    }
    const uint64_t dim_u = binom_u64(n_sites, n_dn);
    if (dim_u >= 2147483647ULL) {
        set_error("qbh_gen_heisenberg: dim %llu exceeds int32 columns", (unsigned long long)dim_u);
        return QBH_EUNSUPP;
    }
    const int64_t dim = (int64_t)dim_u;
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("qbh_gen_heisenberg: bad row range");
        return QBH_EINVAL;
    }
    const int64_t nrows = row_end - row_begin;
    std::vector<void *> pool;
    HeisDev *d_h = nullptr;
    QBH_TRY(upload(hh, &d_h, pool));
    int32_t *d_cnt = nullptr;
    int64_t *d_ia = nullptr;
    int32_t *d_ja = nullptr;
    d2 *d_val = nullptr;
    int64_t nnz = 0;
    int rc = QBH_OK;
    hipError_t e = qbh::dev_alloc(&d_cnt, (size_t)nrows * sizeof(int32_t));
    if (e == hipSuccess) e = qbh::dev_alloc(&d_ia, (size_t)(nrows + 1) * sizeof(int64_t));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_heis_count, dim3(blas_grid(nrows)), dim3(256), 0, 0, d_h, row_begin, row_end, d_cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) rc = exclusive_scan(d_cnt, nrows, d_ia, 0);
    if (e == hipSuccess && rc == QBH_OK)
        e = hipMemcpy(&nnz, d_ia + nrows, sizeof(int64_t), hipMemcpyDeviceToHost);
    if (d_cnt) (void)hipFree(d_cnt);
    if (e == hipSuccess && rc == QBH_OK) e = qbh::dev_alloc(&d_ja, (size_t)nnz * sizeof(int32_t));
    if (e == hipSuccess && rc == QBH_OK) e = qbh::dev_alloc(&d_val, (size_t)nnz * sizeof(d2));
    if (e == hipSuccess && rc == QBH_OK) {
        hipLaunchKernelGGL(k_heis_fill, dim3(blas_grid(nrows)), dim3(256), 0, 0, d_h, row_begin, row_end, d_ia, d_ja,
                           d_val);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    free_pool(pool);
    if (e != hipSuccess || rc != QBH_OK) {
        if (e != hipSuccess) set_error("qbh_gen_heisenberg: %s", hipGetErrorString(e));
        (void)hipGetLastError();      // reported: not left sticky for the next call
        if (d_ia) (void)hipFree(d_ia);
        if (d_ja) (void)hipFree(d_ja);
        if (d_val) (void)hipFree(d_val);
        return rc != QBH_OK ? rc : (e == hipErrorOutOfMemory ? QBH_ENOMEM : QBH_EHIP);
    }
    // ownership passes with the call: on failure the arrays have already been released
    qbh_opts og;                                       // generated rows are in the generator's own order: nothing to look for
    opts_generated(opts, &og);
    // qbh_opts.sector_cut: a whole complex128 operator large enough for the split is held as a CUT sector (class-major, near / far /
    // cross parts) unless the caller named a basis or said -1.  The cut: h low sites such that every class fits the kernels' windows
    // (the limits basis_to_internal checks) with the fewest bonds across it -- those entries are the ones that stay unstructured.
    if (og.basis_kind == QBH_BASIS_NONE && og.sector_cut >= 0 && row_begin == 0 && row_end == dim && og.value_dict == 0 && og.real_fast_path == 0 &&
        og.kron_split != 0 && (og.kron_split == 2 || nnz >= 100000000) && n_sites <= 31) {
        int h = og.sector_cut;
        if (h == 0) {
            int best = -1, best_cross = 1 << 30;
            const int part_min = std::max(4, n_sites / 4);           // both parts of a cut hold a quarter of the sites at least
            for (int c = part_min; c <= n_sites - part_min; ++c) {
                if (n_sites - c > 24) continue;
                const int p_min = std::max(0, n_dn - c), p_max = std::min(n_sites - c, n_dn);
                if (p_max <= p_min || p_max - p_min + 1 > kKronMaxClasses) continue;
                bool ok = true;
                for (int p = p_min; p <= p_max && ok; ++p) {
                    ok = (double)binom_u64(n_sites - c, p) * 128.0 <= 2.5e6          // a band of the class's x inside an XCD's L2
                         && (double)binom_u64(c, n_dn - p) * 16.0 <= 4.0e6;         // ... and the window of x a block of the class gathers its near entries from
                }
                if (!ok) continue;
                int cross = 0;
                for (const auto &bw : bmap) cross += (bw.first.first < c) != (bw.first.second < c) ? 1 : 0;
                if (cross < best_cross || (cross == best_cross && std::abs(2 * c - n_sites) < std::abs(2 * best - n_sites))) {
                    best = c;
                    best_cross = cross;
                }
            }
            h = best;
        }
        if (h > 0) {
            og.basis_kind = QBH_BASIS_SPIN_SECTOR;
            og.n_sites = n_sites;
            og.n_up = h;
            og.n_dn = n_dn;
        }
    }
    return qbh_csr_create_device(out, nrows, dim, row_begin, nnz, d_ia, d_ja, reinterpret_cast<qbh_z *>(d_val), 1, &og);
}

// ---------------------------------------------- matrix-free Heisenberg operator --
extern "C" int qbh_mf_heisenberg(qbh_csr **out, int n_sites, int n_dn, int n_bonds, const int32_t *bonds, double J,
                                 int64_t row_begin, int64_t row_end, const qbh_opts *opts)
{
    using namespace qbh;
    if (!out || !bonds || n_sites <= 0 || n_sites > 62 || n_dn < 0 || n_dn > n_sites || n_dn > 33 || n_bonds <= 0) {
        set_error("qbh_mf_heisenberg: invalid lattice / magnetisation");
        return QBH_EINVAL;
    }
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    if (opts && opts->device >= 0) QBH_HIP(hipSetDevice(opts->device));
    std::map<std::pair<int, int>, double> bmap;
    QBH_TRY(merge_bonds(n_sites, n_bonds, bonds, bmap));
    const uint64_t dim_u = binom_u64(n_sites, n_dn);
    if (dim_u >= (1ULL << 62)) return QBH_EUNSUPP;
    const int64_t dim = (int64_t)dim_u;
    if (row_end < 0) row_end = dim;
    if (row_begin < 0 || row_begin >= row_end || row_end > dim) {
        set_error("qbh_mf_heisenberg: bad row range");
        return QBH_EINVAL;
    }
    const int nk = n_dn + 1, n_chunks = (n_sites + 5) / 6;
    std::vector<uint64_t> binom((size_t)(n_sites + 1) * nk), chunk((size_t)n_chunks * nk * 64, 0ULL);
    for (int p = 0; p <= n_sites; ++p)
        for (int k = 0; k < nk; ++k) binom[(size_t)p * nk + k] = binom_u64(p, k);
    // chunk[c][j][bits]: the t-th set bit of `bits` (site 6c + b) is the (j + t + 1)-th particle of the pattern
    for (int c = 0; c < n_chunks; ++c)
        for (int j = 0; j < nk; ++j)
            for (int bits = 0; bits < 64; ++bits) {
                uint64_t r = 0;
                int k = j;
                bool ok = true;
                for (int b = 0; b < 6; ++b)
                    if ((bits >> b) & 1) {
                        const int site = 6 * c + b;
                        ++k;
                        if (site >= n_sites || k > n_dn) {
                            ok = false;
                            break;
                        }
                        r += binom_u64(site, k);
                    }
                chunk[((size_t)c * nk + j) * 64 + bits] = ok ? r : 0ULL;
            }
    const int nb = (int)bmap.size(), nbp = ((nb + 7) / 8) * 8;
    std::vector<uint64_t> mask((size_t)nbp, 0ULL);
    std::vector<double> offd((size_t)nbp, 0.0), diag((size_t)nbp, 0.0);
    int i = 0;
    int64_t nnz_full = dim;
    for (const auto &bw : bmap) {
        mask[(size_t)i] = (1ULL << bw.first.first) | (1ULL << bw.first.second);
        offd[(size_t)i] = 0.5 * J * bw.second;
        diag[(size_t)i] = 0.25 * J * bw.second;
        if (n_sites >= 2 && n_dn >= 1 && n_dn <= n_sites - 1 && std::fabs(offd[(size_t)i]) >= QBH_SPARSE_PRECISION) nnz_full += 2 * (int64_t)binom_u64(n_sites - 2, n_dn - 1);
        ++i;
    }
    MfHeis t;
    t.n_sites = n_sites;
    t.n_dn = n_dn;
    t.n_real = nb;
    t.uniform = 1;
    for (int q = 1; q < nb; ++q)
        if (offd[(size_t)q] != offd[0]) t.uniform = 0;
    t.offd0 = nb > 0 ? offd[0] : 0.0;
    t.diag0 = nb > 0 ? diag[0] : 0.0;
    t.n_bonds = nbp;
    t.n_chunks = n_chunks;
    std::vector<void *> pool;
    int rc = upload(binom, &t.binom, pool);
    if (rc == QBH_OK) rc = upload(chunk, &t.chunk, pool);
    if (rc == QBH_OK) rc = upload(mask, &t.mask, pool);
    if (rc == QBH_OK) rc = upload(offd, &t.offd, pool);
    if (rc == QBH_OK) rc = upload(diag, &t.diag, pool);
    if (rc != QBH_OK) {
        free_pool(pool);
        return rc;
    }
    const int64_t nrows = row_end - row_begin;
    const int64_t nnz_equiv = (int64_t)((double)nnz_full * ((double)nrows / (double)dim));
    const int64_t bytes = ((int64_t)(t.n_sites + 1) * (t.n_dn + 1) + (int64_t)t.n_chunks * (t.n_dn + 1) * 64 + 3 * (int64_t)t.n_bonds) * 8;
    rc = adopt_mf(out, 2, &qbh_csr::mfh, t, pool, bytes, true, nrows, dim, row_begin, nnz_equiv, opts);      // J is real
    if (rc != QBH_OK) free_pool(pool);
    return rc;
}
