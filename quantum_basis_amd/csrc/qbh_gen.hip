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
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_dict.hpp"
#include "qbh_qudit.hpp"
#include "qbh_kondo.hpp"

namespace qbh {
namespace {

// ------------------------------------------------------------------ Hubbard ----
}  // namespace
struct HopTableView {
    int64_t n;
    const int32_t *ptr, *tgt;
    const double *val;
};
namespace {

struct HopTable {              // per configuration: sorted (target rank, amplitude) lists
    std::vector<uint32_t> cfg;
    std::vector<int32_t> ptr, tgt, nlo;
    std::vector<double> val;
};

void enumerate_configs(int L, int n, std::vector<uint32_t> &cfg)
{
    cfg.clear();
    if (n == 0) {
        cfg.push_back(0u);
        return;
    }
    // ascending bit patterns with n bits set among L (Gosper's hack)
    uint64_t c = (1ULL << n) - 1ULL, lim = 1ULL << L;
    while (c < lim) {
        cfg.push_back((uint32_t)c);
        const uint64_t t = c | (c - 1ULL);
        c = (t + 1ULL) | (((~t & (t + 1ULL)) - 1ULL) >> (__builtin_ctzll(c) + 1));
    }
}

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

template <typename T>
int upload(const std::vector<T> &h, T **d, std::vector<void *> &pool)
{
    const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    QBH_HIP(qbh::dev_alloc((void **)d, bytes));
    pool.push_back(*d);
    if (!h.empty()) QBH_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return QBH_OK;
}

void free_pool(std::vector<void *> &pool)
{
    for (void *p : pool) (void)hipFree(p);
    pool.clear();
}

// device arrays freed together when the owner goes out of scope, unless release() has handed them on
struct DevBufs {
    std::vector<void *> pool;
    DevBufs() = default;
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    ~DevBufs() { free_pool(pool); }
    template <typename T>
    hipError_t alloc(T **d, size_t bytes)
    {
        const hipError_t e = qbh::dev_alloc(d, bytes);
        if (e == hipSuccess) pool.push_back(*d);
        return e;
    }
    void release() { pool.clear(); }
};

// QBH_HIP with the public entry point's name `who` in front of the message
#define QBH_HIP_WHO(who, call)                                                            \
    do {                                                                                  \
        hipError_t _e = (call);                                                           \
        if (_e != hipSuccess) {                                                           \
            qbh::set_error("%s: %s failed: %s", (who), #call, hipGetErrorString(_e));     \
            (void)hipGetLastError();                                                      \
            return _e == hipErrorOutOfMemory ? QBH_ENOMEM : QBH_EHIP;                     \
        }                                                                                 \
    } while (0)

int merge_bonds(int n_sites, int n_bonds, const int32_t *bonds, std::map<std::pair<int, int>, double> &out)
{
    for (int i = 0; i < n_bonds; ++i) {
        int a = bonds[2 * i], b = bonds[2 * i + 1];
        if (a < 0 || b < 0 || a >= n_sites || b >= n_sites || a == b) {
            set_error("bond %d = (%d, %d) is invalid for %d sites", i, a, b, n_sites);
            return QBH_EINVAL;
        }
        if (a > b) std::swap(a, b);
        out[{a, b}] += 1.0;
    }
    return QBH_OK;
}

// ---------------------------------------------------------------- Heisenberg ---
constexpr int kMaxBonds = 192;

struct HeisDev {
    uint64_t binom[65][34];       // C(p, k), k <= 33
    int n_sites, n_dn, n_bonds;
    int sa[kMaxBonds], sb[kMaxBonds];
    double offd[kMaxBonds];       // 0.5 * J * w
    double diag[kMaxBonds];       // 0.25 * J * w
};

__device__ __forceinline__ uint64_t heis_unrank(const HeisDev &h, uint64_t r)
{
    uint64_t bits = 0;
    int p = h.n_sites - 1;
    for (int k = h.n_dn; k >= 1; --k) {
        while (h.binom[p][k] > r) --p;
        bits |= 1ULL << p;
        r -= h.binom[p][k];
        --p;
    }
    return bits;
}

__device__ __forceinline__ uint64_t heis_rank(const HeisDev &h, uint64_t bits)
{
    uint64_t r = 0;
    int k = 1;
    while (bits) {
        const int p = __ffsll((long long)bits) - 1;
        r += h.binom[p][k];
        bits &= bits - 1;
        ++k;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_heis_count(const HeisDev *hp, int64_t row_begin, int64_t row_end,
                                                    int32_t *cnt)
{
    const HeisDev &h = *hp;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t row = row_begin + (int64_t)blockIdx.x * 256 + threadIdx.x; row < row_end; row += stride) {
        const uint64_t s = heis_unrank(h, (uint64_t)row);
        int c = 1;
        for (int bnd = 0; bnd < h.n_bonds; ++bnd) c += (int)(((s >> h.sa[bnd]) ^ (s >> h.sb[bnd])) & 1ULL);
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

uint64_t binom_u64(int n, int k)
{
    if (k < 0 || k > n) return 0;
    long double r = 1.0L;
    uint64_t v = 1;
    k = std::min(k, n - k);
    for (int i = 1; i <= k; ++i) {
        v = v * (uint64_t)(n - k + i) / (uint64_t)i;      // exact: product of i consecutive ints divisible by i!
        r = r * (n - k + i) / i;
    }
    (void)r;
    return v;
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

namespace {
// hop table -> ELL (entry k of configuration c at [k*N + c]), padded to groups of 8 with (c, amplitude 0); targets as
// uint32, amplitudes as codes into amp[] (shared by both species)
int upload_ell(const qbh::HopTableView &H, std::vector<double> &amp, int *width, uint32_t **d_tgt, uint8_t **d_val)
{
    const int64_t N = H.n;
    int w = 0;
    for (int64_t i = 0; i < N; ++i) w = std::max(w, H.ptr[i + 1] - H.ptr[i]);
    w = std::max(8, ((w + 7) / 8) * 8);
    std::vector<uint32_t> tgt((size_t)w * N);
    std::vector<uint8_t> val((size_t)w * N, 0);               // code 0 = amplitude 0.0
    for (int k = 0; k < w; ++k)
        for (int64_t i = 0; i < N; ++i) tgt[(size_t)k * N + i] = (uint32_t)i;
    for (int64_t i = 0; i < N; ++i)
        for (int q = H.ptr[i]; q < H.ptr[i + 1]; ++q) {
            int code = -1;
            for (size_t c = 0; c < amp.size(); ++c)
                if (amp[c] == H.val[q]) code = (int)c;
            if (code < 0) {
                if (amp.size() == 16) {
                    qbh::set_error("qbh_mf_hubbard: more than 15 distinct hopping amplitudes");
                    return QBH_EUNSUPP;
                }
                amp.push_back(H.val[q]);
                code = (int)amp.size() - 1;
            }
            tgt[(size_t)(q - H.ptr[i]) * N + i] = (uint32_t)H.tgt[q];
            val[(size_t)(q - H.ptr[i]) * N + i] = (uint8_t)code;
        }
    *width = w;
    QBH_HIP(qbh::dev_alloc(d_tgt, tgt.size() * sizeof(uint32_t)));
    QBH_HIP(qbh::dev_alloc(d_val, val.size()));
    QBH_HIP(hipMemcpy(*d_tgt, tgt.data(), tgt.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    QBH_HIP(hipMemcpy(*d_val, val.data(), val.size(), hipMemcpyHostToDevice));
    return QBH_OK;
}
}  // namespace

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
    auto free_tables = [&]() {
        for (void *q : {(void *)m.cfg_u, (void *)m.cfg_d, (void *)m.tgt_u, (void *)m.tgt_d, (void *)m.val_u, (void *)m.val_d, (void *)m.pk_d})
            if (q) (void)hipFree(q);
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
    if (rc == QBH_OK) rc = adopt_mf_hubbard(out, m, row_end - row_begin, dim, row_begin, rowptr(row_end) - rowptr(row_begin), opts);
    if (rc != QBH_OK) free_tables();         // the handle takes the tables only when adoption succeeds
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
        if (n_sites >= 2 && n_dn >= 1 && n_dn <= n_sites - 1) nnz_full += 2 * (int64_t)binom_u64(n_sites - 2, n_dn - 1);
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
    rc = adopt_mf_heis(out, t, nrows, dim, row_begin, nnz_equiv, opts);
    if (rc != QBH_OK) free_pool(pool);
    return rc;
}

// ------------------------------------------------- translation-symmetric sectors --
// Device counterpart of model::generate_Ham_sparse_repr (src/model.cc:687-836) for spin-1/2 Heisenberg models:
// the Hamiltonian in the basis of momentum states built on orbit representatives.  The reference reaches the
// representative of a hopped state through its sublattice (Weisse) tables; here every state is canonicalised
// directly -- all |G| translations are applied with byte-sliced lookup tables and the smallest image wins.
//   basis      the orbit representatives of the fixed-n_dn sector (see k_sector_flag for what every family's basis holds)
//   H[a][b]    sum over bond terms taking |a> to c = l.b of h * conj(chi(g*)) * sqrt(|S_b|/|S_a|), g* c = b
//              (the phase exp(2 pi i k.d/L) * sqrt(nu_i/nu_j) of src/model.cc:808-814)
namespace qbh {
namespace {

constexpr int kReprMaxTrans = 64;

// the symmetry tables of a momentum sector: checks that translation 0 is the identity and every translation a site
// permutation, fills the binomials (unless binom is null) and the characters, stores the permutations in perm8
// (perm8[g * n_sites + site]) unless it is null and builds the chunk tables tab[(g*n_chunks + c)*64 + v] = scattered bits
// of chunk c with value v under g.  A site holds `bits` bits (1, 2 or 3), so a 6-bit chunk holds 6 / bits whole sites.
// `who` prefixes error messages.
int sector_symmetry(int n_sites, int n_trans, const int32_t *perms, const double *chars, const char *who, uint64_t (*binom)[34],
                    double *chr, int8_t *perm8, int &n_chunks, std::vector<uint64_t> &tab, int bits = 1)
{
    for (int i = 0; i < n_sites; ++i)
        if (perms[i] != i) {
            set_error("%s: translation 0 must be the identity", who);
            return QBH_EINVAL;
        }
    for (int g = 0; g < n_trans; ++g) {
        std::vector<int> seen((size_t)n_sites, 0);
        for (int s = 0; s < n_sites; ++s) {
            const int img = perms[(size_t)g * n_sites + s];
            if (img < 0 || img >= n_sites || seen[(size_t)img]++) {
                set_error("%s: translation %d is not a site permutation", who, g);
                return QBH_EINVAL;
            }
            if (perm8) perm8[g * n_sites + s] = (int8_t)img;
        }
    }
    if (binom)
        for (int p = 0; p <= 64; ++p)
            for (int k = 0; k <= 33; ++k) binom[p][k] = binom_u64(p, k);
    for (int g = 0; g < n_trans; ++g) {
        chr[2 * g] = chars[2 * g];
        chr[2 * g + 1] = chars[2 * g + 1];
    }
    const int per = 6 / bits;                 // sites per chunk
    const uint64_t field = (1ULL << bits) - 1ULL;
    n_chunks = (n_sites + per - 1) / per;
    tab.assign((size_t)n_trans * n_chunks * 64, 0ULL);
    for (int g = 0; g < n_trans; ++g)
        for (int c = 0; c < n_chunks; ++c)
            for (int v = 0; v < 64; ++v) {
                uint64_t m = 0;
                for (int b = 0; b < per; ++b) {
                    const int site = per * c + b;
                    const uint64_t l = ((uint64_t)v >> (b * bits)) & field;
                    if (site < n_sites && l) m |= l << (perms[(size_t)g * n_sites + site] * bits);
                }
                tab[((size_t)g * n_chunks + c) * 64 + v] = m;
            }
    return QBH_OK;
}

// image of bit pattern s under translation g; tab[(g*n_chunks + c)*64 + v] = scattered bits of chunk c with value v
__device__ __forceinline__ uint64_t repr_translate(const uint64_t *tab, int n_chunks, int g, uint64_t s)
{
    uint64_t out = 0;
    const uint64_t *t = tab + (size_t)g * n_chunks * 64;
    for (int c = 0; c < n_chunks; ++c) out |= t[c * 64 + ((s >> (6 * c)) & 63ULL)];
    return out;
}

__device__ __forceinline__ uint64_t unrank_k(const uint64_t (*binom)[34], int n_sites, int k, uint64_t r)
{
    uint64_t bits = 0;
    int p = n_sites - 1;
    for (; k >= 1; --k) {
        while (binom[p][k] > r) --p;
        bits |= 1ULL << p;
        r -= binom[p][k];
        --p;
    }
    return bits;
}

// next bit pattern with the same popcount (Gosper)
__device__ __forceinline__ uint64_t next_same_popcount(uint64_t s)
{
    const uint64_t t2 = s | (s - 1ULL);
    return (t2 + 1ULL) | (((~t2 & (t2 + 1ULL)) - 1ULL) >> (__ffsll((long long)s)));
}

// ---- what a sector family is ----
// A family is a device struct Dev (n_trans, n_chunks, chr, fake_pos and its own terms) with, next to it,
//   sector_word_count(R, ctab)      host: the number of words of the sector (UINT64_MAX if that overflows); a family whose
//                                   cursor reads a counting table on the device leaves it in ctab, and
//   sector_tables(R, ctab, pool)    uploads it and points R at it (default: nothing)
//   sector_seek(R, r)               the cursor at the word of rank r (ascending words); sector_word(R, cur) the word under it,
//   sector_step(R, cur)             the step to the next word
//   sector_allowed(R, s)            whether word s is in the space at all (default: yes)
//   sector_translate(R, tab, g, s)  the image of s under translation g (default: one field of n_chunks chunks)
//   sector_parity(R, g, s)          1 if T_g |s> = -|g(s)> (default: 0, no signs)
//   sector_row(R, ...), max_row<Dev>  one row of the sector operator and its capacity
// The defaults below serve a family whose word is one field and whose cursor is the word itself; a family with more
// structure overloads them for its struct.
template <class Dev> int sector_tables(Dev &, const std::vector<uint64_t> &, std::vector<void *> &) { return QBH_OK; }
template <class Dev> __device__ __forceinline__ uint64_t sector_word(const Dev &, uint64_t cur) { return cur; }
template <class Dev> __device__ __forceinline__ bool sector_allowed(const Dev &, uint64_t) { return true; }
template <class Dev> __device__ __forceinline__ int sector_parity(const Dev &, int, uint64_t) { return 0; }
template <class Dev>
__device__ __forceinline__ uint64_t sector_translate(const Dev &R, const uint64_t *tab, int g, uint64_t s)
{
    return repr_translate(tab, R.n_chunks, g, s);
}
template <class Dev> constexpr int max_row = 0;

// ---- the row toolkit of the families: everything from the point where a term's value v and its column are known ----
// smallest image of s and the translation that produces it
template <class Dev>
__device__ __forceinline__ uint64_t sector_canonical(const Dev &R, const uint64_t *tab, uint64_t s, int *gstar)
{
    uint64_t best = s;
    int gb = 0;                           // g = 0 is the identity
    for (int g = 1; g < R.n_trans; ++g) {
        const uint64_t t = sector_translate(R, tab, g, s);
        if (t < best) {
            best = t;
            gb = g;
        }
    }
    *gstar = gb;
    return best;
}

// position of representative b in the ascending list reps[0, dim)
__device__ __forceinline__ int64_t sector_find(const uint64_t *reps, int64_t dim, uint64_t b)
{
    int64_t lo = 0, hi = dim;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (reps[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the row of a representative whose norm vanishes at this momentum: it stays in the basis, decoupled, with the fake diagonal
// fake_pos + i/dim (src/model.cc:735-740)
__device__ __forceinline__ int row_zero_norm(double fake_pos, int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    cols[0] = (int32_t)i;
    vals[0] = d2{fake_pos + (double)i / (double)dim, 0.0};
    return 1;
}

// v at column lo among the entries [first, n): added to that column if the row has it, else appended while there is room
__device__ __forceinline__ void row_merge(int32_t *cols, d2 *vals, int &n, int cap, int first, int64_t lo, d2 v)
{
    int q = first;
    while (q < n && cols[q] != (int32_t)lo) ++q;
    if (q < n) {
        vals[q] += v;
    } else if (n < cap) {
        cols[n] = (int32_t)lo;
        vals[n] = v;
        ++n;
    }
}

// v at column lo of row i, whose slot 0 is kept for the diagonal dg
__device__ __forceinline__ void row_add(int32_t *cols, d2 *vals, int &n, int cap, int64_t i, int64_t lo, d2 v, d2 &dg)
{
    if (lo == i) dg += v;
    else row_merge(cols, vals, n, cap, 1, lo, v);
}

__device__ __forceinline__ void row_sort(int32_t *cols, d2 *vals, int m)      // insertion sort by column (rows are short)
{
    for (int q = 1; q < m; ++q) {
        const int32_t c = cols[q];
        const d2 v = vals[q];
        int p = q - 1;
        while (p >= 0 && cols[p] > c) {
            cols[p + 1] = cols[p];
            vals[p + 1] = vals[p];
            --p;
        }
        cols[p + 1] = c;
        vals[p + 1] = v;
    }
}

// the diagonal into slot 0, cancelled off-diagonal entries dropped (lil_mat::add, src/sparse.cc:72-77), columns ascending;
// returns the row's length
__device__ __forceinline__ int row_finish(int32_t *cols, d2 *vals, int n, d2 dg)
{
    vals[0] = dg;
    int m = 1;
    for (int q = 1; q < n; ++q)
        if (vals[q].x * vals[q].x + vals[q].y * vals[q].y >= 1e-28) {
            cols[m] = cols[q];
            vals[m] = vals[q];
            ++m;
        }
    row_sort(cols, vals, m);
    return m;
}

// ------------------------------------ spin-1/2 family (qbh_gen_heisenberg_repr) --
constexpr int kReprMaxRow = 160;          // distinct columns in one row (unique bonds + diagonal)

struct ReprDev {
    HeisDev h;                            // binomials, bonds, amplitudes
    int n_trans, n_chunks;
    double chr[2 * kReprMaxTrans];        // characters chi(g)
    double fake_pos;
};
template <> constexpr int max_row<ReprDev> = kReprMaxRow;

uint64_t sector_word_count(const ReprDev &R, std::vector<uint64_t> &) { return binom_u64(R.h.n_sites, R.h.n_dn); }
__device__ __forceinline__ uint64_t sector_seek(const ReprDev &R, uint64_t r) { return heis_unrank(R.h, r); }
__device__ __forceinline__ void sector_step(const ReprDev &, uint64_t &cur) { cur = next_same_popcount(cur); }

// one row of the sector Hamiltonian into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int repr_row(const ReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                        int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double si = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    int n = 1;
    cols[0] = (int32_t)i;
    d2 dg = {0.0, 0.0};
    for (int bnd = 0; bnd < R.h.n_bonds; ++bnd) {
        const int x = R.h.sa[bnd], y = R.h.sb[bnd];
        if (((a >> x) ^ (a >> y)) & 1ULL) {
            dg.x -= R.h.diag[bnd];
            const uint64_t c = a ^ (1ULL << x) ^ (1ULL << y);
            int g = 0;
            const uint64_t b = sector_canonical(R, tab, c, &g);
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;      // zero-norm target: dropped (src/model.cc:806)
            const double f = R.h.offd[bnd] * sqrt((double)(cj & 0x7f) / si);
            const d2 v = {f * R.chr[2 * g], -f * R.chr[2 * g + 1]};          // h * conj(chi(g*)) * sqrt(|S_b|/|S_a|)
            row_add(cols, vals, n, kReprMaxRow, i, lo, v, dg);
        } else {
            dg.x += R.h.diag[bnd];
        }
    }
    return row_finish(cols, vals, n, dg);
}

__device__ __forceinline__ int sector_row(const ReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim,
                                          int64_t i, int32_t *cols, d2 *vals)
{
    return repr_row(R, tab, reps, info, dim, i, cols, vals);
}

// moprXvec_repr for S^z_q (src/model.cc:1715-1846, diagonal branch :1756-1759): in the basis of ALL representatives the
// operator sum_s c_s S^z_s with c_{g(s)} = eta(g) c_s maps |a, k> to z_a |a, k * eta>, z_a = sum_s c_s s^z_s(a) evaluated on
// the representative itself (the stabiliser, hence the normalisation, does not depend on the momentum); representatives
// whose norm vanishes at the NEW momentum get 0.  info_new[] comes from the enumeration with the new characters.
struct SpinCoefR { double re[64], im[64]; };
__global__ __launch_bounds__(256) void k_repr_apply_sz(int n_sites, const uint64_t *reps, const uint8_t *info_new, int64_t dim,
                                                       SpinCoefR cf, const d2 *x_old, d2 *y_new)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += stride) {
        d2 out = {0.0, 0.0};
        if (!(info_new[i] & 0x80)) {
            const uint64_t s = reps[i];
            double zr = 0.0, zi = 0.0;
            for (int site = 0; site < n_sites; ++site) {
                const double sz = ((s >> site) & 1ULL) ? -0.5 : 0.5;
                zr += sz * cf.re[site];
                zi += sz * cf.im[site];
            }
            const d2 x = x_old[i];
            out = d2{zr * x.x - zi * x.y, zr * x.y + zi * x.x};
        }
        y_new[i] = out;
    }
}

// moprXvec_repr, off-diagonal branch (src/model.cc:1760-1830), for S^-_q / S^+_q = sum_s c_s S^-+_s with c_{g(s)} = eta(g) c_s:
//   A_q |a, k> = sum_s c_s chi_k'(g*) sqrt(|S_b| / |S_a|) |b, k'>,   c = a with spin s flipped,  b = g* c its representative,
// k' = k * eta, in the convention |a, k> = (|G| |S_a|)^(-1/2) sum_g chi_k(g) T_g |a> of the sector generator (H[a][b] =
// h conj(chi(g*)) sqrt(|S_b|/|S_a|) is the conjugate-transposed statement of the same formula).  One lane per SOURCE
// representative; contributions are added with fp64 atomics (the reference adds them inside a critical section).
__global__ __launch_bounds__(128) void k_repr_apply_flip(const ReprDev *Rnew, const uint64_t *tab, const uint64_t *reps_old,
                                                         const uint8_t *info_old, int64_t dim_old, const uint64_t *reps_new,
                                                         const uint8_t *info_new, int64_t dim_new, int lower, SpinCoefR cf,
                                                         const d2 *x_old, double *y_new)
{
    const ReprDev &R = *Rnew;                  // characters of the TARGET momentum
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x; i < dim_old; i += stride) {
        const uint8_t ci = info_old[i];
        if (ci & 0x80) continue;               // zero norm at the source momentum
        const d2 x = x_old[i];
        if (x.x == 0.0 && x.y == 0.0) continue;
        const uint64_t a = reps_old[i];
        const double sa = (double)(ci & 0x7f);
        for (int site = 0; site < R.h.n_sites; ++site) {
            const bool down = (a >> site) & 1ULL;
            if (lower ? down : !down) continue;   // S^- acts on an up spin (bit 0), S^+ on a down spin (bit 1)
            const uint64_t c = a ^ (1ULL << site);
            int g = 0;
            const uint64_t b = sector_canonical(R, tab, c, &g);
            const int64_t lo = sector_find(reps_new, dim_new, b);
            const uint8_t cj = info_new[lo];
            if (cj & 0x80) continue;           // zero norm at the target momentum
            const double f = sqrt((double)(cj & 0x7f) / sa);
            // w = coef[site] * chi_k'(g*) * f
            const double wr = f * (cf.re[site] * R.chr[2 * g] - cf.im[site] * R.chr[2 * g + 1]);
            const double wi = f * (cf.re[site] * R.chr[2 * g + 1] + cf.im[site] * R.chr[2 * g]);
            atomicAdd(&y_new[2 * lo], wr * x.x - wi * x.y);
            atomicAdd(&y_new[2 * lo + 1], wr * x.y + wi * x.x);
        }
    }
}

// ------------------------------------ Hubbard family in translation-symmetric sectors --
// Device counterpart of model::enumerate_basis_repr + generate_Ham_sparse_repr (src/model.cc:687-836) for two-species
// fermions (the reference's examples/trans_symmetric/latt_square/square_Fermi_Hubbard.cc).  A basis state is the pair of
// occupation patterns (u, d) with the operator order "all up (ascending site), then all down", stored as the word
// s = u | d << n_sites (ascending words: rank = rank(d) * C(n, n_up) + rank(u)); a translation g maps c^dag_{i,sigma} to
// c^dag_{g(i),sigma}, so
//     T_g |u, d> = sgn(g, u) sgn(g, d) |g(u), g(d)>,   sgn = parity of the inversions among the images of the occupied sites,
// and the norm of a representative is the SIGNED character sum over its stabiliser.  The operator is a list of directed
// one-body terms  amp_sigma * c^dag_{i,sigma} c_{j,sigma}  plus U sum_i n_{i,up} n_{i,dn}; it must commute with the
// translations (a Hamiltonian does; a single-site operator has to be translation-averaged first, exactly as
// measure_repr_static does, src/model.cc:1874-1888).  With |a,k> = (|G||S_a|)^(-1/2) sum_g chi_k(g) T_g |a>, row a holds
//     O[a][b] = sum over terms that move a particle of a from i to j, giving c with T_{g*} |c> = sigma |b>:
//               amp * (hop sign) * sigma * conj(chi_k(g*)) * sqrt(|S_b| / |S_a|).
constexpr int kHubReprMaxTerms = 512;
constexpr int kHubReprMaxPairs = 256;
constexpr int kHubReprMaxRow = 160;       // distinct columns in one row: one move per bond and species, one exchange, the diagonal

struct HubReprDev {
    uint64_t binom[65][34];
    int n_sites, n_up, n_dn, n_terms, n_trans, n_chunks;
    int8_t ti[kHubReprMaxTerms], tj[kHubReprMaxTerms];     // term t: amp * c^dag_{ti} c_{tj}
    double aup[kHubReprMaxTerms][2], adn[kHubReprMaxTerms][2];
    int n_pairs;                                           // density-density terms v * n_{pi,s} n_{pj,s'}
    int8_t pi[kHubReprMaxPairs], pj[kHubReprMaxPairs];
    double pv[kHubReprMaxPairs][4];                        // (up,up) (up,dn) (dn,up) (dn,dn)
    int n_exch, no_double;                                 // spin-exchange terms xa * (S+_i S-_j + S-_i S+_j); t-J constraint
    int8_t xi[kHubReprMaxPairs], xj[kHubReprMaxPairs];
    double xa[kHubReprMaxPairs];
    double U, fake_pos;
    double chr[2 * kReprMaxTrans];
    int8_t perm[kReprMaxTrans * 32];                       // perm[g * n_sites + site]
};
template <> constexpr int max_row<HubReprDev> = kHubReprMaxRow;

uint64_t sector_word_count(const HubReprDev &R, std::vector<uint64_t> &)
{
    const uint64_t cu = binom_u64(R.n_sites, R.n_up), cd = binom_u64(R.n_sites, R.n_dn);
    return cu > UINT64_MAX / cd ? UINT64_MAX : cu * cd;
}

struct HubCursor { uint64_t u, d, ru; };                   // the two patterns and the rank of the up pattern

__device__ __forceinline__ HubCursor sector_seek(const HubReprDev &R, uint64_t r)
{
    const uint64_t cu = R.binom[R.n_sites][R.n_up];
    HubCursor c;
    c.ru = r % cu;
    c.u = unrank_k(R.binom, R.n_sites, R.n_up, c.ru);
    c.d = unrank_k(R.binom, R.n_sites, R.n_dn, r / cu);
    return c;
}
__device__ __forceinline__ uint64_t sector_word(const HubReprDev &R, const HubCursor &c) { return c.u | (c.d << R.n_sites); }
__device__ __forceinline__ void sector_step(const HubReprDev &R, HubCursor &c)
{
    if (++c.ru == R.binom[R.n_sites][R.n_up]) {            // next down pattern, up patterns start over
        c.ru = 0;
        c.u = (R.n_up > 0) ? ((1ULL << R.n_up) - 1ULL) : 0ULL;
        c.d = R.n_dn > 0 ? next_same_popcount(c.d) & ((1ULL << R.n_sites) - 1ULL) : 0ULL;
    } else {
        c.u = next_same_popcount(c.u);
    }
}
// t-J: words with a doubly occupied site are not in the space
__device__ __forceinline__ bool sector_allowed(const HubReprDev &R, uint64_t s)
{
    return !(R.no_double && (s & (s >> R.n_sites) & ((1ULL << R.n_sites) - 1ULL)));
}
__device__ __forceinline__ uint64_t sector_translate(const HubReprDev &R, const uint64_t *tab, int g, uint64_t s)
{
    const uint64_t m = (1ULL << R.n_sites) - 1ULL;
    const uint64_t u = repr_translate(tab, R.n_chunks, g, s & m), d = repr_translate(tab, R.n_chunks, g, s >> R.n_sites);
    return u | (d << R.n_sites);
}

// parity (0 / 1) of the permutation that sorts the images of the occupied sites of `occ` under translation g
__device__ __forceinline__ int hubrepr_parity(const HubReprDev &R, int g, uint64_t occ)
{
    const int8_t *p = R.perm + g * R.n_sites;
    uint64_t seen = 0;
    int par = 0;
    while (occ) {
        const int i = __ffsll((long long)occ) - 1;
        occ &= occ - 1;
        const int img = p[i];
        par ^= __popcll(seen >> img) & 1;                  // images placed so far that lie above this one
        seen |= 1ULL << img;
    }
    return par;
}
__device__ __forceinline__ int sector_parity(const HubReprDev &R, int g, uint64_t s)
{
    return hubrepr_parity(R, g, s & ((1ULL << R.n_sites) - 1ULL)) ^ hubrepr_parity(R, g, s >> R.n_sites);
}

// smallest image, the translation that produces it and the sign of T_{g*}
__device__ __forceinline__ uint64_t hubrepr_canonical(const HubReprDev &R, const uint64_t *tab, uint64_t s, int *gstar, int *parity)
{
    const uint64_t best = sector_canonical(R, tab, s, gstar);
    *parity = *gstar ? sector_parity(R, *gstar, s) : 0;
    return best;
}

// one row of the sector operator into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int hubrepr_row(const HubReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                           int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double sa = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    const uint64_t mlow = (1ULL << R.n_sites) - 1ULL;
    const uint64_t au = a & mlow, ad = a >> R.n_sites;
    int n = 1;
    cols[0] = (int32_t)i;
    d2 dg = {R.U * (double)__popcll(au & ad), 0.0};
    for (int p = 0; p < R.n_pairs; ++p) {
        const int iu = (int)((au >> R.pi[p]) & 1ULL), id = (int)((ad >> R.pi[p]) & 1ULL);
        const int ju = (int)((au >> R.pj[p]) & 1ULL), jd = (int)((ad >> R.pj[p]) & 1ULL);
        dg.x += R.pv[p][0] * (iu & ju) + R.pv[p][1] * (iu & jd) + R.pv[p][2] * (id & ju) + R.pv[p][3] * (id & jd);
    }
    for (int t = 0; t < R.n_terms; ++t) {
        const int ti = R.ti[t], tj = R.tj[t];
        for (int sp = 0; sp < 2; ++sp) {
            const double ar = sp ? R.adn[t][0] : R.aup[t][0], ai = sp ? R.adn[t][1] : R.aup[t][1];
            if (ar == 0.0 && ai == 0.0) continue;
            const uint64_t occ = sp ? ad : au;
            if (ti == tj) {                                // number operator: diagonal
                if ((occ >> ti) & 1ULL) dg += d2{ar, ai};
                continue;
            }
            // row a of O = conj of O^dag |a>: the particle moves from ti to tj
            if (!((occ >> ti) & 1ULL) || ((occ >> tj) & 1ULL)) continue;
            if (R.no_double && (((sp ? au : ad) >> tj) & 1ULL)) continue;      // projected hopping
            const int lo_s = ti < tj ? ti : tj, hi_s = ti < tj ? tj : ti;
            const uint64_t between = ((1ULL << hi_s) - 1ULL) & ~((2ULL << lo_s) - 1ULL);
            int par = __popcll(occ & between) & 1;
            const uint64_t occ2 = occ ^ (1ULL << ti) ^ (1ULL << tj);
            const uint64_t c = sp ? (au | (occ2 << R.n_sites)) : (occ2 | (ad << R.n_sites));
            int g = 0, pt = 0;
            const uint64_t b = hubrepr_canonical(R, tab, c, &g, &pt);
            par ^= pt;
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;                       // zero-norm target
            const double f = (par ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
            // amp * conj(chi(g*)) * f
            const double cr = R.chr[2 * g], cim = -R.chr[2 * g + 1];
            const d2 v = {f * (ar * cr - ai * cim), f * (ar * cim + ai * cr)};
            row_add(cols, vals, n, kHubReprMaxRow, i, lo, v, dg);
        }
    }
    // spin exchange xa * (S+_i S-_j + S-_i S+_j): the up particle of one site and the down particle of the other trade
    // places.  S+_i S-_j = -(c^dag_{i,up} c_{j,up})(c^dag_{j,dn} c_{i,dn}): the product of the two hop signs, times -1.
    for (int e = 0; e < R.n_exch; ++e) {
        const int xi = R.xi[e], xj = R.xj[e];
        for (int dir = 0; dir < 2; ++dir) {
            const int su = dir ? xj : xi, sd = dir ? xi : xj;           // su carries the up particle, sd the down particle
            if (!((au >> su) & 1ULL) || ((ad >> su) & 1ULL) || !((ad >> sd) & 1ULL) || ((au >> sd) & 1ULL)) continue;
            const int lo_s = su < sd ? su : sd, hi_s = su < sd ? sd : su;
            const uint64_t between = ((1ULL << hi_s) - 1ULL) & ~((2ULL << lo_s) - 1ULL);
            int par = 1 ^ ((__popcll(au & between) + __popcll(ad & between)) & 1);
            const uint64_t u2 = au ^ (1ULL << su) ^ (1ULL << sd), d2w = ad ^ (1ULL << su) ^ (1ULL << sd);
            const uint64_t c = u2 | (d2w << R.n_sites);
            int g = 0, pt = 0;
            const uint64_t b = hubrepr_canonical(R, tab, c, &g, &pt);
            par ^= pt;
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;
            const double f = (par ? -1.0 : 1.0) * R.xa[e] * sqrt((double)(cj & 0x7f) / sa);
            const d2 v = {f * R.chr[2 * g], -f * R.chr[2 * g + 1]};
            row_add(cols, vals, n, kHubReprMaxRow, i, lo, v, dg);
        }
    }
    return row_finish(cols, vals, n, dg);
}

__device__ __forceinline__ int sector_row(const HubReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                          int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    return hubrepr_row(R, tab, reps, info, dim, i, cols, vals);
}

// moprXvec_repr (src/model.cc:1715-1846, diagonal branch :1756-1759) for O = sum_s ( c_up[s] n_{s,up} + c_dn[s] n_{s,dn} )
// with c_{g(s)} = eta(g) c_s (a density or S^z Fourier component).  Then O T_g = eta(g) T_g O, so O |a, k> = z_a |a, k*eta>
// with z_a evaluated on the representative itself: |S_a| does not depend on the momentum (the fermion signs sit inside
// T_g on both sides).  Representatives whose norm vanishes at the TARGET momentum get 0.
struct HubCoef { double up_re[32], up_im[32], dn_re[32], dn_im[32]; };

__global__ __launch_bounds__(256) void k_hubrepr_apply_diag(int n_sites, const uint64_t *reps, const uint8_t *info_new, int64_t dim,
                                                            HubCoef cf, const d2 *x_old, d2 *y_new)
{
    const uint64_t mlow = (1ULL << n_sites) - 1ULL;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += stride) {
        d2 y = {0.0, 0.0};
        if (!(info_new[i] & 0x80)) {
            const uint64_t a = reps[i];
            uint64_t u = a & mlow, d = a >> n_sites;
            double zr = 0.0, zi = 0.0;
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
            const d2 x = x_old[i];
            y = d2{zr * x.x - zi * x.y, zr * x.y + zi * x.x};
        }
        y_new[i] = y;
    }
}

// moprXvec_repr (src/model.cc:1715-1846, general branch) for  O = sum_s coef[s] c_{s,sigma}  (kind -1) or
// sum_s coef[s] c^dag_{s,sigma} (kind +1) with coef_{g(s)} = eta(g) coef_s -- the operators of the single-particle spectral
// function.  O T_g = eta(g) T_g O, so with chi' = chi * eta
//     O |a, k> = sum_s coef_s sgn_s(a) sigma(g_c) chi'(g_c) sqrt(|S_b| / |S_a|) |b, k'>,   c = a -/+ s,  T_{g_c} |c> = sigma |b>,
// sgn_s = (-1)^(operators left of (s, sigma) in the word's operator string: all up ascending, then all down ascending).
// One lane per old representative scatters into the new sector with fp64 atomics.
__global__ __launch_bounds__(128) void k_hubrepr_apply_c(const HubReprDev *Rnew, const uint64_t *tab, const uint64_t *reps_old,
                                                         const uint8_t *info_old, int64_t dim_old, const uint64_t *reps_new,
                                                         const uint8_t *info_new, int64_t dim_new, int species, int create,
                                                         HubCoef cf, const d2 *x_old, double *y_new)
{
    const HubReprDev &R = *Rnew;
    const int n = R.n_sites;
    const uint64_t mlow = (1ULL << n) - 1ULL;
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x; i < dim_old; i += stride) {
        const uint8_t ci = info_old[i];
        if (ci & 0x80) continue;
        const d2 x = x_old[i];
        if (x.x == 0.0 && x.y == 0.0) continue;
        const double sa = (double)(ci & 0x7f);
        const uint64_t a = reps_old[i];
        const uint64_t au = a & mlow, ad = a >> n;
        const uint64_t occ = species ? ad : au;
        const int left0 = species ? __popcll(au) : 0;      // the whole up block stands left of every down operator
        for (int s = 0; s < n; ++s) {
            const bool has = (occ >> s) & 1ULL;
            if (create ? has : !has) continue;
            const double cr0 = species ? cf.dn_re[s] : cf.up_re[s], ci0 = species ? cf.dn_im[s] : cf.up_im[s];
            if (cr0 == 0.0 && ci0 == 0.0) continue;
            int par = (left0 + __popcll(occ & ((1ULL << s) - 1ULL))) & 1;
            const uint64_t occ2 = occ ^ (1ULL << s);
            const uint64_t c = species ? (au | (occ2 << n)) : (occ2 | (ad << n));
            int g = 0, pt = 0;
            const uint64_t b = hubrepr_canonical(R, tab, c, &g, &pt);
            par ^= pt;
            const int64_t lo = sector_find(reps_new, dim_new, b);
            const uint8_t cj = info_new[lo];
            if (cj & 0x80) continue;
            const double f = (par ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
            // w = coef * chi'(g_c) * f
            const double wr = f * (cr0 * R.chr[2 * g] - ci0 * R.chr[2 * g + 1]);
            const double wi = f * (cr0 * R.chr[2 * g + 1] + ci0 * R.chr[2 * g]);
            atomicAdd(&y_new[2 * lo], wr * x.x - wi * x.y);
            atomicAdd(&y_new[2 * lo + 1], wr * x.y + wi * x.x);
        }
    }
}

// ------------------------------------ d-level sites in translation-symmetric sectors (qbh_gen_qudit_repr) --
// Words packed as in qbh_gen_qudit (site s in bits [s b, (s+1) b), qbh_qudit.hpp), so the chunk tables of sector_symmetry
// with `bits` = b translate them and the integer order of the words is the generator's order.  Row a:
//     O[a][b] = sum over the pair entries <a|M|c> that move a to c, b = g* c:  <a|M|c> * conj(chi(g*)) * sqrt(|S_b|/|S_a|)
// (the Heisenberg convention above; no signs: bosons and spins).
constexpr int kQuditReprMaxRow = 160;     // entries of one row before merging, counted from the merged terms

struct QuditReprDev {
    int n_sites, d, bits, total, tw, n_pairs, n_trans, n_chunks;
    double chr[2 * kReprMaxTrans];
    double fake_pos;
    const uint64_t *cum;                  // [n_sites * tw], qudit_table
    const int32_t *pair_ij, *eoff, *eout; // the term tables of QuditTerms
    const double *pdiag, *sdiag;
    const d2 *eval;
};
template <> constexpr int max_row<QuditReprDev> = kQuditReprMaxRow;

uint64_t sector_word_count(const QuditReprDev &R, std::vector<uint64_t> &cum)    // cum: the counting table of qd_unrank
{
    std::vector<uint64_t> dims;
    qudit_table(R.n_sites, R.d, R.tw, cum, dims);
    return dims[(size_t)R.total];
}
int sector_tables(QuditReprDev &R, const std::vector<uint64_t> &cum, std::vector<void *> &pool)
{
    uint64_t *d_cum = nullptr;
    QBH_TRY(upload(cum, &d_cum, pool));
    R.cum = d_cum;
    return QBH_OK;
}
__device__ __forceinline__ uint64_t sector_seek(const QuditReprDev &R, uint64_t r)
{
    return qd_unrank(R.cum, R.n_sites, R.d, R.bits, R.tw, R.total, r);
}
__device__ __forceinline__ void sector_step(const QuditReprDev &R, uint64_t &cur) { cur = qd_next(cur, R.n_sites, R.d, R.bits); }

// one row of the sector operator into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int qrepr_row(const QuditReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                         int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double sa = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    const int d2n = R.d * R.d;
    const uint64_t field = (1ULL << R.bits) - 1ULL;
    int n = 1;
    cols[0] = (int32_t)i;
    d2 dg = {0.0, 0.0};
    for (int s = 0; s < R.n_sites; ++s) dg.x += R.sdiag[s * R.d + qd_level(a, R.bits, s)];
    for (int p = 0; p < R.n_pairs; ++p) {
        const int ij = R.pair_ij[p];
        const int si = ij & 0xff, sj = ij >> 8;
        const int in = qd_level(a, R.bits, si) * R.d + qd_level(a, R.bits, sj);
        dg.x += R.pdiag[p * d2n + in];
        const int e1 = R.eoff[p * d2n + in + 1];
        for (int e = R.eoff[p * d2n + in]; e < e1; ++e) {
            const int o = R.eout[e];
            const uint64_t c = (a & ~((field << (si * R.bits)) | (field << (sj * R.bits)))) | ((uint64_t)(o & 0xff) << (si * R.bits)) |
                               ((uint64_t)(o >> 8) << (sj * R.bits));
            int g = 0;
            const uint64_t b = sector_canonical(R, tab, c, &g);
            const int64_t lo = sector_find(reps, dim, b);
            const uint8_t cj = info[lo];
            if (cj & 0x80) continue;      // zero-norm target: dropped
            const double f = sqrt((double)(cj & 0x7f) / sa);
            const d2 h = R.eval[e];
            const double cr = f * R.chr[2 * g], cim = -f * R.chr[2 * g + 1];        // conj(chi(g*)) * sqrt(|S_b|/|S_a|)
            const d2 v = {h.x * cr - h.y * cim, h.x * cim + h.y * cr};
            row_add(cols, vals, n, kQuditReprMaxRow, i, lo, v, dg);
        }
    }
    return row_finish(cols, vals, n, dg);
}

__device__ __forceinline__ int sector_row(const QuditReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                          int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    return qrepr_row(R, tab, reps, info, dim, i, cols, vals);
}

// moprXvec_repr (src/model.cc:1715-1846) for O_q = sum_s c_s O_s with c_{g(s)} = eta(g) c_s, from the sector (total, chi)
// to (total + dq, chi eta), gathered by TARGET row b: the entry for the source word c = b with the level of site s lowered
// by dq, a = g* c its representative, is  c_s <b_s|O|c_s> conj(chi(g*)) sqrt(|S_a| / |S_b|)  (the row formula of the sector
// operators with the source sector's characters).  Zero-norm targets get 0, zero-norm sources are skipped.
__global__ __launch_bounds__(256) void k_qrepr_mopr(const QuditReprDev *Rold, const uint64_t *tab, const uint64_t *reps_old,
                                                    const uint8_t *info_old, int64_t dim_old, const uint64_t *reps_new,
                                                    const uint8_t *info_new, int64_t dim_new, int dq, QuditMopr cf, const d2 *x_old,
                                                    d2 *y_new)
{
    const QuditReprDev &R = *Rold;
    const uint64_t field = (1ULL << R.bits) - 1ULL;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim_new; i += stride) {
        const uint8_t cb = info_new[i];
        double ar = 0.0, ai = 0.0;
        if (!(cb & 0x80)) {
            const uint64_t b = reps_new[i];
            const double sb = (double)(cb & 0x7f);
            for (int s = 0; s < R.n_sites; ++s) {
                const int l = qd_level(b, R.bits, s), ls = l - dq;
                if (ls < 0 || ls >= R.d) continue;
                const double lr = cf.la[l], li = cf.lb[l];
                if ((lr == 0.0 && li == 0.0) || (cf.ca[s] == 0.0 && cf.cb[s] == 0.0)) continue;
                const uint64_t c = (b & ~(field << (s * R.bits))) | ((uint64_t)ls << (s * R.bits));
                int g = 0;
                const uint64_t a = sector_canonical(R, tab, c, &g);
                const int64_t lo = sector_find(reps_old, dim_old, a);
                const uint8_t ca = info_old[lo];
                if (ca & 0x80) continue;
                const double f = sqrt((double)(ca & 0x7f) / sb);
                const double wr0 = cf.ca[s] * lr - cf.cb[s] * li, wi0 = cf.ca[s] * li + cf.cb[s] * lr;
                const double xr = f * R.chr[2 * g], xi = -f * R.chr[2 * g + 1];
                const double wr = wr0 * xr - wi0 * xi, wi = wr0 * xi + wi0 * xr;
                const d2 x = x_old[lo];
                ar += wr * x.x - wi * x.y;
                ai += wr * x.y + wi * x.x;
            }
        }
        y_new[i] = d2{ar, ai};
    }
}

// ------------------------------------ Kondo lattice in translation-symmetric sectors (qbh_gen_kondo_repr) --
// Words w = u | d << n | s << 2n as in qbh_gen_kondo (qbh_kondo.hpp): a translation permutes the sites of all three fields,
// the two electron fields carry the fermion sign of hubrepr_parity, the local spins none.  The sector is a union of
// particle-number blocks, so the cursor keeps the rank and seeks again where a block of s ends.  Row a as in
// qbh_gen_hubbard_repr: O[a][b] = sum of <a|H|c> sigma(g*) conj(chi(g*)) sqrt(|S_b|/|S_a|), b = g* c.
struct KondoReprDev {
    KondoDev k;                           // shape, counting tables, terms
    int n_trans, n_chunks;
    double chr[2 * kReprMaxTrans];
    double fake_pos;
    int8_t perm[kReprMaxTrans * kKondoMaxSites];           // perm[g * n_sites + site]
};
template <> constexpr int max_row<KondoReprDev> = kKondoMaxRow;

uint64_t sector_word_count(const KondoReprDev &R, std::vector<uint64_t> &) { return R.k.total; }

struct KondoCursor { uint64_t u, d, s, ru, rd, r; };       // the three fields, the ranks of u and d in their block, the word's rank

__device__ __forceinline__ KondoCursor sector_seek(const KondoReprDev &R, uint64_t r)
{
    KondoCursor c;
    c.r = r;
    kd_unrank(R.k, R.k.A, R.k.binom, r, &c.u, &c.d, &c.s, &c.ru, &c.rd);
    return c;
}
__device__ __forceinline__ uint64_t sector_word(const KondoReprDev &R, const KondoCursor &c)
{
    return c.u | (c.d << R.k.n_sites) | (c.s << (2 * R.k.n_sites));
}
__device__ __forceinline__ void sector_step(const KondoReprDev &R, KondoCursor &c)
{
    if (c.r + 1 >= R.k.total) return;                      // the last word stays
    ++c.r;
    const int n = R.k.n_sites, nu = R.k.nu0 + __popcll(c.s);
    if (++c.ru < R.k.binom[n * kKondoTab + nu]) {
        c.u = next_same_popcount(c.u);
    } else if (++c.rd < R.k.binom[n * kKondoTab + R.k.n_elec - nu]) {      // next down pattern, up patterns start over
        c.ru = 0;
        c.u = (1ULL << nu) - 1ULL;
        c.d = next_same_popcount(c.d);
    } else {
        c = sector_seek(R, c.r);                           // the block of this s is done: the next s may lie in another block
    }
}
__device__ __forceinline__ uint64_t sector_translate(const KondoReprDev &R, const uint64_t *tab, int g, uint64_t w)
{
    const int n = R.k.n_sites;
    const uint64_t m = (1ULL << n) - 1ULL;
    return repr_translate(tab, R.n_chunks, g, w & m) | (repr_translate(tab, R.n_chunks, g, (w >> n) & m) << n) |
           (repr_translate(tab, R.n_chunks, g, w >> (2 * n)) << (2 * n));
}
// parity (0 / 1) of the permutation that sorts the images of the occupied sites of `occ` under translation g
__device__ __forceinline__ int kondo_parity(const KondoReprDev &R, int g, uint64_t occ)
{
    const int8_t *p = R.perm + g * R.k.n_sites;
    uint64_t seen = 0;
    int par = 0;
    while (occ) {
        const int i = __ffsll((long long)occ) - 1;
        occ &= occ - 1;
        const int img = p[i];
        par ^= __popcll(seen >> img) & 1;
        seen |= 1ULL << img;
    }
    return par;
}
__device__ __forceinline__ int sector_parity(const KondoReprDev &R, int g, uint64_t w)
{
    const uint64_t m = (1ULL << R.k.n_sites) - 1ULL;
    return kondo_parity(R, g, w & m) ^ kondo_parity(R, g, (w >> R.k.n_sites) & m);
}

// one row of the sector operator into (cols, vals), columns ascending, duplicates merged; returns its length
__device__ int kondo_row(const KondoReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info, int64_t dim, int64_t i,
                         int32_t *cols, d2 *vals)
{
    const uint8_t ci = info[i];
    if (ci & 0x80) return row_zero_norm(R.fake_pos, dim, i, cols, vals);
    const double sa = (double)(ci & 0x7f);
    const uint64_t a = reps[i];
    const int nb = R.k.n_sites;
    const uint64_t mlow = (1ULL << nb) - 1ULL;
    int n = 1;
    cols[0] = (int32_t)i;
    d2 off = {0.0, 0.0};                  // what the moves add to the diagonal (a word that comes back to its own orbit)
    const d2 dg0 = kd_row_terms(R.k, a & mlow, (a >> nb) & mlow, a >> (2 * nb), [&](uint64_t u2, uint64_t d2w, uint64_t s2, int code) {
        const uint64_t c = u2 | (d2w << nb) | (s2 << (2 * nb));
        int g = 0;
        const uint64_t b = sector_canonical(R, tab, c, &g);
        const int pt = g ? sector_parity(R, g, c) : 0;
        const int64_t lo = sector_find(reps, dim, b);
        const uint8_t cj = info[lo];
        if (cj & 0x80) return;            // zero-norm target: dropped
        const double f = (pt ? -1.0 : 1.0) * sqrt((double)(cj & 0x7f) / sa);
        const d2 h = kd_value(R.k, code);
        const double cr = f * R.chr[2 * g], cim = -f * R.chr[2 * g + 1];          // sigma(g*) conj(chi(g*)) sqrt(|S_b|/|S_a|)
        const d2 v = {h.x * cr - h.y * cim, h.x * cim + h.y * cr};
        row_add(cols, vals, n, kKondoMaxRow, i, lo, v, off);
    });
    return row_finish(cols, vals, n, dg0 + off);
}

__device__ __forceinline__ int sector_row(const KondoReprDev &R, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                          int64_t dim, int64_t i, int32_t *cols, d2 *vals)
{
    return kondo_row(R, tab, reps, info, dim, i, cols, vals);
}

// moprXvec_repr, diagonal branch, for O = sum_s ( c_up[s] n_{s,up} + c_dn[s] n_{s,dn} + c_sp[s] S^z_s ) with every coefficient
// set transforming with the same character: O |a, k> = z_a |a, k * eta>, z_a evaluated on the representative (see
// k_hubrepr_apply_diag).  Representatives whose norm vanishes at the TARGET momentum get 0.
struct KondoCoef { double up_re[kKondoMaxSites], up_im[kKondoMaxSites], dn_re[kKondoMaxSites], dn_im[kKondoMaxSites],
                          sp_re[kKondoMaxSites], sp_im[kKondoMaxSites]; };

__global__ __launch_bounds__(256) void k_kondo_apply_diag(int n_sites, const uint64_t *reps, const uint8_t *info_new, int64_t dim,
                                                          KondoCoef cf, const d2 *x_old, d2 *y_new)
{
    const uint64_t mlow = (1ULL << n_sites) - 1ULL;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < dim; i += stride) {
        d2 y = {0.0, 0.0};
        if (!(info_new[i] & 0x80)) {
            const uint64_t a = reps[i];
            const uint64_t u = a & mlow, d = (a >> n_sites) & mlow, sp = a >> (2 * n_sites);
            double zr = 0.0, zi = 0.0;
            for (int s = 0; s < n_sites; ++s) {
                const double nu = (double)((u >> s) & 1ULL), nd = (double)((d >> s) & 1ULL);
                const double sz = ((sp >> s) & 1ULL) ? -0.5 : 0.5;
                zr += nu * cf.up_re[s] + nd * cf.dn_re[s] + sz * cf.sp_re[s];
                zi += nu * cf.up_im[s] + nd * cf.dn_im[s] + sz * cf.sp_im[s];
            }
            const d2 x = x_old[i];
            y = d2{zr * x.x - zi * x.y, zr * x.y + zi * x.x};
        }
        y_new[i] = y;
    }
}

// ------------------------------------ the enumeration and the row kernels every family shares --
// The basis of a sector is ALL orbit representatives (the smallest word of each orbit) of the family's words, ascending; a
// representative whose (signed) character sum over its stabiliser vanishes has zero norm at this momentum and stays in the
// basis as a decoupled fake row (row_zero_norm).  Two passes over the words in ascending order, one workgroup per chunk of
// kSectorChunk consecutive words, a lane seeking the first of its kSectorRun words and stepping from there.  Nothing is
// kept per word besides one code byte (4x5 Hubbard at half filling has 3.4e10 words): the counts are per chunk.
constexpr int kSectorRun = 16, kSectorChunk = kSectorRun * 256;

// pass 1: code[r] = 0 if the word of rank r is not a representative, else |S| | (zero-norm << 7); chunk_cnt = the number of
// representatives of each chunk
template <class Dev>
__global__ __launch_bounds__(256) void k_sector_flag(const Dev *Rp, const uint64_t *tab, int64_t nstates, uint8_t *code,
                                                     int32_t *chunk_cnt, int64_t nchunks)
{
    const Dev &R = *Rp;
    __shared__ int wsum[4];
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t r0 = chunk * kSectorChunk + (int64_t)threadIdx.x * kSectorRun;
        const int64_t r1 = (r0 + kSectorRun < nstates) ? r0 + kSectorRun : nstates;
        int mine = 0;
        if (r0 < nstates) {
            auto cur = sector_seek(R, (uint64_t)r0);
            for (int64_t r = r0; r < r1; ++r) {
                const uint64_t s = sector_word(R, cur);
                bool rep = sector_allowed(R, s);
                int nstab = 1;
                double sr = R.chr[0], si = R.chr[1];
                for (int g = 1; rep && g < R.n_trans; ++g) {
                    const uint64_t t = sector_translate(R, tab, g, s);
                    if (t < s) {
                        rep = false;
                        break;
                    }
                    if (t == s) {
                        const double sg = sector_parity(R, g, s) ? -1.0 : 1.0;
                        nstab++;
                        sr += sg * R.chr[2 * g];
                        si += sg * R.chr[2 * g + 1];
                    }
                }
                code[r] = rep ? (uint8_t)(nstab | ((sr * sr + si * si < 1e-20) ? 0x80 : 0)) : 0;
                mine += rep ? 1 : 0;
                sector_step(R, cur);
            }
        }
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) chunk_cnt[chunk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

// pass 2: the representatives of a chunk go to reps[chunk_pos[chunk] ...] in ascending order, their codes to info[].  Every
// lane takes every barrier of every chunk; only the walk through its own run depends on what the lane found.
template <class Dev>
__global__ __launch_bounds__(256) void k_sector_compact(const Dev *Rp, int64_t nstates, const uint8_t *code, const int64_t *chunk_pos,
                                                        int64_t nchunks, uint64_t *reps, uint8_t *info)
{
    const Dev &R = *Rp;
    __shared__ int scan[256];
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t r0 = chunk * kSectorChunk + (int64_t)threadIdx.x * kSectorRun;
        const int64_t r1 = (r0 + kSectorRun < nstates) ? r0 + kSectorRun : nstates;
        int mine = 0;
        for (int64_t r = r0; r < r1; ++r) mine += code[r] ? 1 : 0;
        __syncthreads();
        scan[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {          // inclusive Hillis-Steele scan
            const int v = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        if (mine > 0) {                                    // then r0 < nstates, and the walk ends at the lane's last one
            int64_t at = chunk_pos[chunk] + scan[threadIdx.x] - mine;
            auto cur = sector_seek(R, (uint64_t)r0);
            for (int64_t r = r0; mine > 0; ++r) {
                if (code[r]) {
                    reps[at] = sector_word(R, cur);
                    info[at] = code[r];
                    ++at;
                    --mine;
                }
                sector_step(R, cur);
            }
        }
    }
}

// row lengths of rows [r0, r1); with T.fp != nullptr the distinct values met on the way are collected for the value
// dictionary, so that the fill pass can emit 1- or 2-byte codes and the 16 B/nnz value array never exists
template <class Dev>
__global__ __launch_bounds__(128) void k_sector_count(const Dev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                      int64_t dim, int64_t r0, int64_t r1, int32_t *cnt, DictTab T)
{
    __shared__ DictCollect D;
    int32_t cols[max_row<Dev>];
    d2 vals[max_row<Dev>];
    bool collect = T.fp != nullptr;
    if (T.fp != nullptr) dict_collect_init(D);
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = r0 + (int64_t)blockIdx.x * 128 + threadIdx.x; i < r1; i += stride) {
        const int m = sector_row(*Rp, tab, reps, info, dim, i, cols, vals);
        cnt[i - r0] = m;
        for (int q = 0; collect && q < m; ++q) collect = dict_collect_insert(D, T, vals[q]);
    }
}

// ia is local to the shard (ia[0] = 0 at row r0)
template <class Dev>
__global__ __launch_bounds__(128) void k_sector_fill(const Dev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                     int64_t dim, int64_t r0, int64_t r1, const int64_t *ia, int32_t *ja, d2 *val)
{
    int32_t cols[max_row<Dev>];
    d2 vals[max_row<Dev>];
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = r0 + (int64_t)blockIdx.x * 128 + threadIdx.x; i < r1; i += stride) {
        const int m = sector_row(*Rp, tab, reps, info, dim, i, cols, vals);
        const int64_t p0 = ia[i - r0];
        for (int q = 0; q < m; ++q) {
            ja[p0 + q] = cols[q];
            val[p0 + q] = vals[q];
        }
    }
}

template <class Dev, typename CT>
__global__ __launch_bounds__(128) void k_sector_fill_coded(const Dev *Rp, const uint64_t *tab, const uint64_t *reps, const uint8_t *info,
                                                           int64_t dim, int64_t r0, int64_t r1, const int64_t *ia, int32_t *ja, CT *code,
                                                           const d2 *dict, DictTab T)
{
    __shared__ DictEncode E;
    int32_t cols[max_row<Dev>];
    d2 vals[max_row<Dev>];
    dict_encode_init(E);
    const int64_t stride = (int64_t)gridDim.x * 128;
    for (int64_t i = r0 + (int64_t)blockIdx.x * 128 + threadIdx.x; i < r1; i += stride) {
        const int m = sector_row(*Rp, tab, reps, info, dim, i, cols, vals);
        const int64_t p0 = ia[i - r0];
        for (int q = 0; q < m; ++q) {
            ja[p0 + q] = cols[q];
            code[p0 + q] = (CT)dict_encode_one(E, T, dict, vals[q]);
        }
    }
}

// number of words of the sector, refused beyond what one code byte per word can enumerate; ctab as in sector_word_count
template <class Dev>
int sector_words(const Dev &R, std::vector<uint64_t> &ctab, int64_t *nstates, const char *who)
{
    const uint64_t n = sector_word_count(R, ctab);
    if (n >= (1ULL << 40)) {
        set_error("%s: sector too large to enumerate", who);
        return QBH_EUNSUPP;
    }
    *nstates = (int64_t)n;
    return QBH_OK;
}

// a sector on the device: the family's struct, the translation tables, the representatives and their info bytes
template <class Dev>
struct SectorDev {
    Dev *R = nullptr;
    uint64_t *tab = nullptr, *reps = nullptr;
    uint8_t *info = nullptr;          // |S| | zero-norm << 7
    int64_t dim = 0;
};

// enumerates the sector described by R (its term pointers already set, or unused); everything in S joins `pool`
template <class Dev>
int sector_enumerate(const Dev &R, const std::vector<uint64_t> &tab, std::vector<void *> &pool, SectorDev<Dev> &S, const char *who)
{
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));
    std::vector<Dev> rr(1, R);
    QBH_TRY(sector_tables(rr[0], ctab, pool));
    QBH_TRY(upload(rr, &S.R, pool));
    QBH_TRY(upload(tab, &S.tab, pool));
    const int64_t nchunks = (nstates + kSectorChunk - 1) / kSectorChunk;
    const int egrid = (int)std::min<int64_t>(nchunks, 256 * 32);
    DevBufs tmp;
    uint8_t *d_code = nullptr;
    int32_t *d_cnt = nullptr;
    int64_t *d_pos = nullptr;
    QBH_HIP_WHO(who, tmp.alloc(&d_code, (size_t)nstates));
    QBH_HIP_WHO(who, tmp.alloc(&d_cnt, (size_t)nchunks * sizeof(int32_t)));
    QBH_HIP_WHO(who, tmp.alloc(&d_pos, (size_t)(nchunks + 1) * sizeof(int64_t)));
    hipLaunchKernelGGL(k_sector_flag<Dev>, dim3(egrid), dim3(256), 0, 0, S.R, S.tab, nstates, d_code, d_cnt, nchunks);
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_TRY(exclusive_scan(d_cnt, nchunks, d_pos, 0));
    QBH_HIP_WHO(who, hipMemcpy(&S.dim, d_pos + nchunks, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (S.dim <= 0 || S.dim >= 2147483647LL) {         // row and column indices are int32
        set_error("%s: sector dimension %lld out of range", who, (long long)S.dim);
        return QBH_EUNSUPP;
    }
    QBH_HIP_WHO(who, qbh::dev_alloc(&S.reps, (size_t)S.dim * sizeof(uint64_t)));
    pool.push_back(S.reps);
    QBH_HIP_WHO(who, qbh::dev_alloc(&S.info, (size_t)S.dim));
    pool.push_back(S.info);
    hipLaunchKernelGGL(k_sector_compact<Dev>, dim3(egrid), dim3(256), 0, 0, S.R, nstates, d_code, d_pos, nchunks, S.reps, S.info);
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    return QBH_OK;
}

// R zeroed, then the symmetry part of the fixed-n_dn spin sector filled in (bonds and fake_pos are the caller's)
int repr_symmetry(ReprDev &R, std::vector<uint64_t> &tab, int n_sites, int n_dn, int n_trans, const int32_t *perms,
                  const double *chars, const char *who)
{
    memset(&R, 0, sizeof(R));
    R.h.n_sites = n_sites;
    R.h.n_dn = n_dn;
    R.n_trans = n_trans;
    return sector_symmetry(n_sites, n_trans, perms, chars, who, R.h.binom, R.chr, nullptr, R.n_chunks, tab);
}

// R zeroed, then the symmetry part of the (n_up, n_dn) sector filled in (the operator's terms are the caller's)
int hubrepr_symmetry(HubReprDev &R, std::vector<uint64_t> &tab, int n_sites, int n_up, int n_dn, int n_trans, const int32_t *perms,
                     const double *chars, const char *who)
{
    memset(&R, 0, sizeof(R));
    R.n_sites = n_sites;
    R.n_up = n_up;
    R.n_dn = n_dn;
    R.n_trans = n_trans;
    return sector_symmetry(n_sites, n_trans, perms, chars, who, R.binom, R.chr, R.perm, R.n_chunks, tab);
}

// one-body terms amp * c^dag_i c_j merged on the same (i, j): (up re, up im, dn re, dn im)
using TermMap = std::map<std::pair<int, int>, std::array<double, 4>>;

// merges the terms and refuses what hubrepr_row would silently truncate: a row holds at most one move per unordered site
// pair and species, one per spin-exchange term, and the diagonal
int merge_terms(int n_sites, int n_terms, const int32_t *term_sites, const qbh_z *amp_up, const qbh_z *amp_dn, int n_exch,
                const char *who, TermMap &tmap)
{
    for (int t = 0; t < n_terms; ++t) {
        const int i = term_sites[2 * t], j = term_sites[2 * t + 1];
        if (i < 0 || i >= n_sites || j < 0 || j >= n_sites) {
            set_error("%s: term %d acts on a site outside the lattice", who, t);
            return QBH_EINVAL;
        }
        auto &a = tmap[{i, j}];
        a[0] += amp_up[t].re;
        a[1] += amp_up[t].im;
        a[2] += amp_dn[t].re;
        a[3] += amp_dn[t].im;
    }
    std::map<std::pair<int, int>, int> pairs;
    for (const auto &kv : tmap)
        if (kv.first.first != kv.first.second) pairs[{std::min(kv.first.first, kv.first.second), std::max(kv.first.first, kv.first.second)}] = 1;
    if ((int)tmap.size() > kHubReprMaxTerms || 2 * (int)pairs.size() + n_exch + 1 > kHubReprMaxRow) {
        set_error("%s: too many distinct one-body terms (%d on %d site pairs)", who, (int)tmap.size(), (int)pairs.size());
        return QBH_EUNSUPP;
    }
    return QBH_OK;
}

// R zeroed, then the symmetry part of the d-level sector of charge `total` filled in (the terms are the caller's)
int qrepr_symmetry(QuditReprDev &R, std::vector<uint64_t> &tab, int n_sites, int d, int total, int n_trans, const int32_t *perms,
                   const double *chars, const char *who)
{
    memset(&R, 0, sizeof(R));
    R.n_sites = n_sites;
    R.d = d;
    R.bits = bits_per_level(d);
    R.total = total;
    R.tw = total + 1;
    R.n_trans = n_trans;
    return sector_symmetry(n_sites, n_trans, perms, chars, who, nullptr, R.chr, nullptr, R.n_chunks, tab, R.bits);
}

// the sector matrix is only right for an operator that commutes with every translation: the pair on (g(i), g(j)) must carry
// the matrix of (i, j) (transposed when g swaps the order) and the single-site diagonals of s and g(s) must agree
int qrepr_invariant(const QuditTerms &T, int n_sites, int d, int n_trans, const int32_t *perms, const char *who)
{
    const int d2n = d * d;
    const std::vector<std::complex<double>> zero((size_t)d2n * d2n, 0.0);
    auto close = [](std::complex<double> x, std::complex<double> y) {
        return std::abs(x - y) <= QBH_SPARSE_PRECISION * std::max(1.0, std::max(std::abs(x), std::abs(y)));
    };
    for (int g = 1; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * n_sites;
        for (const auto &kv : T.pm) {
            const int gi = pg[kv.first.first], gj = pg[kv.first.second];
            const auto it = T.pm.find({std::min(gi, gj), std::max(gi, gj)});
            const std::vector<std::complex<double>> &img = it == T.pm.end() ? zero : it->second;
            for (int r = 0; r < d2n; ++r)
                for (int c = 0; c < d2n; ++c) {
                    const int rr = gi < gj ? r : (r % d) * d + r / d, cc = gi < gj ? c : (c % d) * d + c / d;
                    if (!close(kv.second[(size_t)r * d2n + c], img[(size_t)rr * d2n + cc])) {
                        set_error("%s: the terms are not invariant under translation %d: pair (%d, %d) and its image (%d, %d) differ",
                                  who, g, kv.first.first, kv.first.second, gi, gj);
                        return QBH_EINVAL;
                    }
                }
        }
        for (int s = 0; s < n_sites; ++s)
            for (int l = 0; l < d; ++l)
                if (!close(T.sdiag[(size_t)s * d + l], T.sdiag[(size_t)pg[s] * d + l])) {
                    set_error("%s: the single-site terms are not invariant under translation %d: site %d and its image %d differ", who,
                              g, s, pg[s]);
                    return QBH_EINVAL;
                }
    }
    return QBH_OK;
}

}  // namespace
}  // namespace qbh

// ------------------------------ stored sector operators: qbh_gen_heisenberg_repr, qbh_gen_hubbard_repr --
// row range of shard `shard`: the uniform partition of qbh_comm, or the caller's cuts (nnz- or cost-balanced)
static int sector_row_range(const char *who, int64_t dim, int shard, int n_shards, const int64_t *row_cuts, int64_t *r0, int64_t *r1)
{
    if (row_cuts) {
        bool ok = row_cuts[0] == 0 && row_cuts[n_shards] == dim;
        for (int q = 0; q < n_shards && ok; ++q) ok = row_cuts[q + 1] >= row_cuts[q];
        if (!ok) {
            qbh::set_error("%s: row_cuts must rise from 0 to the sector dimension %lld", who, (long long)dim);
            return QBH_EINVAL;
        }
        *r0 = row_cuts[shard];
        *r1 = row_cuts[shard + 1];
    } else {
        const int64_t nblk = (dim + n_shards - 1) / n_shards;
        *r0 = std::min<int64_t>((int64_t)shard * nblk, dim);
        *r1 = std::min<int64_t>(*r0 + nblk, dim);
    }
    return QBH_OK;
}

// this shard's rows of a sector operator: lengths (+ the distinct values) -> row pointers -> coded or uncoded fill, adopted
// into *out.  `pool` holds the caller's tables and representatives; it is released before the handle takes the arrays.
template <class Dev>
static int assemble_sector_rows(const char *who, std::vector<void *> &pool, const Dev *d_R, const uint64_t *d_tab,
                                const uint64_t *d_reps, const uint8_t *d_info, int64_t dim, int shard, int n_shards,
                                const int64_t *row_cuts, const qbh_opts *opts, qbh_csr **out, int64_t *dim_out)
{
    using namespace qbh;
    if (dim >= 2147483647LL) {            // column indices are int32
        set_error("%s: sector dimension %lld out of range", who, (long long)dim);
        return QBH_EUNSUPP;
    }
    int64_t r0 = 0, r1 = 0;
    QBH_TRY(sector_row_range(who, dim, shard, n_shards, row_cuts, &r0, &r1));
    const int64_t nloc = r1 - r0;
    if (nloc <= 0) {
        set_error("%s: shard %d of %d is empty (dim %lld)", who, shard, n_shards, (long long)dim);
        return QBH_EINVAL;
    }
    DictBuild db;
    std::unique_ptr<DictBuild, void (*)(DictBuild *)> db_end(&db, dict_build_end);
    const bool want_dict = !opts || opts->value_dict;
    if (want_dict) {
        const bool rows_kernel = !opts || opts->spmv_kernel == QBH_KERNEL_AUTO || opts->spmv_kernel == QBH_KERNEL_ROWS;
        QBH_TRY(dict_build_begin(&db, (opts && opts->value_dict == 2) || !rows_kernel ? 256 : kDictMax, 0));
    }
    DevBufs csr;                          // the operator's arrays until the handle adopts them
    int64_t *d_ia = nullptr;
    int32_t *d_ja = nullptr;
    uint8_t *d_code = nullptr;
    d2 *d_val = nullptr, *d_dict = nullptr;
    const int rgrid = (int)std::min<int64_t>((nloc + 127) / 128, 256 * 16);
    int64_t nnz = 0;
    {
        DevBufs tmp;
        int32_t *d_cnt = nullptr;
        QBH_HIP_WHO(who, tmp.alloc(&d_cnt, (size_t)nloc * sizeof(int32_t)));
        QBH_HIP_WHO(who, csr.alloc(&d_ia, (size_t)(nloc + 1) * sizeof(int64_t)));
        hipLaunchKernelGGL(k_sector_count<Dev>, dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1, d_cnt, db.tab);
        QBH_HIP_WHO(who, hipGetLastError());
        QBH_TRY(exclusive_scan(d_cnt, nloc, d_ia, 0));
        QBH_HIP_WHO(who, hipMemcpy(&nnz, d_ia + nloc, sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    QBH_HIP_WHO(who, csr.alloc(&d_ja, (size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
    int n_dict = 0;
    if (want_dict) {
        QBH_TRY(dict_build_finalize(&db, &d_dict, &n_dict, 0));
        if (d_dict) csr.pool.push_back(d_dict);
    }
    if (n_dict > 0) {
        // few distinct values (amplitudes x signs x phases x square roots of stabiliser ratios): 1- or 2-byte codes are
        // emitted directly (5 or 6 B/nnz instead of 20)
        const int w = dict_code_width(n_dict);
        QBH_HIP_WHO(who, csr.alloc(&d_code, (size_t)nnz * w + 16));
        QBH_HIP_WHO(who, hipMemset(d_code + (size_t)nnz * w, 0, 16));
        if (w == 1)
            hipLaunchKernelGGL((k_sector_fill_coded<Dev, uint8_t>), dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1,
                               d_ia, d_ja, d_code, d_dict, db.tab);
        else
            hipLaunchKernelGGL((k_sector_fill_coded<Dev, uint16_t>), dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1,
                               d_ia, d_ja, reinterpret_cast<uint16_t *>(d_code), d_dict, db.tab);
        QBH_HIP_WHO(who, hipGetLastError());
        int bad = 0;
        QBH_TRY(dict_build_mismatch(&db, &bad, 0));
        if (bad) {
            set_error("%s: value dictionary mismatch between the count and fill passes", who);
            return QBH_EHIP;
        }
    } else {
        const hipError_t e = csr.alloc(&d_val, (size_t)std::max<int64_t>(nnz, 1) * sizeof(d2));
        if (e == hipErrorOutOfMemory) {
            set_error("%s: %lld nonzeros with more than 65536 distinct values do not fit this GPU uncoded (%.1f GB); shard the "
                      "sector over more GPUs", who, (long long)nnz, 20e-9 * (double)nnz);
            (void)hipGetLastError();
            return QBH_ENOMEM;
        }
        QBH_HIP_WHO(who, e);
        hipLaunchKernelGGL(k_sector_fill<Dev>, dim3(rgrid), dim3(128), 0, 0, d_R, d_tab, d_reps, d_info, dim, r0, r1, d_ia, d_ja, d_val);
        QBH_HIP_WHO(who, hipGetLastError());
    }
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    free_pool(pool);
    db_end.reset();
    csr.release();                        // ownership passes with the call: on failure the arrays have already been released
    if (dim_out) *dim_out = dim;
    if (d_code) return adopt_coded_csr(out, nloc, dim, r0, nnz, d_ia, d_ja, d_code, d_dict, n_dict, opts);
    qbh_opts og;
    opts_generated(opts, &og);
    return qbh_csr_create_device(out, nloc, dim, r0, nnz, d_ia, d_ja, reinterpret_cast<qbh_z *>(d_val), 1, &og);
}

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

// ---- operators between sectors.  perms / chars as in the generators; the vectors are indexed like the rows of the sector
// operators (all representatives, ascending) ----
// S^z_q (see k_repr_apply_sz), with the characters of the TARGET momentum
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
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    std::vector<ReprDev> rr(1);
    std::vector<uint64_t> tab;
    QBH_TRY(repr_symmetry(rr[0], tab, n_sites, n_dn, n_trans, perms, chars_new, who));
    SpinCoefR cf{};
    for (int sidx = 0; sidx < n_sites; ++sidx) {
        cf.re[sidx] = coef[sidx].re;
        cf.im[sidx] = coef[sidx].im;
    }
    DevBufs bufs;
    SectorDev<ReprDev> S;
    QBH_TRY(sector_enumerate(rr[0], tab, bufs.pool, S, who));
    hipLaunchKernelGGL(k_repr_apply_sz, dim3(blas_grid(S.dim)), dim3(256), 0, 0, n_sites, S.reps, S.info, S.dim, cf,
                       reinterpret_cast<const d2 *>(d_vec_old), reinterpret_cast<d2 *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    if (dim_out) *dim_out = S.dim;
    return QBH_OK;
}

// S^-_q (kind -1: n_dn -> n_dn + 1) and S^+_q (kind +1: n_dn -> n_dn - 1) between momentum sectors; see k_repr_apply_flip.
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
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    SpinCoefR cf{};
    for (int sidx = 0; sidx < n_sites; ++sidx) {
        cf.re[sidx] = coef[sidx].re;
        cf.im[sidx] = coef[sidx].im;
    }
    std::vector<ReprDev> ro(1), rn(1);
    std::vector<uint64_t> tab_o, tab_n;
    QBH_TRY(repr_symmetry(ro[0], tab_o, n_sites, n_dn_old, n_trans, perms, chars_old, who));
    QBH_TRY(repr_symmetry(rn[0], tab_n, n_sites, n_new, n_trans, perms, chars_new, who));
    DevBufs bufs;
    SectorDev<ReprDev> So, Sn;
    QBH_TRY(sector_enumerate(ro[0], tab_o, bufs.pool, So, who));
    QBH_TRY(sector_enumerate(rn[0], tab_n, bufs.pool, Sn, who));
    QBH_HIP_WHO(who, hipMemset(d_vec_new, 0, (size_t)Sn.dim * sizeof(d2)));
    hipLaunchKernelGGL(k_repr_apply_flip, dim3(blas_grid(So.dim)), dim3(128), 0, 0, Sn.R, Sn.tab, So.reps, So.info, So.dim, Sn.reps,
                       Sn.info, Sn.dim, kind < 0 ? 1 : 0, cf, reinterpret_cast<const d2 *>(d_vec_old),
                       reinterpret_cast<double *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    if (dim_old_out) *dim_old_out = So.dim;
    if (dim_new_out) *dim_new_out = Sn.dim;
    return QBH_OK;
}

// see k_qrepr_mopr; the target characters chi_old * eta follow from coef
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
    QuditMopr cf{};
    for (int lp = 0; lp < d; ++lp)
        for (int l = 0; l < d; ++l) {
            const qbh_z z = local[lp * d + l];
            if (z.re == 0.0 && z.im == 0.0) continue;
            if (lp != l + dq) {
                set_error("%s: local[%d][%d] is nonzero but does not change the level by dq = %d", who, lp, l, dq);
                return QBH_EINVAL;
            }
            cf.la[lp] = z.re;
            cf.lb[lp] = z.im;
        }
    for (int s = 0; s < n_sites; ++s) {
        cf.ca[s] = coef[s].re;
        cf.cb[s] = coef[s].im;
    }
    QuditReprDev Ro, Rn;
    std::vector<uint64_t> tab, tab_n;
    QBH_TRY(qrepr_symmetry(Ro, tab, n_sites, d, total_old, n_trans, perms, chars_old, who));
    // eta(g) = c_{g(s)} / c_s from the largest coefficient, then c_{g(s)} = eta(g) c_s checked on every site
    std::vector<std::complex<double>> c(n_sites);
    int s0 = 0;
    for (int s = 0; s < n_sites; ++s) {
        c[s] = std::complex<double>(coef[s].re, coef[s].im);
        if (std::abs(c[s]) > std::abs(c[s0])) s0 = s;
    }
    const double cmax = std::abs(c[s0]);
    std::vector<double> chars_new((size_t)2 * n_trans);
    for (int g = 0; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * n_sites;
        const std::complex<double> eta = cmax > 0.0 ? c[pg[s0]] / c[s0] : 1.0;
        for (int s = 0; s < n_sites; ++s)
            if (std::abs(c[pg[s]] - eta * c[s]) > 1e-12 * cmax) {
                set_error("%s: coef does not transform with a character under translation %d (site %d)", who, g, s);
                return QBH_EINVAL;
            }
        const std::complex<double> chi = std::complex<double>(chars_old[2 * g], chars_old[2 * g + 1]) * eta;
        chars_new[2 * g] = chi.real();
        chars_new[2 * g + 1] = chi.imag();
    }
    QBH_TRY(qrepr_symmetry(Rn, tab_n, n_sites, d, total_new, n_trans, perms, chars_new.data(), who));
    int64_t nst = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(Ro, ctab, &nst, who));          // every refusal comes before the device is looked for
    QBH_TRY(sector_words(Rn, ctab, &nst, who));
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    DevBufs bufs;
    SectorDev<QuditReprDev> So, Sn;
    QBH_TRY(sector_enumerate(Ro, tab, bufs.pool, So, who));
    QBH_TRY(sector_enumerate(Rn, tab_n, bufs.pool, Sn, who));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_qrepr_mopr, dim3(blas_grid(Sn.dim)), dim3(256), 0, st, So.R, So.tab, So.reps, So.info, So.dim, Sn.reps, Sn.info,
                       Sn.dim, dq, cf, reinterpret_cast<const d2 *>(d_vec_old), reinterpret_cast<d2 *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipStreamSynchronize(st));
    if (dim_old_out) *dim_old_out = So.dim;
    if (dim_new_out) *dim_new_out = Sn.dim;
    return QBH_OK;
}

// ------------------------------ Kondo lattice: qbh_gen_kondo_repr(_cuts), qbh_mopr_diag_kondo_repr_dev --
// the symmetry part of the sector on top of R.k (shape and terms already in place)
static int kondo_symmetry(qbh::KondoReprDev &R, std::vector<uint64_t> &tab, int n_trans, const int32_t *perms, const double *chars,
                          const char *who)
{
    using namespace qbh;
    if (!perms || !chars || n_trans < 1) {
        set_error("%s: invalid symmetry argument", who);
        return QBH_EINVAL;
    }
    if (n_trans > kReprMaxTrans) {
        set_error("%s: %d translations; at most %d are supported", who, n_trans, kReprMaxTrans);
        return QBH_EUNSUPP;
    }
    R.n_trans = n_trans;
    return sector_symmetry(R.k.n_sites, n_trans, perms, chars, who, nullptr, R.chr, R.perm, R.n_chunks, tab);
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

// N_q and the two S^z_q of a Kondo lattice between momentum sectors (see k_kondo_apply_diag), with the characters of the TARGET
// momentum
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
    // the three coefficient sets must transform with one character: c_{g(s)} = eta(g) c_s
    const qbh_z *sets[3] = {coef_up, coef_dn, coef_spin};
    for (int g = 0; g < n_trans; ++g) {
        const int32_t *pg = perms + (size_t)g * n_sites;
        std::complex<double> eta = 1.0;
        double best = 0.0;
        for (int q = 0; q < 3; ++q)
            for (int s = 0; s < n_sites; ++s) {
                const std::complex<double> c(sets[q][s].re, sets[q][s].im);
                if (std::abs(c) > best) {                  // eta(g) from the largest coefficient
                    best = std::abs(c);
                    eta = std::complex<double>(sets[q][pg[s]].re, sets[q][pg[s]].im) / c;
                }
            }
        for (int q = 0; q < 3; ++q)
            for (int s = 0; s < n_sites; ++s) {
                const std::complex<double> c(sets[q][s].re, sets[q][s].im), ci(sets[q][pg[s]].re, sets[q][pg[s]].im);
                if (std::abs(ci - eta * c) > 1e-10 * std::max(1.0, best)) {
                    set_error("%s: the coefficients do not transform with a character under translation %d", who, g);
                    return QBH_EINVAL;
                }
            }
    }
    int64_t nstates = 0;
    std::vector<uint64_t> ctab;
    QBH_TRY(sector_words(R, ctab, &nstates, who));       // every refusal comes before the device is looked for
    if (qbh_device_count() <= 0) {
        set_error("no HIP device visible");
        return QBH_ENODEVICE;
    }
    KondoCoef cf{};
    for (int s = 0; s < n_sites; ++s) {
        cf.up_re[s] = coef_up[s].re;
        cf.up_im[s] = coef_up[s].im;
        cf.dn_re[s] = coef_dn[s].re;
        cf.dn_im[s] = coef_dn[s].im;
        cf.sp_re[s] = coef_spin[s].re;
        cf.sp_im[s] = coef_spin[s].im;
    }
    DevBufs bufs;
    SectorDev<KondoReprDev> S;
    QBH_TRY(sector_enumerate(R, tab, bufs.pool, S, who));
    hipLaunchKernelGGL(k_kondo_apply_diag, dim3(blas_grid(S.dim)), dim3(256), 0, 0, n_sites, S.reps, S.info, S.dim, cf,
                       reinterpret_cast<const d2 *>(d_vec_old), reinterpret_cast<d2 *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    if (dim_out) *dim_out = S.dim;
    return QBH_OK;
}

// N_q / S^z_q between Hubbard momentum sectors (see k_hubrepr_apply_diag), with the characters of the TARGET momentum
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
    // the coefficients must transform with a one-dimensional representation: c_{g(s)} = eta(g) c_s for both species
    for (int g = 0; g < n_trans; ++g) {
        bool have = false;
        double er = 0.0, ei = 0.0;
        for (int pass = 0; pass < 2; ++pass)
            for (int sp = 0; sp < 2; ++sp)
                for (int s = 0; s < n_sites; ++s) {
                    const qbh_z *c = sp ? coef_dn : coef_up;
                    const int img = perms[(size_t)g * n_sites + s];
                    if (img < 0 || img >= n_sites) continue;          // reported by hubrepr_symmetry below
                    const double a2 = c[s].re * c[s].re + c[s].im * c[s].im;
                    if (pass == 0) {
                        if (!have && a2 > 1e-24) {                    // eta(g) = c_{g(s)} / c_s
                            er = (c[img].re * c[s].re + c[img].im * c[s].im) / a2;
                            ei = (c[img].im * c[s].re - c[img].re * c[s].im) / a2;
                            have = true;
                        }
                    } else {
                        const double wr = (have ? er : 1.0) * c[s].re - (have ? ei : 0.0) * c[s].im;
                        const double wi = (have ? er : 1.0) * c[s].im + (have ? ei : 0.0) * c[s].re;
                        if (std::fabs(wr - c[img].re) > 1e-10 || std::fabs(wi - c[img].im) > 1e-10) {
                            set_error("qbh_mopr_diag_hubrepr_dev: the coefficients do not transform with a character under translation %d", g);
                            return QBH_EINVAL;
                        }
                    }
                }
    }
    std::vector<HubReprDev> rr(1);
    std::vector<uint64_t> tab;
    QBH_TRY(hubrepr_symmetry(rr[0], tab, n_sites, n_up, n_dn, n_trans, perms, chars_new, who));
    HubCoef cf{};
    for (int s = 0; s < n_sites; ++s) {
        cf.up_re[s] = coef_up[s].re;
        cf.up_im[s] = coef_up[s].im;
        cf.dn_re[s] = coef_dn[s].re;
        cf.dn_im[s] = coef_dn[s].im;
    }
    DevBufs bufs;
    SectorDev<HubReprDev> S;
    QBH_TRY(sector_enumerate(rr[0], tab, bufs.pool, S, who));
    hipLaunchKernelGGL(k_hubrepr_apply_diag, dim3(blas_grid(S.dim)), dim3(256), 0, 0, n_sites, S.reps, S.info, S.dim, cf,
                       reinterpret_cast<const d2 *>(d_vec_old), reinterpret_cast<d2 *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    if (dim_out) *dim_out = S.dim;
    return QBH_OK;
}

// c_{q,sigma} (kind -1) / c^dag_{q,sigma} (kind +1) between Hubbard momentum sectors; see k_hubrepr_apply_c
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
    std::vector<HubReprDev> ro(1), rn(1);
    std::vector<uint64_t> tab_o, tab_n;
    QBH_TRY(hubrepr_symmetry(ro[0], tab_o, n_sites, n_up_old, n_dn_old, n_trans, perms, chars_old, who));
    QBH_TRY(hubrepr_symmetry(rn[0], tab_n, n_sites, n_up_new, n_dn_new, n_trans, perms, chars_new, who));
    HubCoef cf{};
    for (int s = 0; s < n_sites; ++s) {
        cf.up_re[s] = cf.dn_re[s] = coef[s].re;
        cf.up_im[s] = cf.dn_im[s] = coef[s].im;
    }
    DevBufs bufs;
    SectorDev<HubReprDev> So, Sn;
    QBH_TRY(sector_enumerate(ro[0], tab_o, bufs.pool, So, who));
    QBH_TRY(sector_enumerate(rn[0], tab_n, bufs.pool, Sn, who));
    QBH_HIP_WHO(who, hipMemset(d_vec_new, 0, (size_t)Sn.dim * sizeof(d2)));
    hipLaunchKernelGGL(k_hubrepr_apply_c, dim3(blas_grid(So.dim)), dim3(128), 0, 0, Sn.R, Sn.tab, So.reps, So.info, So.dim, Sn.reps,
                       Sn.info, Sn.dim, species, kind > 0 ? 1 : 0, cf, reinterpret_cast<const d2 *>(d_vec_old),
                       reinterpret_cast<double *>(d_vec_new));
    QBH_HIP_WHO(who, hipGetLastError());
    QBH_HIP_WHO(who, hipDeviceSynchronize());
    if (dim_old_out) *dim_old_out = So.dim;
    if (dim_new_out) *dim_new_out = Sn.dim;
    return QBH_OK;
}

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
// ORD: the ordered walk of the wave kernels (qbh_kernels.hip, DynWalk) at workgroup granularity -- every XCD owns one contiguous
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
                if (REALX) sum.x = dr * a.xr[row];
                else       sum = dr * a.xg[row];
                for (int k0 = 0; k0 < T.w_up; k0 += kSecUnroll) {          // up hops: inside the block
                    uint32_t e[kSecUnroll];
#pragma unroll
                    for (int q = 0; q < kSecUnroll; ++q) e[q] = k0 + q < T.w_up ? T.upell[(size_t)(k0 + q) * cu + r] : 0xFFFFFFFFu;
                    if (REALX) {
                        double xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = e[q] != 0xFFFFFFFFu ? a.xr[B.row0 + (e[q] & 0xFFFFFFu)] : 0.0;
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (e[q] != 0xFFFFFFFFu) sum.x += T.updict[e[q] >> 24] * xv[q];
                    } else {
                        d2 xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = e[q] != 0xFFFFFFFFu ? a.xg[B.row0 + (e[q] & 0xFFFFFFu)] : d2{0.0, 0.0};
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
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = h0 + q < B.nhop ? a.xr[sh[h0 + q].off + (pr[q] & 0x7FFFFFFFu)] : 0.0;
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (h0 + q < B.nhop) sum.x += ((pr[q] >> 31) ? -sh[h0 + q].cr : sh[h0 + q].cr) * xv[q];
                    } else {
                        d2 xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            xv[q] = h0 + q < B.nhop ? a.xg[sh[h0 + q].off + (pr[q] & 0x7FFFFFFFu)] : d2{0.0, 0.0};
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
            if (a.beta != 0.0) yo = a.y_re ? d2{a.y_re[row], 0.0} : a.y[row];
            if (a.gamma != 0.0) xi = a.y_re ? d2{a.xl_re[row], 0.0} : a.xl[row];
            const d2 yn = a.alpha * sum + a.beta * yo + a.gamma * xi;
            if (a.y_re) a.y_re[row] = yn.x;
            else        a.y[row] = yn;
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
        const double *xrb = REALX ? a.xr + B.row0 : nullptr;              // the block's own x
        const d2 *xgb = REALX ? nullptr : a.xg + B.row0;
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
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = h0 + q < B.nhop ? sec_at(a.xr + off[q], ix[q]) : 0.0;
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q)
                            if (h0 + q < B.nhop) sum.x += (((tp >> gg[q]) & 1ULL) ? -sh[h0 + q].cr : sh[h0 + q].cr) * xv[q];
                    } else {
                        d2 xv[kSecUnroll];
#pragma unroll
                        for (int q = 0; q < kSecUnroll; ++q) xv[q] = h0 + q < B.nhop ? sec_at(a.xg + off[q], ix[q]) : d2{0.0, 0.0};
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
            if (a.beta != 0.0) yo = a.y_re ? d2{sec_at(a.y_re + B.row0 + tb, ln), 0.0} : sec_at(a.y + B.row0 + tb, ln);
            if (a.gamma != 0.0) xi = a.y_re ? d2{sec_at(a.xl_re + B.row0 + tb, ln), 0.0} : sec_at(a.xl + B.row0 + tb, ln);
            const d2 yn = a.alpha * sum + a.beta * yo + a.gamma * xi;
            if (a.y_re) a.y_re[row] = yn.x;
            else        a.y[row] = yn;
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
                sum.x += v.x * a.xr[a.rja[q]];
            } else {
                const d2 xv = a.xg[a.rja[q]];
                sum += d2{v.x * xv.x - v.y * xv.y, v.x * xv.y + v.y * xv.x};
            }
        }
        for (int off = TPR / 2; off > 0; off >>= 1) {
            sum.x += __shfl_xor(sum.x, off, 64);
            if (!REALX) sum.y += __shfl_xor(sum.y, off, 64);
        }
        if (sub == 0) {
            const int64_t row = a.rrow[p];
            if (a.y_re) a.y_re[row] += a.alpha * sum.x;
            else        a.y[row] += a.alpha * sum;
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
        const d2 xi = a.y_re ? d2{a.xl_re[i], 0.0} : a.xl[i];
        const d2 yn = a.y_re ? d2{a.y_re[i], 0.0} : a.y[i];
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
        for (int c = 0; c < 3; ++c) a.partials[(size_t)blockIdx.x * 3 + c] = (red[c * 4] + red[c * 4 + 1]) + (red[c * 4 + 2] + red[c * 4 + 3]);
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
        if (a.xr != nullptr) {
            if (un == 4) sector_orbit_launch_t<true, 4>(a, s);
            else         sector_orbit_launch_t<true, 8>(a, s);
        } else {
            if (un == 4) sector_orbit_launch_t<false, 4>(a, s);
            else         sector_orbit_launch_t<false, 8>(a, s);
        }
    } else if (a.xr != nullptr) {
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
        if (a.xr != nullptr) hipLaunchKernelGGL(k_sec_remainder<true>, dim3(rg), dim3(256), 0, s, a);
        else                 hipLaunchKernelGGL(k_sec_remainder<false>, dim3(rg), dim3(256), 0, s, a);
        QBH_HIP(hipGetLastError());
    }
    const int parts = blas_grid(a.dim);
    if (a.partials != nullptr) {
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
