// qbh_gen_util.hpp -- what the generators share on the host and the device: uploads and pooled device buffers, bond
// merging, the colexicographic rank / unrank of the fixed-n_dn spin basis, hop tables in ELL form.  Internal linkage: every
// translation unit that includes this gets its own copy.
#pragma once
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

namespace qbh {
struct HopTableView {
    int64_t n;
    const int32_t *ptr, *tgt;
    const double *val;
};
namespace {

inline void enumerate_configs(int L, int n, std::vector<uint32_t> &cfg)
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

template <typename T>
int upload(const std::vector<T> &h, T **d, std::vector<void *> &pool)
{
    const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    QBH_HIP(qbh::dev_alloc((void **)d, bytes));
    pool.push_back(*d);
    if (!h.empty()) QBH_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return QBH_OK;
}

inline void free_pool(std::vector<void *> &pool)
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

inline int merge_bonds(int n_sites, int n_bonds, const int32_t *bonds, std::map<std::pair<int, int>, double> &out)
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

inline uint64_t binom_u64(int n, int k)
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

namespace {
// hop table -> ELL (entry k of configuration c at [k*N + c]), padded to groups of 8 with (c, amplitude 0); targets as
// uint32, amplitudes as codes into amp[] (shared by both species)
inline int upload_ell(const qbh::HopTableView &H, std::vector<double> &amp, int *width, uint32_t **d_tgt, uint8_t **d_val)
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
