// qbh_csrprep.hip -- one-time preparation of a CSR operator: row blocks, longest row, value dictionary (host side of
// qbh_dict.hpp), column split of a row shard, exclusive scan.
#include <algorithm>
#include <cstring>
#include <vector>

#include "qbh_internal.hpp"
#include "qbh_dict.hpp"

namespace qbh {

// ------------------------------------------------------ row-block builder ------
// Row block w = the rows whose first nonzero falls in the nnz window
// [w*window, (w+1)*window): rb[w] = lower_bound(ia, w*window).  Embarrassingly parallel
// and nnz-balanced; block nnz < window + (longest row).
__global__ void k_build_rowblocks(const int64_t *ia, int64_t nrows, int64_t window, int32_t *rb,
                                  int64_t *bp, int64_t n_blocks)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > n_blocks) return;
    if (w == n_blocks) {
        rb[w] = (int32_t)nrows;
        bp[w] = ia[nrows];
        return;
    }
    const int64_t target = w * window;
    int64_t lo = 0, hi = nrows;          // first r in [0, nrows] with ia[r] >= target
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ia[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    rb[w] = (int32_t)lo;
    bp[w] = ia[lo];
}

int launch_build_rowblocks(const int64_t *d_ia, int64_t nrows, int64_t window, int32_t *d_rb,
                           int64_t *d_bp, int64_t n_blocks, hipStream_t s)
{
    const int64_t n = n_blocks + 1;
    return launch_kernel(k_build_rowblocks, (unsigned)((n + 255) / 256), 256, s, d_ia, nrows, window, d_rb, d_bp, n_blocks);
}

__global__ void k_max_rowlen(const int64_t *ia, int64_t nrows, unsigned long long *out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long mx = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += stride) {
        const unsigned long long len = (unsigned long long)(ia[r + 1] - ia[r]);
        mx = len > mx ? len : mx;
    }
    if (mx) atomicMax(out, mx);
}

int launch_max_rowlen(const int64_t *d_ia, int64_t nrows, int64_t *d_out, hipStream_t s)
{
    QBH_HIP(hipMemsetAsync(d_out, 0, sizeof(int64_t), s));
    return launch_kernel(k_max_rowlen, blas_grid(nrows), kBlock, s, d_ia, nrows, (unsigned long long *)d_out);
}

// ------------------------------------------------- value dictionary ------------
// Lossless coding of the value stream: when a matrix holds at most 256 distinct complex128
// values (every full-basis Hamiltonian of the reference's model families does: hopping
// amplitudes, exchange constants and a handful of diagonal sums), each value is replaced by
// a 1-byte index into a dictionary that lives in LDS during SpMV; up to 65536 distinct values
// (momentum sectors) by a 2-byte index.  The stream shrinks from 20 to 5 or 6 bytes per
// nonzero; products are computed from the exact original doubles.
// (device helpers: qbh_dict.hpp)
__global__ __launch_bounds__(kBlock) void k_dict_collect(const d2 *val, int64_t nnz, DictTab T)
{
    __shared__ DictCollect D;
    dict_collect_init(D);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += stride)
        if (!dict_collect_insert(D, T, val[i])) break;
}

template <typename CT>
__global__ __launch_bounds__(kBlock) void k_dict_encode(const d2 *val, int64_t nnz, DictTab T, const d2 *dict, CT *code)
{
    __shared__ DictEncode E;
    dict_encode_init(E);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += stride)
        code[i] = (CT)dict_encode_one(E, T, dict, val[i]);
}

int dict_build_begin(DictBuild *b, int cap, hipStream_t s)
{
    DictTab &T = b->tab;
    T.cap = cap < kDictMax ? cap : kDictMax;
    QBH_HIP(qbh::dev_alloc(&T.fp, (size_t)kDictSlots * sizeof(unsigned long long)));
    QBH_HIP(qbh::dev_alloc(&T.val, (size_t)kDictSlots * sizeof(d2)));
    QBH_HIP(qbh::dev_alloc(&T.code, (size_t)kDictSlots * sizeof(uint32_t)));
    QBH_HIP(qbh::dev_alloc(&T.flags, 4 * sizeof(int)));
    QBH_HIP(hipMemsetAsync(T.fp, 0, (size_t)kDictSlots * sizeof(unsigned long long), s));
    QBH_HIP(hipMemsetAsync(T.flags, 0, 4 * sizeof(int), s));
    return QBH_OK;
}

int dict_build_finalize(DictBuild *b, d2 **d_dict_out, int *n_out, hipStream_t s)
{
    DictTab &T = b->tab;
    *n_out = 0;
    *d_dict_out = nullptr;
    int h[4] = {0, 0, 0, 0};
    QBH_HIP(hipMemcpyAsync(h, T.flags, sizeof(h), hipMemcpyDeviceToHost, s));
    QBH_HIP(hipStreamSynchronize(s));
    if (debug_sw().trace_dict) fprintf(stderr, "dict: overflow %d claimed %d cap %d\n", h[0], h[1], T.cap);
    if (h[0] || h[1] <= 0 || h[1] > T.cap) return QBH_OK;
    std::vector<unsigned long long> fp((size_t)kDictSlots);
    std::vector<d2> val((size_t)kDictSlots);
    QBH_HIP(hipMemcpy(fp.data(), T.fp, fp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    QBH_HIP(hipMemcpy(val.data(), T.val, val.size() * sizeof(d2), hipMemcpyDeviceToHost));
    struct Ent {
        unsigned long long a, b;
        int slot;
    };
    std::vector<Ent> ents;
    ents.reserve((size_t)h[1]);
    for (int sl = 0; sl < kDictSlots; ++sl)
        if (fp[(size_t)sl] != 0ULL) {
            Ent e;
            const double vx = val[(size_t)sl].x, vy = val[(size_t)sl].y;
            memcpy(&e.a, &vx, 8);
            memcpy(&e.b, &vy, 8);
            e.slot = sl;
            ents.push_back(e);
        }
    // order by bit pattern: the codes do not depend on which workgroup won an atomic
    std::sort(ents.begin(), ents.end(), [](const Ent &x, const Ent &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    // two different values with one fingerprint would share a slot: the count would not add up
    const int n = (int)ents.size();
    if (debug_sw().trace_dict) fprintf(stderr, "dict: %d entries\n", n);
    if (n != h[1] || n > T.cap) return QBH_OK;
    const size_t n_alloc = (size_t)std::max(n, kDictLds);
    std::vector<d2> dict(n_alloc, d2{0.0, 0.0});
    std::vector<uint32_t> code((size_t)kDictSlots, 0u);
    for (int c = 0; c < n; ++c) {
        dict[(size_t)c] = val[(size_t)ents[(size_t)c].slot];
        code[(size_t)ents[(size_t)c].slot] = (uint32_t)c;
    }
    d2 *d_dict = nullptr;
    QBH_HIP(qbh::dev_alloc(&d_dict, n_alloc * sizeof(d2)));
    hipError_t e1 = hipMemcpy(d_dict, dict.data(), n_alloc * sizeof(d2), hipMemcpyHostToDevice);
    hipError_t e2 = hipMemcpy(T.code, code.data(), code.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e1 != hipSuccess || e2 != hipSuccess) {
        (void)hipFree(d_dict);
        set_error("value dictionary upload failed");
        return QBH_EHIP;
    }
    *d_dict_out = d_dict;
    *n_out = n;
    return QBH_OK;
}

int dict_build_mismatch(DictBuild *b, int *bad, hipStream_t s)
{
    int h[4] = {0, 0, 0, 0};
    QBH_HIP(hipMemcpyAsync(h, b->tab.flags, sizeof(h), hipMemcpyDeviceToHost, s));
    QBH_HIP(hipStreamSynchronize(s));
    *bad = h[3];
    return QBH_OK;
}

void dict_build_end(DictBuild *b)
{
    DictTab &T = b->tab;
    if (T.fp) (void)hipFree(T.fp);
    if (T.val) (void)hipFree(T.val);
    if (T.code) (void)hipFree(T.code);
    if (T.flags) (void)hipFree(T.flags);
    T = DictTab{nullptr, nullptr, nullptr, nullptr, 0};
}

// Codes the value stream when it holds at most `cap` distinct values: *d_code_out (nnz * width + 16 bytes),
// *d_dict_out and *n_out > 0 on success; n = 0 (nothing allocated) when there are too many distinct values.
int build_value_dict(const d2 *d_val, int64_t nnz, int cap, uint8_t **d_code_out, d2 **d_dict_out, int *n_out, hipStream_t s)
{
    *n_out = 0;
    *d_code_out = nullptr;
    *d_dict_out = nullptr;
    DictBuild b;
    int rc = dict_build_begin(&b, cap, s);
    uint8_t *code = nullptr;
    d2 *dict = nullptr;
    if (rc == QBH_OK) {
        const int grid = blas_grid(nnz);
        hipLaunchKernelGGL(k_dict_collect, dim3(grid), dim3(kBlock), 0, s, d_val, nnz, b.tab);
        int n = 0;
        rc = dict_build_finalize(&b, &dict, &n, s);
        if (rc == QBH_OK && n > 0) {
            const int w = dict_code_width(n);
            if (qbh::dev_alloc(&code, (size_t)nnz * w + 16) != hipSuccess) {
                (void)hipGetLastError();
                n = 0;                                   // no room for the codes: stay uncoded
            } else {
                (void)hipMemsetAsync(code + (size_t)nnz * w, 0, 16, s);
                if (w == 1) hipLaunchKernelGGL(k_dict_encode<uint8_t>, dim3(grid), dim3(kBlock), 0, s, d_val, nnz, b.tab, dict, code);
                else hipLaunchKernelGGL(k_dict_encode<uint16_t>, dim3(grid), dim3(kBlock), 0, s, d_val, nnz, b.tab, dict,
                                        reinterpret_cast<uint16_t *>(code));
                int bad = 0;
                rc = dict_build_mismatch(&b, &bad, s);
                if (rc != QBH_OK || bad) n = 0;
            }
        }
        if (n > 0) {
            *n_out = n;
            *d_code_out = code;
            *d_dict_out = dict;
        } else {
            if (code) (void)hipFree(code);
            if (dict) (void)hipFree(dict);
        }
    }
    dict_build_end(&b);
    return rc;
}

// ------------------------------------------------------- shard column split -----
// A row shard is split once, at creation, into the entries whose column lies inside the shard's own
// row range [lo, hi) and the rest.  The first part needs only the locally owned block of x, so it can
// run while the all-gather of x is still in flight; the second part runs after it and accumulates.
__global__ __launch_bounds__(kBlock) void k_split_count(const int64_t *ia, const int32_t *ja, int64_t nrows, int32_t lo,
                                                        int32_t hi, int32_t *cnt0)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < nrows; r += stride) {
        int c = 0;
        for (int64_t p = ia[r]; p < ia[r + 1]; ++p) {
            const int32_t col = ja[p];
            c += (col >= lo && col < hi) ? 1 : 0;
        }
        cnt0[r] = c;
    }
}

__global__ __launch_bounds__(kBlock) void k_split_fill(const int64_t *ia, const int32_t *ja, const d2 *val, const uint8_t *code,
                                                       int64_t nrows, int32_t lo, int32_t hi, const int64_t *ia0, int32_t *ja0,
                                                       d2 *val0, uint8_t *code0, int64_t *ia1, int32_t *ja1, d2 *val1,
                                                       uint8_t *code1, int code_w)
{
    const uint16_t *wcode = reinterpret_cast<const uint16_t *>(code);
    uint16_t *wcode0 = reinterpret_cast<uint16_t *>(code0), *wcode1 = reinterpret_cast<uint16_t *>(code1);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r <= nrows; r += stride) {
        ia1[r] = ia[r] - ia0[r];
        if (r == nrows) break;
        int64_t q0 = ia0[r], q1 = ia[r] - ia0[r];
        for (int64_t p = ia[r]; p < ia[r + 1]; ++p) {
            const int32_t col = ja[p];
            if (col >= lo && col < hi) {
                ja0[q0] = col;
                if (code && code_w == 2) wcode0[q0] = wcode[p];
                else if (code) code0[q0] = code[p];
                else      val0[q0] = val[p];
                ++q0;
            } else {
                ja1[q1] = col;
                if (code && code_w == 2) wcode1[q1] = wcode[p];
                else if (code) code1[q1] = code[p];
                else      val1[q1] = val[p];
                ++q1;
            }
        }
    }
}

int launch_split_count(const int64_t *ia, const int32_t *ja, int64_t nrows, int32_t lo, int32_t hi, int32_t *cnt0, hipStream_t s)
{
    return launch_kernel(k_split_count, blas_grid(nrows), kBlock, s, ia, ja, nrows, lo, hi, cnt0);
}

int launch_split_fill(const int64_t *ia, const int32_t *ja, const d2 *val, const uint8_t *code, int64_t nrows, int32_t lo,
                      int32_t hi, const int64_t *ia0, int32_t *ja0, d2 *val0, uint8_t *code0, int64_t *ia1, int32_t *ja1,
                      d2 *val1, uint8_t *code1, int code_w, hipStream_t s)
{
    return launch_kernel(k_split_fill, blas_grid(nrows + 1), kBlock, s, ia, ja, val, code, nrows, lo, hi, ia0, ja0, val0, code0, ia1, ja1, val1,
                         code1, code_w);
}

// exclusive scan int32 counts -> int64 offsets (three small kernels; one-time setup work)
constexpr int kScanChunk = 2048;

__global__ __launch_bounds__(256) void k_scan_chunksum(const int32_t *cnt, int64_t n, int64_t *chunk_sum)
{
    __shared__ double red_dummy;   // keep LDS layout trivial
    (void)red_dummy;
    __shared__ long long sm[4];
    const int64_t base = (int64_t)blockIdx.x * kScanChunk;
    long long s = 0;
    for (int i = threadIdx.x; i < kScanChunk; i += 256)
        if (base + i < n) s += cnt[base + i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ void k_scan_chunks_serial(int64_t *chunk_sum, int64_t nchunks)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int64_t run = 0;
        for (int64_t i = 0; i < nchunks; ++i) {
            const int64_t t = chunk_sum[i];
            chunk_sum[i] = run;
            run += t;
        }
        chunk_sum[nchunks] = run;
    }
}

__global__ __launch_bounds__(256) void k_scan_apply(const int32_t *cnt, int64_t n, const int64_t *chunk_off,
                                                    int64_t *ia)
{
    // one workgroup per chunk; thread t scans 8 consecutive elements, wave/LDS scan of the sums
    __shared__ long long wsum[4];
    const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * 8;
    long long loc[8], tot = 0;
    for (int i = 0; i < 8; ++i) {
        loc[i] = tot;
        if (base + i < n) tot += cnt[base + i];
    }
    long long incl = tot;                                // inclusive scan across the wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const long long t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    long long woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    const long long excl = chunk_off[blockIdx.x] + woff + incl - tot;
    for (int i = 0; i < 8; ++i)
        if (base + i < n) ia[base + i] = excl + loc[i];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) ia[n] = chunk_off[gridDim.x];
}

int exclusive_scan(const int32_t *d_cnt, int64_t n, int64_t *d_ia, hipStream_t s)
{
    if (n <= 0) {                                // an empty part (a cut sector's class without rows of that kind): ia = {0}; a launch of no
        QBH_HIP(hipMemsetAsync(d_ia, 0, sizeof(int64_t), s));       // workgroups is an error that would stay behind as the "last error"
        QBH_HIP(hipStreamSynchronize(s));
        return QBH_OK;
    }
    const int64_t nchunks = (n + kScanChunk - 1) / kScanChunk;
    int64_t *d_chunk = nullptr;
    QBH_HIP(qbh::dev_alloc(&d_chunk, (size_t)(nchunks + 1) * sizeof(int64_t)));
    hipLaunchKernelGGL(k_scan_chunksum, dim3((unsigned)nchunks), dim3(256), 0, s, d_cnt, n, d_chunk);
    hipLaunchKernelGGL(k_scan_chunks_serial, dim3(1), dim3(64), 0, s, d_chunk, nchunks);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nchunks), dim3(256), 0, s, d_cnt, n, d_chunk, d_ia);
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(d_chunk);
    if (e != hipSuccess) {
        set_error("scan failed: %s", hipGetErrorString(e));
        return QBH_EHIP;
    }
    return QBH_OK;
}

}  // namespace qbh
