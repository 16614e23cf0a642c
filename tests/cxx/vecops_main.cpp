// vecops_main.cpp -- calls the launchers of the solvers' vector kernels (qbh::launch_*, csrc/qbh_internal.hpp) one by one on
// inputs the Python side wrote, for tests/test_gpu_vecops.py.  Compiled as HIP (d2 is an ext_vector_type), linked to libqbhip.so.
//
//   vecops_main <manifest> <inputs.bin> <outputs.bin>
//
// manifest (text):  <ncases>, then per case
//   C <op> <nbuf> <ni> <nd> <npost>
//   B <bytes> <mode> <offset>      nbuf lines; mode 0 = device, const for the launcher; 1 = device, writable; 2 = hipHostMalloc,
//                                  writable; offset into inputs.bin, or -1 = filled with the sentinel
//   I <ni integers>                buffer numbers (-1 = nullptr), sizes, switches: the meaning is per op, see run_op
//   D <nd doubles as 16 hex digits>
//   R <pbuf> <gridn> <ncomp> <rbuf>   npost lines: rbuf = launch_reduce_partials(pbuf, blas_grid(gridn), ncomp)
// Every case runs on the null stream and is synchronised; every HIP return code is checked.  A writable buffer lies between two
// guard zones of 256 elements (4 KB each) that hold a NaN with a fixed payload, as does every byte no input was given for.
// stdout, one line per case:  CASE <k> rc <launcher's return code> guard <changed guard words> const <changed words of const buffers>
// outputs.bin: the writable buffers of every case, in order.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "qbh_internal.hpp"

using qbh::d2;

namespace {

constexpr uint64_t kSentinel = 0x7FF8DEADBEEF0001ULL;      // quiet NaN, fixed payload
constexpr size_t kGuard = 4096;                             // bytes: 256 elements of 16 bytes

#define CK(call)                                                                                       \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            std::printf("HIPERR %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);          \
            std::fflush(stdout);                                                                       \
            std::exit(4);                                                                              \
        }                                                                                              \
    } while (0)

struct Buf {
    size_t bytes = 0, padded = 0;
    int mode = 0;
    long long off = -1;
    char *base = nullptr;            // allocation: guard | padded payload | guard
    std::vector<uint64_t> init;      // payload as uploaded (padded / 8 words)
    char *ptr() const { return base + kGuard; }
};

struct Case {
    std::string op;
    std::vector<Buf> b;
    std::vector<long long> I;
    std::vector<double> D;
    struct Post { int p; long long gridn; int ncomp, r; };
    std::vector<Post> post;
};

[[noreturn]] void die(const char *what)
{
    std::printf("ERROR %s\n", what);
    std::fflush(stdout);
    std::exit(2);
}

template <typename T>
T *ptr(const Case &c, int k)
{
    const long long i = c.I.at(k);
    if (i < 0) return nullptr;
    return reinterpret_cast<T *>(c.b.at((size_t)i).ptr());
}
template <typename T>
T *wptr(const Case &c, int k)      // a pointer the launcher writes through: the buffer must be writable (guarded and reported)
{
    const long long i = c.I.at(k);
    if (i >= 0 && c.b.at((size_t)i).mode == 0) die("a const buffer passed as output");
    return ptr<T>(c, k);
}

int run_op(const Case &c)
{
    const std::string &op = c.op;
    const auto &I = c.I;
    const auto &D = c.D;
    hipStream_t s = nullptr;
    auto tile = [&](int k) { return qbh::KronTile{(int64_t)I.at(k), (int64_t)I.at(k + 1), (int)I.at(k + 2)}; };
    // I = n, then buffer numbers in the launcher's argument order, then the remaining integers
    if (op == "dotc") return qbh::launch_dotc(ptr<const d2>(c, 1), ptr<const d2>(c, 2), I[0], wptr<double>(c, 3), s);
    if (op == "nrm2sq") return qbh::launch_nrm2sq(ptr<const d2>(c, 1), I[0], wptr<double>(c, 2), s);
    if (op == "scal") return qbh::launch_scal(D.at(0), wptr<d2>(c, 1), I[0], s);
    if (op == "scal_to") return qbh::launch_scal_to(D.at(0), ptr<const d2>(c, 1), wptr<d2>(c, 2), I[0], s);
    if (op == "axpy_norm")       // I: n, alpha_dev, x, y, partials, yr, flag, scale_dev
        return qbh::launch_axpy_norm(d2{D.at(0), D.at(1)}, ptr<const double>(c, 1), ptr<const d2>(c, 2), wptr<d2>(c, 3), I[0], wptr<double>(c, 4),
                                     wptr<double>(c, 5), wptr<int>(c, 6), s, ptr<const double>(c, 7));
    if (op == "xpby")            // I: n, x, y, yr, flag
        return qbh::launch_xpby(ptr<const d2>(c, 1), D.at(0), wptr<d2>(c, 2), I[0], wptr<double>(c, 3), wptr<int>(c, 4), s);
    if (op == "cg_update")       // I: n, p, pp, v, r, partials, delta_dev;  D: alpha.re, alpha.im, accu2
        return qbh::launch_cg_update(d2{D.at(0), D.at(1)}, ptr<const d2>(c, 1), ptr<const d2>(c, 2), wptr<d2>(c, 3), wptr<d2>(c, 4), I[0],
                                     wptr<double>(c, 5), s, ptr<const double>(c, 6), D.at(2));
    if (op == "fill_const") return qbh::launch_fill_const(wptr<d2>(c, 1), I[0], D.at(0), s);
    if (op == "imag_norm") return qbh::launch_imag_norm(ptr<const d2>(c, 1), I[0], wptr<double>(c, 2), s);
    if (op == "pack_real") return qbh::launch_pack_real(ptr<const d2>(c, 1), wptr<double>(c, 2), I[0], wptr<int>(c, 3), s);
    if (op == "unpack_real") return qbh::launch_unpack_real(ptr<const double>(c, 1), wptr<d2>(c, 2), I[0], s);
    if (op == "dot_re") return qbh::launch_dot_re(ptr<const double>(c, 1), ptr<const double>(c, 2), I[0], wptr<double>(c, 3), s);
    if (op == "nrm2sq_re") return qbh::launch_nrm2sq_re(ptr<const double>(c, 1), I[0], wptr<double>(c, 2), s);
    if (op == "scal_re") return qbh::launch_scal_re(D.at(0), wptr<double>(c, 1), I[0], s);
    if (op == "axpy_norm_re") {  // I: n, alpha_dev, x, y, partials, yt, S, NU, B
        if (I.at(5) < 0) return qbh::launch_axpy_norm_re(D.at(0), ptr<const double>(c, 1), ptr<const double>(c, 2), wptr<double>(c, 3), I[0], wptr<double>(c, 4), s);
        return qbh::launch_axpy_norm_re(D.at(0), ptr<const double>(c, 1), ptr<const double>(c, 2), wptr<double>(c, 3), I[0], wptr<double>(c, 4), s,
                                        wptr<double>(c, 5), tile(6));
    }
    if (op == "xpby_re") return qbh::launch_xpby_re(ptr<const double>(c, 1), D.at(0), wptr<double>(c, 2), I[0], s);
    if (op == "cg_update_re")    // I: n, p, pp, v, r, partials
        return qbh::launch_cg_update_re(D.at(0), ptr<const double>(c, 1), ptr<const double>(c, 2), wptr<double>(c, 3), wptr<double>(c, 4), I[0],
                                        wptr<double>(c, 5), s);
    if (op == "basis_scatter") return qbh::launch_basis_scatter(ptr<const uint32_t>(c, 1), ptr<const d2>(c, 2), wptr<d2>(c, 3), I[0], s);
    if (op == "basis_gather") return qbh::launch_basis_gather(ptr<const uint32_t>(c, 1), ptr<const d2>(c, 2), wptr<d2>(c, 3), I[0], s);
    if (op == "basis_scatter_re") return qbh::launch_basis_scatter_re(ptr<const uint32_t>(c, 1), ptr<const double>(c, 2), wptr<double>(c, 3), I[0], s);
    if (op == "reduce_partials")    // I: nparts, partials, ncomp, out
        return qbh::launch_reduce_partials(ptr<const double>(c, 1), (int)I[0], (int)I.at(2), wptr<double>(c, 3), s);
    if (op == "lanczos_tail")    // I: nparts, partials, dot, state, log_slot, use_host, sq_ready;  D: sc_x_host
        return qbh::launch_lanczos_tail(ptr<const double>(c, 1), (int)I[0], ptr<const double>(c, 2), wptr<double>(c, 3), wptr<double>(c, 4), D.at(0),
                                        (int)I.at(5), s, ptr<const double>(c, 6));
    if (op == "multi_dot8")      // I: n, V, ldv, w, nv, partials
        return qbh::launch_multi_dot8(ptr<const d2>(c, 1), I.at(2), ptr<const d2>(c, 3), I[0], (int)I.at(4), wptr<double>(c, 5), s);
    if (op == "multi_axpy8") {   // I: n, V, ldv, nv, w, partials;  D: 16 coefficients
        qbh::Coef8 cf;
        for (int i = 0; i < 16; ++i) cf.v[i] = D.at((size_t)i);
        return qbh::launch_multi_axpy8(ptr<const d2>(c, 1), I.at(2), cf, (int)I.at(3), wptr<d2>(c, 4), I[0], wptr<double>(c, 5), s);
    }
    if (op == "basis_rotate")    // I: n, V, ldv, m, keep, S
        return qbh::launch_basis_rotate(wptr<d2>(c, 1), I.at(2), I[0], (int)I.at(3), (int)I.at(4), ptr<const double>(c, 5), s);
    if (op == "kron_tile")       // I: n, x, xt, S, NU, B, xt_real, flag
        return qbh::launch_kron_tile(ptr<const d2>(c, 1), wptr<d2>(c, 2), I[0], tile(3), s, (int)I.at(6), wptr<int>(c, 7));
    if (op == "kron_tile_re")    // I: n, x, xt, S, NU, B
        return qbh::launch_kron_tile_re(ptr<const double>(c, 1), wptr<double>(c, 2), I[0], tile(3), s);
    if (op == "axpy_norm_tile")  // I: n, alpha_dev, x, y, yt, S, NU, B, partials, scale_dev, yt_real, flag
        return qbh::launch_axpy_norm_tile(d2{D.at(0), D.at(1)}, ptr<const double>(c, 1), ptr<const d2>(c, 2), wptr<d2>(c, 3), wptr<d2>(c, 4), I[0], tile(5),
                                          wptr<double>(c, 8), s, ptr<const double>(c, 9), (int)I.at(10), wptr<int>(c, 11));
    if (op == "xpby_tile")       // I: n, x, y, yt, S, NU, B, yt_real, flag
        return qbh::launch_xpby_tile(ptr<const d2>(c, 1), D.at(0), wptr<d2>(c, 2), wptr<d2>(c, 3), I[0], tile(4), s, (int)I.at(7), wptr<int>(c, 8));
    if (op == "randomize")       // I: n, x, xr, global_offset, seed, partials, major_inv, S
        return qbh::launch_randomize(wptr<d2>(c, 1), wptr<double>(c, 2), I[0], I.at(3), (uint32_t)I.at(4), wptr<double>(c, 5), s, ptr<const int32_t>(c, 6),
                                     I.at(7));
    die(("unknown op " + op).c_str());
}

void read_manifest(const char *path, std::vector<Case> &cases)
{
    FILE *f = std::fopen(path, "r");
    if (!f) die("cannot open the manifest");
    int ncases = 0;
    if (std::fscanf(f, "%d", &ncases) != 1) die("manifest: case count");
    cases.resize((size_t)ncases);
    for (auto &c : cases) {
        char tag[8], op[64];
        int nbuf, ni, nd, npost;
        if (std::fscanf(f, "%7s %63s %d %d %d %d", tag, op, &nbuf, &ni, &nd, &npost) != 6 || tag[0] != 'C') die("manifest: case line");
        c.op = op;
        c.b.resize((size_t)nbuf);
        for (auto &b : c.b) {
            long long bytes;
            if (std::fscanf(f, "%7s %lld %d %lld", tag, &bytes, &b.mode, &b.off) != 4 || tag[0] != 'B') die("manifest: buffer line");
            b.bytes = (size_t)bytes;
            b.padded = (b.bytes + 7) / 8 * 8;
        }
        if (std::fscanf(f, "%7s", tag) != 1 || tag[0] != 'I') die("manifest: I line");
        c.I.resize((size_t)ni);
        for (auto &v : c.I)
            if (std::fscanf(f, "%lld", &v) != 1) die("manifest: integer");
        if (std::fscanf(f, "%7s", tag) != 1 || tag[0] != 'D') die("manifest: D line");
        c.D.resize((size_t)nd);
        for (auto &v : c.D) {
            uint64_t bits;
            if (std::fscanf(f, "%" SCNx64, &bits) != 1) die("manifest: double");
            std::memcpy(&v, &bits, 8);
        }
        c.post.resize((size_t)npost);
        for (auto &p : c.post)
            if (std::fscanf(f, "%7s %d %lld %d %d", tag, &p.p, &p.gridn, &p.ncomp, &p.r) != 5 || tag[0] != 'R') die("manifest: R line");
    }
    std::fclose(f);
}

}  // namespace

int main(int argc, char **argv)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        std::printf("no HIP device\n");
        return 3;
    }
    if (argc != 4) die("usage: vecops_main <manifest> <inputs> <outputs>");
    std::vector<Case> cases;
    read_manifest(argv[1], cases);
    FILE *fin = std::fopen(argv[2], "rb");
    FILE *fout = std::fopen(argv[3], "wb");
    if (!fin || !fout) die("cannot open the input or output file");
    CK(hipSetDevice(0));

    std::vector<uint64_t> host;
    for (size_t k = 0; k < cases.size(); ++k) {
        Case &c = cases[k];
        for (auto &b : c.b) {
            const size_t total = b.padded + 2 * kGuard;
            if (b.mode == 2) CK(hipHostMalloc((void **)&b.base, total, hipHostMallocDefault));
            else             CK(hipMalloc((void **)&b.base, total));
            host.assign(total / 8, kSentinel);
            if (b.off >= 0 && b.bytes > 0) {
                if (std::fseek(fin, (long)b.off, SEEK_SET) != 0 || std::fread((char *)host.data() + kGuard, 1, b.bytes, fin) != b.bytes)
                    die("short read of the input file");
            }
            b.init.assign(host.begin() + kGuard / 8, host.begin() + (kGuard + b.padded) / 8);
            CK(hipMemcpy(b.base, host.data(), total, hipMemcpyDefault));
        }
        CK(hipDeviceSynchronize());
        const int rc = run_op(c);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        for (const auto &p : c.post) {
            const int nparts = qbh::blas_grid(p.gridn);
            const Buf &pb = c.b.at((size_t)p.p), &rb = c.b.at((size_t)p.r);
            if ((size_t)nparts * (size_t)p.ncomp * 8 > pb.bytes || (size_t)p.ncomp * 8 > rb.bytes || rb.mode == 0) die("reduction outside its buffers");
            if (qbh::launch_reduce_partials((const double *)pb.ptr(), nparts, p.ncomp, (double *)rb.ptr(), nullptr) != QBH_OK) die("launch_reduce_partials");
            CK(hipGetLastError());
            CK(hipDeviceSynchronize());
        }
        long long guard_bad = 0, const_bad = 0;
        for (auto &b : c.b) {
            const size_t total = b.padded + 2 * kGuard;
            host.resize(total / 8);
            CK(hipMemcpy(host.data(), b.base, total, hipMemcpyDefault));
            for (size_t i = 0; i < kGuard / 8; ++i) {
                guard_bad += host[i] != kSentinel;
                guard_bad += host[(kGuard + b.padded) / 8 + i] != kSentinel;
            }
            if (b.mode == 0) {
                for (size_t i = 0; i < b.padded / 8; ++i) const_bad += host[kGuard / 8 + i] != b.init[i];
            } else if (b.bytes > 0 && std::fwrite((const char *)host.data() + kGuard, 1, b.bytes, fout) != b.bytes) {
                die("short write of the output file");
            }
            if (b.mode == 2) CK(hipHostFree(b.base));
            else             CK(hipFree(b.base));
            b.base = nullptr;
            std::vector<uint64_t>().swap(b.init);
        }
        std::printf("CASE %zu rc %d guard %lld const %lld\n", k, rc, guard_bad, const_bad);
    }
    std::fclose(fin);
    if (std::fclose(fout) != 0) die("closing the output file");
    std::printf("DONE %zu\n", cases.size());
    return 0;
}
