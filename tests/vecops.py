"""References, comparison rules and the driver's file format for the tests of the solvers' vector kernels
(csrc/qbh_blas1.hip and the tile kernels): plain numpy, nothing of the library.

References are formed in np.longdouble from the same double inputs; integer results in Python integers.  Inputs have
magnitudes in [0.5, 1.5] with random signs / phases, so no element is negligible and sum|terms| is of order n.

No tolerance is a tuned number (u = 2^-53):
  element-wise, per real component:  k u sum|terms of that component|, k = floating-point operations of the source expression
                                     (a fused multiply-add rounds once instead of twice and only lowers the error)
  reduction:                         (L + ceil(nparts / 1024) + 40) u sum|t_i|, L = ceil(n / (grid 256)) the chain of one thread;
                                     40 covers the products (and the rounding of an updated element before it is squared:
                                     <= 8 u of its term bound), the 6 + 2 steps of block_sum and the 6 + 16 of the second stage
  exact:                             bit equality
"""
import atexit
import concurrent.futures
import os
import shutil
import subprocess
import tempfile

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
CLD = np.clongdouble
SENTINEL = 0x7FF8DEADBEEF0001           # the driver's NaN with a fixed payload
QBH_EINVAL = -1
KBLOCK, MAXRED = 256, 2048
LEHMER_M = 2147483647
NTHREADS = min(16, len(os.sched_getaffinity(0)))       # numpy's longdouble loops are slow and release the GIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ inputs
def rng(seed):
    return np.random.default_rng(seed)


def rvec(g, n):
    return (g.uniform(0.5, 1.5, n) * g.choice([-1.0, 1.0], n)).astype(np.float64)


def cvec(g, n):
    return (g.uniform(0.5, 1.5, n) * np.exp(2j * np.pi * g.uniform(0.0, 1.0, n))).astype(np.complex128)


def blas_grid(n):
    """grid of the BLAS-1 kernels == number of partial sums (restated; the driver itself calls qbh::blas_grid)"""
    return int(min(max((n + KBLOCK - 1) // KBLOCK, 1), MAXRED))


def chain(n, grid=None):
    grid = blas_grid(n) if grid is None else grid
    return -(-n // (grid * KBLOCK))


# ------------------------------------------------------------------ tile map
def tile_map(S, NU, B):
    """position of element r = u S + d of the product basis in the band-major order: bands of B minor indices (the last one
    narrower), inside a band the major indices one after the other, each with its wB minor indices"""
    pos = np.empty(S * NU, dtype=np.int64)
    at = 0
    for d0 in range(0, S, B):
        wB = min(B, S - d0)
        for u in range(NU):
            pos[u * S + d0:u * S + d0 + wB] = np.arange(at, at + wB)
            at += wB
    return pos


def tile_map_formula(S, NU, B):
    """KronTile::tile restated with array arithmetic"""
    r = np.arange(S * NU, dtype=np.int64)
    u, d = r // S, r % S
    b, j = d // B, d % B
    wB = np.minimum(S - b * B, B)
    return b * B * NU + u * wB + j


# ------------------------------------------------------------------ start vector
def lehmer_stream(n, seed, offset=0, major_inv=None, S=0):
    """element j of k_randomize before normalisation: draw pos(j) + 1 of std::minstd_rand0 seeded with `seed`, as
    v = state * (1 / 2147483647.0) - 0.5 in doubles (two roundings: the kernel is compiled with contraction off)"""
    s0 = seed % LEHMER_M or 1
    pref = np.float64(1.0) / np.float64(2147483647.0)
    out = np.empty(n, dtype=np.float64)
    for j in range(n):
        pos = (int(major_inv[j // S]) * S + j % S) if major_inv is not None else offset + j
        state = s0 * pow(16807, pos + 1, LEHMER_M) % LEHMER_M
        out[j] = np.float64(state) * pref - np.float64(0.5)
    return out


# ------------------------------------------------------------------ comparison rules
def exact(got, want):
    """bit equality (distinguishes -0 from +0 and every NaN payload)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    word = np.uint64 if got.dtype.itemsize % 8 == 0 else np.uint32
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.array_equal(got.view(word), want.view(word)))


def comps(z):
    """real components of a complex (or real) array as longdouble, shape (..., 2) for complex"""
    z = np.asarray(z)
    if np.iscomplexobj(z):
        return np.stack([z.real.astype(LD), z.imag.astype(LD)], axis=-1)
    return np.asarray(z, dtype=LD)


def elementwise_ratio(got, ref, k, sumabs):
    """largest |got - ref| / (k u sum|terms|) over the real components; <= 1 passes.  NaN (an element not written) -> inf."""
    err = np.abs(comps(got) - comps(ref))
    bound = LD(k * U) * np.asarray(sumabs, dtype=LD)
    if err.shape != bound.shape or not np.all(np.isfinite(err)):
        return np.inf
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore"):
        np.divide(err, bound, out=err, where=err > 0)         # an exact element stays 0, whatever its bound
    return float(np.max(err))


def elementwise_ratio_rows(got, ref, k, sumabs):
    """elementwise_ratio of a stack of vectors, the largest over the rows; the rows are shared among threads"""
    with concurrent.futures.ThreadPoolExecutor(NTHREADS) as ex:
        return max(ex.map(lambda c: elementwise_ratio(got[c], ref[c], k, sumabs[c]), range(len(got))))


def reduction_bound(n, nparts, sumabs, L=None):
    L = chain(n, nparts) if L is None else L
    return (L + -(-nparts // 1024) + 40) * U * float(sumabs)


def reduction_ratio(got, ref, n, nparts, sumabs, L=None):
    """|got - ref| / bound for one reduced number; NaN (a partial sum nobody wrote) -> inf"""
    if not np.isfinite(got):
        return np.inf
    b = reduction_bound(n, nparts, sumabs, L)
    e = abs(LD(got) - LD(ref))
    return 0.0 if e == 0 else float(e / LD(b))


def tiled_exact(yt, y, tmap):
    """the tiled copy holds exactly the bits of the natural-order result: yt[tmap[r]] == y[r]"""
    yt = np.ascontiguousarray(yt)
    return yt.shape == np.shape(y) and exact(yt[tmap], y)


# ------------------------------------------------------------------ references (longdouble)
def cmul_abs(a, x):
    """sum|terms| of the two components of a * x, shape (..., 2)"""
    a, x = np.asarray(a), np.asarray(x)
    ar, ai, xr, xi = np.abs(a.real).astype(LD), np.abs(a.imag).astype(LD), np.abs(x.real).astype(LD), np.abs(x.imag).astype(LD)
    return np.stack([ar * xr + ai * xi, ar * xi + ai * xr], axis=-1)


def cabs(y):
    return np.stack([np.abs(y.real).astype(LD), np.abs(y.imag).astype(LD)], axis=-1)


def ref_axpy(alpha, x, y):
    """y + alpha x (complex): reference and sum|terms| per component; k = 4"""
    return y.astype(CLD) + CLD(alpha) * x.astype(CLD), cabs(y) + cmul_abs(alpha, x)


def ref_axpy_re(alpha, x, y):
    return y.astype(LD) + LD(alpha) * x.astype(LD), np.abs(y).astype(LD) + abs(LD(alpha)) * np.abs(x).astype(LD)


def norm_terms(sumabs):
    """|v|^2 of an updated element: the reference sum and the bound's sum|t| take the squares of the components' term sums"""
    return float(np.sum(np.asarray(sumabs, dtype=LD) ** 2))


def ref_nrm2sq(v):
    c = comps(v)
    return np.sum(c * c)


def ref_dotc(x, y):
    """<x, y> = sum conj(x) y: (re, im) and sum|t| of each"""
    xr, xi, yr, yi = x.real.astype(LD), x.imag.astype(LD), y.real.astype(LD), y.imag.astype(LD)
    return (np.sum(xr * yr + xi * yi), np.sum(xr * yi - xi * yr)), (float(np.sum(np.abs(xr * yr) + np.abs(xi * yi))), float(np.sum(np.abs(xr * yi) + np.abs(xi * yr))))


def cg_alpha_from_delta(accu2, delta):
    """alpha = accu2 conj(delta) / |delta|^2 in the kernel's double arithmetic, operation by operation"""
    re, im, a = np.float64(delta.real), np.float64(delta.imag), np.float64(accu2)
    den = re * re + im * im
    return complex((a * re) / den, -((a * im) / den))


def ref_multi_dot(V, w):
    """h_i = <V_i, w>: list of ((re, im), (sum|t| re, sum|t| im))"""
    return [ref_dotc(V[i], w) for i in range(V.shape[0])]


def ref_multi_axpy(V, c, w):
    """w - sum_{i < nv} c_i V_i for nv = 1 ... len(V): list of (reference, sum|terms|), entry nv - 1 for nv vectors; k = 4 nv"""
    ref, sa, prefixes = w.astype(CLD), cabs(w), []
    for i in range(V.shape[0]):
        ref = ref - CLD(c[i]) * V[i].astype(CLD)
        sa = sa + cmul_abs(c[i], V[i])
        prefixes.append((ref, sa))
    return prefixes


def _ld_matmul(A, X, step=8192):
    """A @ X in longdouble (A: k x m longdouble, X: m x N double).  numpy has no fast longdouble product, so the columns
    are shared among threads in blocks, each block transposed so that the inner loop runs over contiguous memory."""
    def part(j):
        return (np.ascontiguousarray(X[:, j:j + step].T).astype(LD) @ A.T).T
    with concurrent.futures.ThreadPoolExecutor(NTHREADS) as ex:
        return np.concatenate(list(ex.map(part, range(0, X.shape[1], step))), axis=1)


def ref_rotate(V, Smat, keep):
    """V[c] <- sum_i S[i + c m] V[i], c < keep (S real, column-major m x keep): reference and sum|terms|, shape
    (keep, n, 2); k = 2 m"""
    m, n = V.shape
    Sm = np.ascontiguousarray(np.asarray(Smat, dtype=LD).reshape(keep, m))     # Sm[c, i] = S[i + c m]
    X = np.ascontiguousarray(V).view(np.float64)                               # m x 2n: re, im interleaved
    return _ld_matmul(Sm, X).reshape(keep, n, 2), _ld_matmul(np.abs(Sm), np.abs(X)).reshape(keep, n, 2)


# ------------------------------------------------------------------ injected faults (the CPU tests' teeth)
def drop_one_from_sum(terms, index):
    """the float64 sum of `terms` with one element left out"""
    t = np.array(terms, dtype=np.float64)
    t[index] = 0.0
    return float(np.sum(t))


def exchange_two(a, i, j):
    b = np.array(a)
    b[i], b[j] = a[j], a[i]
    return b


# ------------------------------------------------------------------ the driver
def build_driver(tmp):
    """compile tests/cxx/vecops_main.cpp as HIP against libqbhip.so; returns the program's path"""
    exe = os.path.join(tmp, "vecops_main")
    lib = os.path.join(ROOT, "quantum_basis_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(lib, "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "vecops_main.cpp"), "-o", exe,
                           "-L", lib, "-lqbhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


_DRIVER = []


def driver():
    """the driver, built once per process into a temporary directory"""
    if not _DRIVER:
        tmp = tempfile.mkdtemp(prefix="vecops_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _DRIVER.append(build_driver(tmp))
    return _DRIVER[0]


class Buf:
    def __init__(self, mode, dtype, count, data=None):
        self.mode, self.dtype, self.count, self.data = mode, np.dtype(dtype), int(count), data


def cin(a):
    """input the launcher takes as const"""
    a = np.ascontiguousarray(a)
    return Buf(0, a.dtype, a.size, a)


def io(a):
    """buffer the launcher reads and writes"""
    a = np.ascontiguousarray(a)
    return Buf(1, a.dtype, a.size, a)


def out(dtype, count, host=False):
    """output buffer, pre-filled with the sentinel (hipHostMalloc memory when host)"""
    return Buf(2 if host else 1, dtype, count)


class Result:
    """rc: the launcher's return code; guard, const: changed guard words and changed words of const buffers"""

    def __init__(self, rc, guard, const, outs):
        self.rc, self.guard, self.const, self.out = rc, guard, const, outs


class Batch:
    """the cases of one driver process"""

    def __init__(self):
        self.cases, self.blob, self.seen = [], bytearray(), {}

    def _offset(self, a):
        key = id(a)                      # the same array object is stored once (inputs shared between cases)
        if key not in self.seen:
            self.seen[key] = (len(self.blob), a)
            self.blob += a.tobytes()
            self.blob += b"\0" * (-len(self.blob) % 16)
        return self.seen[key][0]

    def add(self, op, bufs, ints, dbls=(), post=()):
        """post: (partials buffer, n for blas_grid, ncomp, result buffer); returns the case's number"""
        self.cases.append((op, list(bufs), [int(i) for i in ints], [float(d) for d in dbls], list(post)))
        return len(self.cases) - 1

    def run(self, exe, tmp, timeout=120):
        man, inp, outp = (os.path.join(tmp, f) for f in ("manifest.txt", "inputs.bin", "outputs.bin"))
        lines = [str(len(self.cases))]
        for op, bufs, ints, dbls, post in self.cases:
            lines.append("C %s %d %d %d %d" % (op, len(bufs), len(ints), len(dbls), len(post)))
            for b in bufs:
                lines.append("B %d %d %d" % (b.count * b.dtype.itemsize, b.mode, self._offset(b.data) if b.data is not None else -1))
            lines.append("I " + " ".join(str(i) for i in ints))
            lines.append("D " + " ".join("%016x" % int(np.float64(d).view(np.uint64)) for d in dbls))
            lines += ["R %d %d %d %d" % p for p in post]
        with open(man, "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(inp, "wb") as f:
            f.write(self.blob)
        p = subprocess.run([exe, man, inp, outp], capture_output=True, text=True, timeout=timeout)
        assert p.returncode == 0, "driver exit %d\n%s%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
        rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("CASE ")]
        assert len(rows) == len(self.cases) and ("DONE %d" % len(self.cases)) in p.stdout, p.stdout[-4000:]
        res = []
        with open(outp, "rb") as f:
            for k, (op, bufs, ints, dbls, post) in enumerate(self.cases):
                assert int(rows[k][1]) == k
                outs = {}
                for i, b in enumerate(bufs):
                    if b.mode != 0:
                        outs[i] = np.fromfile(f, dtype=b.dtype, count=b.count)
                        assert outs[i].size == b.count
                res.append(Result(int(rows[k][3]), int(rows[k][5]), int(rows[k][7]), outs))
        os.remove(outp)
        return res


def is_sentinel(a):
    """every 8-byte word of the array still holds the sentinel"""
    return bool(np.all(np.ascontiguousarray(a).view(np.uint64) == np.uint64(SENTINEL)))
