"""Time per product of prost.block.wavelet2d (prost_amd/csrc/kernels_linop_wavelet2d.hip) at 256^2, 512^2, 1024^2 and 2048^2, L = 1,
for haar, db2 and a 16-tap filter, fp32 and fp64, forward and transposed, at the deepest level count the limits allow up to 8, through
the C ABI, beside two yardsticks on the same GPU in the same process:
  * `copy`: torch's copy_ of one plane, N values read and N written -- the 2 N values level 1 has to move at the very least;
  * `sparse twin`: the product of prost.block.sparse (prost_hip_csr_spmv) with the explicit matrix of the same transform, built here
    with scipy.sparse from the one-level matrices; only where the matrix stays below `twin_nnz` non-zeros (its coarse rows wrap around
    the whole image and are dense), "not built" otherwise.
Also timed: the forward product with the one-workgroup tail off (geometry.no_tail), one launch per level all the way down.
How it was measured: one sample is `chain` calls back to back between two host synchronisations, divided by `chain` (the launch latency
is amortised, not removed); the candidates alternate inside a round; after one warm-up round `reps` rounds give the median, the
smallest and the largest sample.  The vectors of 256^2 .. 1024^2 fit in the last-level cache, so the small sizes are warm-cache
figures.  Before any timing the forward product is checked against the sparse twin (where built) within the derived bound B of
tests/wavelet2d_reference.py, and K^T K x against x within 2 B: a guard against timing a wrong product, not the accuracy test
(that is tests/test_gpu_wavelet2d.py).  Also printed: launches per product, the device bytes of the block beside the twin's.
usage: python tools/wavelet2d_rate.py [reps] [chain] [largest size] [twin_nnz]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prost_amd as prost  # noqa: E402
import wavelet2d_reference as R  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
largest = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
twin_nnz = int(sys.argv[4]) if len(sys.argv) > 4 else 20_000_000
SIG = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
SPMV = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
TAIL_VALUES = 4096

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(27)


def sync():
    _hip.sync()
    torch.cuda.synchronize()


def rounds(calls):
    """{name: call} -> {name: samples in seconds per call}; the candidates alternate inside a round, the first round warms up"""
    samples = {name: [] for name in calls}
    for r in range(reps + 1):
        for name, call in calls.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(chain):
                call()
            sync()
            if r > 0:
                samples[name].append((time.perf_counter() - t0) / chain)
    return samples


def deepest(size, ntaps):
    return max(l for l in range(1, 9) if size % 2 ** l == 0 and size // 2 ** (l - 1) >= ntaps)


def launches(size, levels, tail):
    tiled = sum(1 for l in range(levels) if (size >> l) ** 2 > TAIL_VALUES) if tail else levels
    return tiled + (1 if tiled < levels else 0)


def one_level(m, h):
    g = R.high_pass(h)
    k, t = np.meshgrid(np.arange(m // 2), np.arange(len(h)), indexing="ij")
    cols = (2 * k + t) % m
    rows = np.concatenate([k.ravel(), m // 2 + k.ravel()])
    vals = np.concatenate([np.broadcast_to(h, k.shape).ravel(), np.broadcast_to(g, k.shape).ravel()])
    return sp.csr_matrix((vals, (rows, np.concatenate([cols.ravel(), cols.ravel()]))), shape=(m, m))


def twin_matrix(size, h, levels):
    """the explicit matrix as CSR, or None once it outgrows twin_nnz: level l is kron(W_x, W_y) on the corner's indices, the identity elsewhere"""
    N = size * size
    K = sp.identity(N, format="csr")
    for l in range(levels):
        m = size >> l
        W = one_level(m, h)
        if W.nnz ** 2 > twin_nnz:
            return None
        corner = (np.arange(m)[:, None] * size + np.arange(m)[None, :]).ravel()          # p = y + x ny, x-major
        inside = np.zeros(N, bool)
        inside[corner] = True
        kron = sp.kron(W, W, format="coo")
        level = sp.coo_matrix((np.concatenate([kron.data, np.ones(N - corner.size)]),
                               (np.concatenate([corner[kron.row], np.nonzero(~inside)[0]]), np.concatenate([corner[kron.col], np.nonzero(~inside)[0]]))), shape=(N, N)).tocsr()
        K = level @ K
        if K.nnz > twin_nnz:
            return None
    K.sort_indices()
    return K


for size in (s for s in (256, 512, 1024, 2048) if s <= largest):
    nx = ny = size
    N = nx * ny
    for wavelet in ("haar", "db2", "lat16"):
        h = R.taps(wavelet)
        levels = deepest(size, len(h))
        t0 = time.perf_counter()
        K = twin_matrix(size, h, levels)
        build = time.perf_counter() - t0
        for dtype in (np.float32, np.float64):
            name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
            fn = _hip.fn("wavelet2d", dtype)
            fn.argtypes, fn.restype = SIG, C.c_int
            spmv = _hip.fn("csr_spmv", dtype)
            spmv.argtypes, spmv.restype = SPMV, C.c_int
            x = rng.standard_normal(N).astype(dtype)
            nwork = R.work_size(nx, ny, 1, levels)
            d_x, d_r, d_b, d_w = _hip.DeviceArray.from_host(x), _hip.DeviceArray.zeros(N, dtype), _hip.DeviceArray.zeros(N, dtype), _hip.DeviceArray.zeros(nwork, dtype)
            taps = np.ascontiguousarray(h, dtype)
            a, b = (torch.zeros(N, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda") for _ in range(2))
            keep = {k: R.abi_record(nx, ny, 1, len(h), levels, k == "transposed", k == "no tail") for k in ("forward", "transposed", "no tail")}
            twin = None
            if K is not None:
                twin = [_hip.DeviceArray.from_host(K.data.astype(dtype)), _hip.DeviceArray.from_host(K.indptr.astype(np.int32)), _hip.DeviceArray.from_host(K.indices.astype(np.int32))]

            def product(g, res=d_r, rhs=d_x):
                _hip.check(fn(g.ctypes.data_as(C.c_void_p), taps.ctypes.data_as(C.c_void_p), d_w.ptr, res.ptr, rhs.ptr, 0, None))

            def twin_product():
                _hip.check(spmv(d_b.ptr, d_x.ptr, N, K.nnz, twin[0].ptr, twin[1].ptr, twin[2].ptr, None))

            # spot checks before any timing
            B = R.bound(wavelet, levels, dtype)
            product(keep["forward"])
            sync()
            got = d_r.to_host()
            product(keep["no tail"], res=d_b)
            sync()
            assert np.array_equal(got, d_b.to_host()), "the tail changes the bits"
            product(keep["transposed"], res=d_b, rhs=d_r)
            sync()
            back = np.linalg.norm(d_b.to_host().astype(np.float64) - x.astype(np.float64)) / np.linalg.norm(x.astype(np.float64))
            assert back <= 2 * B, (back, B)
            err = float("nan")
            if twin:
                twin_product()
                sync()
                err = np.linalg.norm(got.astype(np.float64) - d_b.to_host().astype(np.float64)) / np.linalg.norm(x.astype(np.float64))
                assert err <= B, (err, B)
            calls = {"block forward": lambda: product(keep["forward"]), "block forward, no tail": lambda: product(keep["no tail"]),
                     "block transposed": lambda: product(keep["transposed"]), "copy": lambda: b.copy_(a)}
            if twin:
                calls["sparse twin"] = twin_product
            s = rounds(calls)
            med = {k: statistics.median(v) for k, v in s.items()}
            tag = "%4d^2 %-5s %d levels %s" % (size, wavelet, levels, name)
            for k, v in s.items():
                print("chain %s %-22s: median %.4f ms (%.4f .. %.4f over %d samples of %d calls)" % (tag, k, med[k] * 1e3, min(v) * 1e3, max(v) * 1e3, len(v), chain), flush=True)
            twin_text = ("sparse twin / block forward %.1f, |block - twin| / |x| = %.2g (bound %.2g), twin built in %.1f s, %d non-zeros, %.1f MB for K and K^T"
                         % (med["sparse twin"] / med["block forward"], err, B, build, K.nnz, 2 * (K.nnz * (item + 4) + 4 * (N + 1)) / 1e6)) if twin else \
                "sparse twin not built (%s)" % ("more than %d non-zeros after %.1f s" % (twin_nnz, build))
            print("ratio %s: block forward / copy %.2f, transposed / copy %.2f, forward without the tail / with it %.2f; launches %d with the tail, %d without; "
                  "|K^T K x - x| / |x| = %.2g; device bytes of the block %.2f MB (work buffer of %d values); %s"
                  % (tag, med["block forward"] / med["copy"], med["block transposed"] / med["copy"], med["block forward, no tail"] / med["block forward"],
                     launches(size, levels, True), launches(size, levels, False), back, nwork * item / 1e6, nwork, twin_text), flush=True)
            if twin:
                assert med["block forward"] < med["sparse twin"] and med["block transposed"] < med["sparse twin"], "the block has to be faster than its sparse twin"
            for v in [d_x, d_r, d_b, d_w] + (twin or []):
                v.free()
            del a, b
