"""Time per product of prost.block.fft2d (prost_amd/csrc/kernels_linop_fft2d.hip) at 256^2, 512^2, 1024^2 and 2048^2, L = 1, fp32 and
fp64, forward and transposed, beside two yardsticks on the same GPU in the same process:
  * `torch.fft`: torch.fft.fft2 / torch.fft.ifft2 (norm="ortho") on a complex tensor of the same size (the vendor library; interleaved
    complex values, where the block works on two real planes);
  * `copy`: a plain device copy of the bytes the two passes move -- 2 N values of T copied twice (rhs -> work, work -> res) with
    torch's copy_: what the product would cost if it did no arithmetic and had no strided pass.
How it was measured: one sample is `chain` calls back to back between two host synchronisations, divided by `chain` (the launch latency
is amortised, not removed); the candidates alternate inside a round; after one warm-up round `reps` rounds give the median, the
smallest and the largest sample.  The vectors of 256^2 .. 1024^2 fit in the last-level cache (2048^2 in fp64: 64 MiB per vector, they
do not all), so the small sizes are warm-cache figures.  Before any timing the block's forward product is checked against torch.fft
in the same precision T: |block - torch.fft| <= 2 B |x|, B the derived bound of the block (tests/fft2d_reference.py) -- one B for the
block and one allowed for the library, whose transform in T has an error of the same kind; this is a guard against timing a wrong
product, not the accuracy test (that is tests/test_gpu_fft2d.py, against numpy.fft in float64).  Also printed: the device bytes of
the block (table and work buffer) beside the (2 N)^2 values of a dense twin.
usage: python tools/fft2d_rate.py [reps] [chain] [largest size]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fft2d_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
largest = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
SIG = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(25)


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


for size in (s for s in (256, 512, 1024, 2048) if s <= largest):
    nx = ny = size
    N = nx * ny
    for dtype, ctype in ((np.float32, torch.complex64), (np.float64, torch.complex128)):
        name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
        fn = _hip.fn("fft2d", dtype)
        fn.argtypes, fn.restype = SIG, C.c_int
        x = rng.standard_normal(2 * N).astype(dtype)
        d_x, d_r, d_w = _hip.DeviceArray.from_host(x), _hip.DeviceArray.zeros(2 * N, dtype), _hip.DeviceArray.zeros(2 * N, dtype)
        d_t = _hip.DeviceArray.from_host(np.ascontiguousarray(R.table(size, dtype)).reshape(-1))
        z = torch.from_numpy(x[:N].reshape(nx, ny) + 1j * x[N:].reshape(nx, ny)).to(ctype).cuda()
        a, b, c = (torch.zeros(2 * N, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda") for _ in range(3))
        keep = [R.abi_record(nx, ny, 1, False), R.abi_record(nx, ny, 1, True)]

        def product(g):
            _hip.check(fn(g.ctypes.data_as(C.c_void_p), d_t.ptr, d_w.ptr, d_r.ptr, d_x.ptr, 0, None))

        def copy_twice():
            b.copy_(a)
            c.copy_(b)

        # a spot check before any timing: the comparator runs in T as well, so B for the block plus B allowed for the library
        product(keep[0])
        sync()
        got = d_r.to_host().astype(np.float64)
        want = torch.fft.fft2(z, norm="ortho").cpu().numpy()
        err = np.linalg.norm(got - np.concatenate([want.real.reshape(-1), want.imag.reshape(-1)])) / np.linalg.norm(x.astype(np.float64))
        assert err <= 2 * R.bound(nx, ny, dtype), (err, R.bound(nx, ny, dtype))
        calls = {"block forward": lambda: product(keep[0]), "block transposed": lambda: product(keep[1]),
                 "torch.fft.fft2": lambda: torch.fft.fft2(z, norm="ortho"), "torch.fft.ifft2": lambda: torch.fft.ifft2(z, norm="ortho"), "copy": copy_twice}
        s = rounds(calls)
        med = {k: statistics.median(v) for k, v in s.items()}
        for k, v in s.items():
            print("chain %4d^2 %s %-16s: median %.4f ms (%.4f .. %.4f over %d samples of %d calls)" % (size, name, k, med[k] * 1e3, min(v) * 1e3, max(v) * 1e3, len(v), chain), flush=True)
        print("ratio %4d^2 %s: block forward / torch.fft.fft2 %.2f, block transposed / torch.fft.ifft2 %.2f, block forward / copy %.2f, torch.fft.fft2 / copy %.2f; "
              "|block - torch.fft| / |x| = %.2g (bound %.2g); device bytes of the block %.2f MB (table %d B, work buffer %.2f MB), a dense twin would hold %.3g values = %.3g GB"
              % (size, name, med["block forward"] / med["torch.fft.fft2"], med["block transposed"] / med["torch.fft.ifft2"], med["block forward"] / med["copy"],
                 med["torch.fft.fft2"] / med["copy"], err, R.bound(nx, ny, dtype), (2 * size + 2 * N) * item / 1e6, 2 * size * item, 2 * N * item / 1e6,
                 float(2 * N) ** 2, float(2 * N) ** 2 * item / 1e9), flush=True)
        for v in (d_x, d_r, d_w, d_t):
            v.free()
        del z, a, b, c
