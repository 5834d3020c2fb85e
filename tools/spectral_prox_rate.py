"""Throughput of the spectral prox kernel (prost_amd/csrc/kernels_prox_spectral.hip) against the in-tree elem_operation:norm2:abs
prox at the same dim and count, which moves the same bytes: arg + res (dim values per group each) + tau_diag[first component].
count = 2^22 groups, fp32, both layouts; 2x2 = eigen_2x2 (dim 4), 3x2 = singular_nx2 (dim 6), 3x3 = eigen_3x3 (dim 9).
eval_prox times ONE synchronous launch with a host clock (enqueue + wait: the launch latency is inside), best of `reps`; for
kernel times run this script under `rocprofv3 --kernel-trace --stats`.
usage: python tools/spectral_prox_rate.py [log2_count] [reps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import prost_amd as prost  # noqa: E402

log2_count = int(sys.argv[1]) if len(sys.argv) > 1 else 22
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
prost.set_gpu(0)
prost.set_precision("single")
rng = np.random.default_rng(1)
count = 1 << log2_count
cs = (1, 0, 1, 0, 0, 0, 0)
for label, dim, make in (("2x2 eigen_2x2", 4, lambda il: prost.function.sum_eigen_2x2(il, "abs", *cs)),
                         ("3x2 singular_nx2", 6, lambda il: prost.function.sum_singular_nx2(6, il, "sum_1d:abs", *cs)),
                         ("3x3 eigen_3x3", 9, lambda il: prost.function.sum_eigen_3x3(il, "abs", *cs))):
    n = count * dim
    arg = rng.standard_normal(n) * 10
    Tau = np.ones(n)
    nbytes = count * (2 * dim + 1) * 4
    for il in (False, True):
        t_new = min(prost.eval_prox(make(il), arg, 0.4, Tau)[1] for _ in range(reps))
        t_ref = min(prost.eval_prox(prost.function.sum_norm2(dim, il, "abs", *cs), arg, 0.4, Tau)[1] for _ in range(reps))
        print("%s dim %d %s count 2^%d: spectral %.3f ms %.2f TB/s | norm2:abs %.3f ms %.2f TB/s | ratio %.2f" % (
            label, dim, "interleaved" if il else "planar", log2_count, t_new, nbytes / t_new / 1e9, t_ref, nbytes / t_ref / 1e9, t_new / t_ref), flush=True)
