"""Rates of elem_operation:eigen_nxn:* (n = 4, 5: one matrix per lane, kernels_prox_spectral.hip; n >= 6: several lanes per matrix,
kernels_prox_eigen_nxn.hip) and of the four mass-norm operations, at about 2^24 values per operand, both layouts, both precisions.
eval_prox times ONE synchronous launch with a host clock (enqueue + wait: the launch latency is inside), best of `reps`; for kernel
times run this script under `rocprofv3 --kernel-trace --stats`.
usage: python tools/eigen_mass_rate.py [log2_values] [reps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import prost_amd as prost  # noqa: E402

log2_values = int(sys.argv[1]) if len(sys.argv) > 1 else 24
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
prost.set_gpu(0)
rng = np.random.default_rng(1)
cs = (1, 0, 1, 0, 0, 0, 0)
cases = [("eigen_nxn n=%d" % n, n * n, (lambda n: lambda il: prost.function.sum_eigen_nxn(n, il, "abs", *cs))(n)) for n in (4, 5, 6, 8, 16, 32)]
cases += [("mass4", 6, lambda il: prost.function.sum_mass_norm(4, il)), ("ind_comass4_ball", 6, lambda il: prost.function.sum_ind_comass_ball(4, il)),
          ("mass5", 10, lambda il: prost.function.sum_mass_norm(5, il)), ("ind_comass5_ball", 10, lambda il: prost.function.sum_ind_comass_ball(5, il))]
for precision, size in (("single", 4), ("double", 8)):
    prost.set_precision(precision)
    for label, dim, make in cases:
        count = (1 << log2_values) // dim
        arg = rng.standard_normal(count * dim) * 10
        Tau = np.ones(count * dim)
        nbytes = count * (2 * dim + 1) * size
        for il in (False, True):
            t = min(prost.eval_prox(make(il), arg, 0.4, Tau)[1] for _ in range(reps))
            print("%s %s %s: %d groups, %.3f ms per launch, %.3g groups/s, %.2f TB/s" % (
                label, precision, "interleaved" if il else "planar", count, t, count / t * 1e3, nbytes / t / 1e9), flush=True)
