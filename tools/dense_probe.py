"""Dense block kernels at the C ABI: time, compulsory bytes and fraction of the 8 TB/s HBM peak of kron(K, I_d), kron(I_d, K) for a
small dense K and of the dense matrix-vector product -- and, in the same process, the same product through what a user had before:
sparse_kron_id / id_kron_sparse of the sparsified K, and the CSR product of block.sparse(A).
Compulsory bytes: the operand once, the result once (twice when accumulating), K once.
usage: dense_probe.py [log2 of d, default 22; a K whose vectors do not fit at that d runs at 2^20]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

from prost_amd import _hip as hip

PEAK_GBS = 8000.0
sz = C.c_size_t


def main(logd=22):
    hip.require_device()
    L_ = hip.lib()
    L_.prost_hip_dense_gemv_workspace_bytes.restype = C.c_size_t
    L_.prost_hip_dense_gemv_workspace_bytes.argtypes = [C.c_size_t, C.c_size_t]
    rng = np.random.default_rng(3)
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        hip.check(L_.prost_hip_event_create(C.byref(e)))

    def timeit(run):
        """3 warm-up calls, then enough calls for a window of about 0.2 s (at least 10), timed by device events"""
        for _ in range(3):
            run()
        hip.sync()

        def window(iters):
            hip.check(L_.prost_hip_event_record(ev[0], None))
            for _ in range(iters):
                run()
            hip.check(L_.prost_hip_event_record(ev[1], None)); hip.check(L_.prost_hip_event_synchronize(ev[1]))
            ms = C.c_float(); hip.check(L_.prost_hip_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
            return ms.value / iters
        first = window(5)
        return window(int(min(2000, max(10, 200.0 / max(first, 1e-3)))))

    def line(tag, t, mb, t_sparse):
        print("%-58s %9.4f ms %9.1f MB %7.0f GB/s frac %.3f | sparse route %9.4f ms (x%.2f)" % (
            tag, t, mb, mb / t, mb / t / PEAK_GBS, t_sparse, t_sparse / t), flush=True)

    for dt, name in ((np.float32, "f32"), (np.float64, "f64")):
        item = np.dtype(dt).itemsize
        for (m, n) in ((3, 3), (8, 8), (16, 32), (32, 32), (64, 64)):
            d = 1 << logd
            if (m + n) * d * item > (6 << 30):          # the two vectors past 6 GB: the smaller identity
                d = 1 << min(logd, 20)
            K = rng.standard_normal((m, n))
            dK = hip.DeviceArray.from_host(np.asfortranarray(K).ravel(order="F").astype(dt))
            for id_first, op, twin in ((False, "dense_kron_id", "sparse_kron_id"), (True, "id_kron_dense", "id_kron_sparse")):
                for transpose in (0, 1):
                    S = sp.csr_matrix(K.T if transpose else K)
                    rows, inner = S.shape
                    sv, sp_, si = (hip.DeviceArray.from_host(S.data.astype(np.float32)), hip.DeviceArray.from_host(S.indptr.astype(np.int32)),
                                   hip.DeviceArray.from_host(S.indices.astype(np.int32)))
                    x = hip.DeviceArray.from_host(rng.standard_normal(inner * d).astype(dt)); r = hip.DeviceArray.zeros(rows * d, dt)
                    for acc in (False, True):
                        fn = getattr(L_, "prost_hip_%s%s_%s" % (op, "_acc" if acc else "", name))
                        fs = getattr(L_, "prost_hip_%s%s_%s" % (twin, "_acc" if acc else "", name))
                        t = timeit(lambda: hip.check(fn(r.ptr, x.ptr, sz(d), sz(m), sz(n), dK.ptr, C.c_int(transpose), None)))
                        if id_first:
                            ts = timeit(lambda: hip.check(fs(r.ptr, x.ptr, sz(d), sz(rows), sz(inner), sv.ptr, sp_.ptr, si.ptr, None)))
                        else:
                            ts = timeit(lambda: hip.check(fs(r.ptr, x.ptr, sz(d), sz(rows), sv.ptr, sp_.ptr, si.ptr, None)))
                        mb = ((inner + rows * (2 if acc else 1)) * d + m * n) * item / 1e6
                        line("%s %-13s %s %s K %2d x %2d d 2^%d" % (name, op, "adj" if transpose else "fwd", "acc" if acc else "   ", m, n, int(np.log2(d))), t, mb, ts)
                    del x, r
        for (m, n) in ((4096, 4096), (64, 1 << 20), (1 << 20, 64)):
            A = rng.standard_normal((m, n)).astype(dt)
            dA = hip.DeviceArray.from_host(np.asfortranarray(A).ravel(order="F"))
            nbytes = int(L_.prost_hip_dense_gemv_workspace_bytes(m, n))
            ws = hip.DeviceArray.zeros(max(nbytes // 8, 2), np.float64)
            for transpose in (0, 1):
                S = sp.csr_matrix(A.T if transpose else A)          # what block.sparse(A) applies: CSR of A, CSR of A^T
                rows, inner = S.shape
                sv, sp_, si = (hip.DeviceArray.from_host(S.data.astype(dt)), hip.DeviceArray.from_host(S.indptr.astype(np.int32)),
                               hip.DeviceArray.from_host(S.indices.astype(np.int32)))
                x = hip.DeviceArray.from_host(rng.standard_normal(inner).astype(dt)); r = hip.DeviceArray.zeros(rows, dt)
                for acc in (False, True):
                    fn = getattr(L_, "prost_hip_dense_gemv%s_%s" % ("_acc" if acc else "", name))
                    fs = getattr(L_, "prost_hip_csr_spmv%s_%s" % ("_acc" if acc else "", name))
                    t = timeit(lambda: hip.check(fn(r.ptr, x.ptr, sz(m), sz(n), dA.ptr, C.c_int(transpose), ws.ptr, None)))
                    ts = timeit(lambda: hip.check(fs(r.ptr, x.ptr, sz(rows), sz(S.nnz), sv.ptr, sp_.ptr, si.ptr, None)))
                    mb = (inner + rows * (2 if acc else 1) + m * n) * item / 1e6
                    line("%s dense_gemv    %s %s A %d x %d" % (name, "adj" if transpose else "fwd", "acc" if acc else "   ", m, n), t, mb, ts)
                del sv, sp_, si, S
            del dA, A


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 22)
