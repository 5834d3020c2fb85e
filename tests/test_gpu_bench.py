"""bench.py as the driver invokes it, for every BASELINE config it measures (c2 headline, c3, c4), at reduced sizes: the ONE JSON
line with the contract's keys, a `roofline` object whose kernel time was measured with HIP events inside the timed region, with
--full a `cpu_baseline` object from the oracle, the native path (no fallback) -- so that a schema or plumbing error does not wait for
the round-end run.  The bench process is started from the fork server (a process that has touched the GPU must not spawn)."""
import json
import multiprocessing as mp
import os
import sys

import pytest

import multirank_workers as workers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                 "roofline", "cpu_baseline")


def _bench(*argv):
    ctx = mp.get_context("forkserver")
    out = ctx.Queue()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + list(argv)
    p = ctx.Process(target=workers.run_command, args=(cmd, {"HSA_ENABLE_IPC_MODE_LEGACY": "0"}, ROOT, out))
    p.start()
    rc, stdout, stderr = out.get(timeout=900)
    p.join(timeout=60)
    assert rc == 0, stderr
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def _check_contract(d, steps, warmup, dtype="f32"):
    for k in CONTRACT_KEYS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["unit"] == "it/s" and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == dtype and d["data"] == "synthetic"
    assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"] and d["iterates_finite"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and r["avg_launch_ms"] > 0
    # a short run stamps EVERY launch: at least 8 samples of the dominant kernel behind the fraction (round-3 review, weak #9)
    assert r["sample_every"] == 1 and r["launches_timed"] >= 8, r["launches_timed"]
    # frac = compulsory bytes of the kernel that ran / time / peak: a fraction
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] <= 1 and "traffic" in r
    assert abs(r["achieved"] - r["compulsory_bytes_per_launch"] / 1e9 / (r["avg_launch_ms"] * 1e-3)) <= 1e-9 * r["achieved"]
    if r["algorithmic_bytes_per_launch"]:
        assert abs(r["algorithmic_equiv_frac"] - r["algorithmic_bytes_per_launch"] / 1e9 / (r["avg_launch_ms"] * 1e-3) / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] == "port" and c["sample"]
    assert "workload" in d["config"] and "model" not in d["config"]


def test_bench_c2_reduced():
    d = _bench("--steps", "20", "--warmup", "5", "--size", "512", "--prelude-iters", "50", "--full")
    _check_contract(d, 20, 5)
    assert d["config"]["name"] == "c2" and d["config"]["path"] == "pdhg:fused-grad2d" and d["metric"] == "PDHG iters/sec, ROF-TV 512^2 fp32"
    assert d["roofline"]["kernel"].startswith("fused_iter2d") and d["roofline"]["algorithmic_bytes_per_launch"] in (11 * 4 * 512 * 512, 22 * 4 * 512 * 512)
    assert d["roofline"]["compulsory_bytes_per_launch"] == 7 * 4 * 512 * 512 and d["roofline"]["iterations_per_launch"] == 2
    assert d["config"]["stepsize"] == "alg2" and d["config"]["residual_iter"] == 10
    # the tolerance-class leg beside the exact one (round 6): same problem, same loop, K iterations per launch
    assert d["value_fmad"] > 0 and d["fmad"]["arithmetic"] == "fmad" and d["fmad"]["path"] == "pdhg:fused-grad2d+fmad" and d["fmad"]["iterates_finite"]
    rf = d["roofline_fmad"]
    assert rf["kernel"].startswith("fused_iter2d_xk_kernel<") and rf["compulsory_bytes_per_launch"] == 7 * 4 * 512 * 512 and 0 < rf["frac"] <= 1
    assert any(k.endswith("+residuals") for k in rf["all_kernels"]) and "two_pass_equiv_GBps" in d and "achieved_hbm_GBps" not in d


def test_bench_plain_run_and_its_dumped_outputs(tmp_path):
    """a plain run (no --full) measures the headline alone: no bare-loop rate, no tolerance-class leg, no CPU baseline.  With
    --dump-outputs it writes x, y, z, w as the timed loop left them, fp32 -- bit for bit the CPU oracle's iterates after the same
    prelude + warm-up + timed iterations (exact class)"""
    import numpy as np

    import oracle
    import prost_amd as prost
    from prost_amd import synthetic
    out = tmp_path / "outputs"
    d = _bench("--steps", "20", "--warmup", "5", "--size", "64", "--prelude-iters", "10", "--dump-outputs", str(out))
    for k in CONTRACT_KEYS[:-1]:
        assert k in d, k
    assert d["steps"] == 20 and d["warmup"] == 5 and d["dtype"] == "f32" and d["higher_is_better"] is True and d["iterates_finite"]
    assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"] and d["config"]["path"] == "pdhg:fused-grad2d"
    for k in ("cpu_baseline", "value_fmad", "roofline_fmad", "fmad", "iterate_only_it_per_s"):
        assert k not in d, k
    prob = synthetic.rof_problem(64, 64, lmb=10.0, seed=42)[0]
    prob.finalize()
    b = prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5)
    o = prost.options(max_iters=10 ** 9, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    orc = oracle.Solver(prob.data, prob.nrows, prob.ncols, b, o, np.float32)
    orc.initialize()
    orc.iterate(10 + 5 + 20)
    ost = orc.state()
    assert sorted(os.listdir(out)) == ["w.npy", "x.npy", "y.npy", "z.npy"]
    for v in "xyzw":
        got = np.load(out / (v + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, np.asarray(ost[v], dtype=np.float32)), v


def test_bench_c2_reduced_fp64_and_the_reference_default_options():
    """--dtype f64 (the precision the reference front end ships with, config.hpp:7) and --stepsize boyd --residual-iter 1 (the
    reference's DEFAULT backend options, pdhg.m:4-14) keep the schema"""
    d = _bench("--steps", "20", "--warmup", "5", "--size", "512", "--prelude-iters", "50", "--dtype", "f64", "--full")
    _check_contract(d, 20, 5, "f64")
    assert d["metric"] == "PDHG iters/sec, ROF-TV 512^2 fp64" and d["roofline"]["compulsory_bytes_per_launch"] == 7 * 8 * 512 * 512
    d = _bench("--steps", "40", "--warmup", "5", "--size", "512", "--prelude-iters", "50", "--stepsize", "boyd", "--residual-iter", "1", "--no-cpu-baseline")
    assert d["config"]["stepsize"] == "boyd" and d["config"]["residual_iter"] == 1 and d["value"] > 0 and 0 < d["roofline"]["frac"] <= 1
    assert "PDHG boyd, residual_iter=1" in d["config"]["workload"]


def test_bench_c3_reduced():
    d = _bench("--config", "c3", "--steps", "20", "--warmup", "5", "--volume", "96", "64", "8", "--prelude-iters", "20", "--full")
    _check_contract(d, 20, 5)
    assert d["config"]["name"] == "c3" and d["config"]["path"] == "pdhg:fused-grad3d" and d["metric"] == "PDHG iters/sec, TV-3D 96x64x8 fp32"
    vox = 96 * 64 * 8
    assert d["roofline"]["kernel"].startswith("fused_iter3d") and d["roofline"]["algorithmic_bytes_per_launch"] in (14 * 4 * vox, 28 * 4 * vox)
    assert d["roofline"]["compulsory_bytes_per_launch"] in (9 * 4 * vox, 13 * 4 * vox)
    assert abs(d["two_pass_equiv_GBps"] - d["value"] * 14 * 4 * vox / 1e9) <= 1e-9 * d["two_pass_equiv_GBps"]
    assert d["cpu_baseline"]["voxel_iterations_per_s"] > 0


def bench_module():
    import importlib
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    return importlib.import_module("bench")


def test_bench_c4_reduced():
    d = _bench("--config", "c4", "--steps", "20", "--warmup", "5", "--size", "128", "--prelude-iters", "10", "--full")
    _check_contract(d, 20, 5)
    assert d["config"]["name"] == "c4" and d["config"]["path"] == "admm:pixel-op" and d["metric"] == "ADMM iters/sec, TV-L1 flow-like 128^2 fp32"
    r = d["roofline"]
    assert set(r["all_kernels"]) == {"cg_pixel_pq_kernel", "cg_pixel_xrs_kernel"}      # the two-launch CG round ran
    px = 128 * 128
    assert r["compulsory_bytes_per_iteration"] == bench_module().c4_iteration_bytes("admm:pixel-op", d["cg_iterations_last_solve"], px) and 0 < r["frac_iteration"] <= 1
    assert r["kernel"] in r["all_kernels"] and r["compulsory_bytes_per_launch"] == r["all_kernels"][r["kernel"]]["compulsory_bytes"]
    assert d["two_pass_equiv_GBps"] is None and d["cg_iterations_last_solve"] >= 1
    assert d["oracle_pin"].startswith("unpinned")


def test_bench_c4w_reduced():
    """BASELINE.json configs[3] as worded (warp matrix): the two-launch CG rounds with the rows of W gathered (round 6; four launches before)"""
    d = _bench("--config", "c4w", "--steps", "20", "--warmup", "5", "--size", "128", "--prelude-iters", "10", "--full")
    _check_contract(d, 20, 5)
    assert d["config"]["name"] == "c4w" and d["config"]["path"] == "admm:pixel-op" and "warp matrix" in d["config"]["workload"]
    r = d["roofline"]
    assert set(r["all_kernels"]) == {"cg_pixel_pq_kernel", "cg_pixel_xrs_kernel"}
    px = 128 * 128
    bm = bench_module()
    assert r["compulsory_bytes_per_iteration"] == bm.c4_iteration_bytes("admm:pixel-op", d["cg_iterations_last_solve"], px, 4, 4) and 0 < r["frac_iteration"] <= 1
    # launch A: W's 4 values + 4 column indices + 1 row start per pixel instead of the 2 values of a pixel-diagonal W
    assert bm.c4_kernel_bytes("cg_pixel_pq_kernel", px, 4, 4) == bm.c4_kernel_bytes("cg_pixel_pq_kernel", px, 4, 2) + (2 * 4 + 5 * 4) * px
    # 4 non-zeros per row: two more values and two more column indices per pixel than C4's W in every stage that applies it
    assert bm.c4_kernel_bytes("op_stage_kernel<EpiFwdQ>", px, 4, 4) == bm.c4_kernel_bytes("op_stage_kernel<EpiFwdQ>", px, 4, 2) + 16 * px
    assert d["oracle_pin"].startswith("unpinned")
