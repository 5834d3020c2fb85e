"""Build and run one stand-alone host harness of tests/host/ (plain g++, its own main, no HIP) under AddressSanitizer and
UndefinedBehaviorSanitizer.  A plain module, shared by the tests/test_*_host.py files and tests/test_linop_product_trace.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include")]


def sanitizer_env():
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def run_sanitized(name, build_dir, args=(), extra_flags=()):
    """Compiles tests/host/<name>.cpp into <build_dir>/<name>, runs it with `args` and returns its stdout.  Skips without g++; a
    failed build, a non-zero exit status or a sanitizer report in stderr fail the calling test."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "host", name + ".cpp")
    exe = os.path.join(str(build_dir), name)
    b = subprocess.run(["g++"] + FLAGS + list(extra_flags) + [src, "-o", exe], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=sanitizer_env())
    print(r.stdout if len(r.stdout) < 200000 else r.stdout[-20000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout
