"""The per-segment walks of the stream pack and unpack kernels (norm_amd/csrc/kernels_stream.hip: the
rules of stream_layout.hpp and segment_copy.hpp) on the host under AddressSanitizer + UBSan, every
byte a call may not touch poisoned (tests/native/stream_copy_asan.cpp).  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="needs hipcc (host compile only)")
def test_stream_walks_clean_under_asan():
    b = subprocess.run(["make", "-s", "-C", NATIVE, "-f", "stream_copy_asan.mk"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(NATIVE, "_build", "stream_copy_asan")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("stream copy driver done")
