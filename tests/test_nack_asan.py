"""The per-block walk of the repair requests and the parser of their content (norm_amd/csrc/
nack_layout.hpp: what nfec_rx_repair_requests_host and nfec_repair_parse_host run) on the host under
AddressSanitizer + UBSan, every byte a call may not touch poisoned (tests/native/nack_walk_asan.cpp).
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="needs hipcc (host compile only)")
def test_nack_walk_and_parser_clean_under_asan():
    b = subprocess.run(["make", "-s", "-C", NATIVE, "-f", "nack_walk_asan.mk"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(NATIVE, "_build", "nack_walk_asan")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("nack walk driver done")
