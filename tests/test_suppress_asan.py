"""NACK suppression and repair advertisements on the host (norm_amd/csrc/suppress_host.cpp and
nack_host.cpp over suppress_layout.hpp: what nfec_rx_handle_repair_content_host,
nfec_rx_repair_pending_host and nfec_tx_repair_adv_host run) under AddressSanitizer + UBSan, every byte
a call may not touch poisoned (tests/native/suppress_asan.cpp).  A stand-alone program; nothing is
loaded into Python.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="needs hipcc (host compile only)")
def test_suppress_host_clean_under_asan():
    b = subprocess.run(["make", "-s", "-C", NATIVE, "-f", "suppress_asan.mk"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(NATIVE, "_build", "suppress_asan")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("suppress driver done")
