"""The host twins of the NORM_NACK / REPAIR_ADV message calls (norm_amd/csrc/ctl_msg_host.cpp,
ctl_msg.hpp) on the host under AddressSanitizer + UBSan, every content buffer, wire buffer and
datagram in an allocation of exactly its length (tests/native/ctl_msg_asan.cpp).  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None,
                    reason="needs hipcc (host compile only)")
def test_control_message_twins_clean_under_asan():
    b = subprocess.run(["make", "-s", "-C", NATIVE, "-f", "ctl_msg_asan.mk"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(NATIVE, "_build", "ctl_msg_asan")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.rstrip().endswith("control message driver done")
