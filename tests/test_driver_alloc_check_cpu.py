"""CPU: tools/driver_alloc_check.cpp — the driver's memory handling on the host simulation, under AddressSanitizer,
LeakSanitizer and UndefinedBehaviorSanitizer: every device or pinned allocation of every scenario fails once (the call
returns LCV_ENOMEM, the same call then succeeds with a fresh context's outputs), the host allocations ahead of the first
device allocation of lcv_set_store_table and lcv_fast_aggregate_verify fail once each (LCV_ENOMEM, no exception leaves
the library), and nothing is live after lcv_destroy.  A stand-alone program: nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

import helpers as H

PKG = os.path.join(H.ROOT, "light-client-consensus-specs_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_driver_alloc_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "driver_alloc_check")
    # (the sanitizer runtimes linked statically, as in test_wire_dec_check_cpu.py; they define operator new themselves,
    # so the program's failing operator new is put in front of theirs with --wrap)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread", "-fopenmp", "-DLCV_ALLOC_CHECK",
                           "-Wl,--wrap=_Znwm", "-Wl,--wrap=_Znam", "-I", os.path.join(PKG, "build"),
                           os.path.join(H.ROOT, "tools", "driver_alloc_check.cpp"),
                           os.path.join(PKG, "csrc", "lcv_wire.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "driver_alloc_check: 21 scenarios" in r.stdout, r.stdout[-2000:]
