"""CPU: tools/dedup_class_check.cpp — F_dedup_key and F_dedup_confirm run lane by lane on their host path over heap
buffers of exactly the column, key, pair and flag sizes (LDS pre-filled with garbage), with the host's grouping between
them, against dedup_classes; and every device, pinned and early host allocation of lcv_batch_classify and
lcv_batch_fan_out failing once — under AddressSanitizer, LeakSanitizer and UndefinedBehaviorSanitizer.  A stand-alone
program: nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

import helpers as H

PKG = os.path.join(H.ROOT, "light-client-consensus-specs_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_dedup_class_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dedup_class_check")
    H.ensure_hostsim()  # (build/lcv_build_id.h, which the host simulation includes)
    # (the sanitizer runtimes linked statically and the failing operator new in front of theirs, as in
    # test_driver_alloc_check_cpu.py)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread", "-fopenmp", "-DLCV_ALLOC_CHECK",
                           "-Wl,--wrap=_Znwm", "-Wl,--wrap=_Znam", "-I", os.path.join(PKG, "build"),
                           os.path.join(H.ROOT, "tools", "dedup_class_check.cpp"),
                           os.path.join(PKG, "csrc", "lcv_wire.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "dedup_class_check: functors: 804 batches" in r.stdout, r.stdout[-2000:]
    assert "dedup_class_check: 3 scenarios" in r.stdout and " 0 failures" in r.stdout, r.stdout[-2000:]
