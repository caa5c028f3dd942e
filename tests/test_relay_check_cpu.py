"""CPU: tools/relay_check.cpp — the asynchronous relay's decode functor (F_wire_relay) run lane by lane on its host path
over heap buffers of exactly the staged, LDS, meta, map and column sizes, under AddressSanitizer and
UndefinedBehaviorSanitizer, on the malformed table, seeded mutations and random pair lists, compared with the host
decoder's rows gathered by the map; and every device, pinned and early host allocation of lcv_relay_async failing once
(tools/driver_alloc_harness.hpp).  A stand-alone program: nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

import helpers as H

PKG = os.path.join(H.ROOT, "light-client-consensus-specs_amd")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_relay_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "relay_check")
    # (built as test_wire_dec_check_cpu.py builds its program — the sanitizer runtimes linked statically — with what the
    # allocation harness needs on top, as in test_driver_alloc_check_cpu.py)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread", "-fopenmp", "-DLCV_ALLOC_CHECK",
                           "-Wl,--wrap=_Znwm", "-Wl,--wrap=_Znam", "-I", os.path.join(PKG, "build"),
                           os.path.join(H.ROOT, "tools", "relay_check.cpp"),
                           os.path.join(PKG, "csrc", "lcv_wire.cpp"), "-o", exe])
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "relay_check:" in r.stdout and "2 scenarios" in r.stdout, r.stdout[-2000:]
