"""CPU: tools/wire_dec_check.cpp — the device SSZ decoder's three functors run lane by lane on their host path over
heap buffers of exactly the staged, LDS and column sizes, under AddressSanitizer and UndefinedBehaviorSanitizer, on
the malformed table and on seeded mutations of good messages, compared with the host decoder.  A stand-alone program:
nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

import helpers as H

CSRC = os.path.join(H.ROOT, "light-client-consensus-specs_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_wire_dec_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wire_dec_check")
    # (the sanitizer runtimes linked statically: the program then runs wherever the suite does, whatever else the
    # environment loads into every process)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-pthread", "-DLCV_HOSTSIM=1", "-I", CSRC,
                           os.path.join(H.ROOT, "tools", "wire_dec_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "wire_dec_check:" in r.stdout, r.stdout[-2000:]
