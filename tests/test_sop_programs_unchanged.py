"""CPU: adding the f12mul program (batch verification's group product) to tools/gen_sop.py left the five existing SOP
programs as they were.  tests/golden/sop_programs_sha256.json holds the SHA-256 of each program's block of the
generated csrc/lcv_sop_programs.inc (its stats comment, #defines and the three arrays) as the generator emitted them
before f12mul existed; the blocks of the file the build generates must hash to the same values, and the closing
LCV_SOP_SCHOOLBOOK flag must be unchanged.  gen_sop.py --check covers f12mul's arithmetic against the oracle's
f12_mul; here its block must be present."""
import hashlib
import json
import os
import subprocess
import sys

import helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sop_programs_sha256.json")
INC = os.path.join(H.PKG, "csrc", "lcv_sop_programs.inc")


def blocks(text):
    """{program name: its block of the generated file}, and the tail after the last program."""
    out, name, cur, tail = {}, None, [], []
    for line in text.splitlines():
        if line.startswith("// 1: some product round"):
            if name:
                out[name] = "\n".join(cur)
            name, cur = None, []
            tail.append(line)
        elif tail:
            tail.append(line)
        elif line.startswith("// ") and ": team " in line:
            if name:
                out[name] = "\n".join(cur)
            name, cur = line[3:].split(":")[0], [line]
        elif name:
            cur.append(line)
    return out, "\n".join(tail)


def test_existing_programs_unchanged(tmp_path):
    want = json.load(open(GOLDEN))
    path = str(tmp_path / "sop.inc")
    subprocess.check_call([sys.executable, os.path.join(H.ROOT, "tools", "gen_sop.py"), "--out", path],
                          stdout=subprocess.DEVNULL)
    fresh = open(path).read()
    got, tail = blocks(fresh)
    assert list(got)[:5] == ["lines", "miller_acc", "fexp", "h2c", "miller"] and "f12mul" in got
    for name, digest in want["programs"].items():
        assert hashlib.sha256(got[name].encode()).hexdigest() == digest, name
    assert hashlib.sha256(tail.encode()).hexdigest() == want["tail"]
    if os.path.exists(INC):  # the file the library was built from is the generator's output
        assert open(INC).read() == fresh
