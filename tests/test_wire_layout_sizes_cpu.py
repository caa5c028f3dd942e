"""CPU: the sizes csrc/lcv_wire_layout.hpp derives from its tables, printed by the stand-alone g++ program
tools/wire_layout_sizes.cpp, against literals written here (the SSZ sizes of the containers of sync-protocol.md and the
driver's encode pitch), and lcv_encode_pitch of the library.  Nothing is loaded into this interpreter but the library
the rest of the suite uses."""
import os
import subprocess

import helpers as H

CSRC = os.path.join(H.ROOT, "light-client-consensus-specs_amd", "csrc")

HEADER_MAX = {"deneb": 244 + 584 + 32, "capella": 244 + 568 + 32}
EXPECTED = {
    "exec_fixed_deneb": 584, "exec_fixed_capella": 568, "exec_offset_pos": 436, "exec_extra_rec": 320,
    "exec_extralen_rec": 800, "header_fixed": 244, "header_offset_pos": 112, "committee_off": 4,
    "committee_off_altair": 112, "bootstrap_fixed": 24788, "bootstrap_fixed_altair": 24896,
    "fixed_update": 25152, "fixed_finality": 368, "fixed_optimistic": 172,
    "fixed_update_altair": 25368, "fixed_finality_altair": 584, "fixed_optimistic_altair": 280,
    "second_offset_pos_update": 4 + 24624 + 160, "second_offset_pos_finality": 4, "second_offset_pos_optimistic": 0,
    "max_update_deneb": 25152 + 2 * HEADER_MAX["deneb"], "max_update_capella": 25152 + 2 * HEADER_MAX["capella"],
    "max_update_altair": 25368,
    "max_finality_deneb": 368 + 2 * HEADER_MAX["deneb"], "max_finality_capella": 368 + 2 * HEADER_MAX["capella"],
    "max_finality_altair": 584,
    "max_optimistic_deneb": 172 + HEADER_MAX["deneb"], "max_optimistic_capella": 172 + HEADER_MAX["capella"],
    "max_optimistic_altair": 280,
    "pitch_update": 26880, "pitch_finality": 2096, "pitch_optimistic": 1040, "image_bytes": 2272, "max_extra": 32,
    "kind_ok": "01100", "fork_ok": "01100",
}


def test_derived_sizes(tmp_path):
    exe = str(tmp_path / "wire_layout_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(H.ROOT, "tools", "wire_layout_sizes.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    got = dict(line.split() for line in out.splitlines())
    assert got == {k: str(v) for k, v in EXPECTED.items()}


def test_encode_pitch_of_the_library(sim_verifier):
    assert [sim_verifier.encode_pitch(k) for k in ("update", "finality", "optimistic")] == [26880, 2096, 1040]
    assert sim_verifier.lib.lcv_encode_pitch(3) == 0 and sim_verifier.lib.lcv_encode_pitch(-1) == 0
