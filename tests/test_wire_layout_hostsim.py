"""CPU: every ExecutionPayloadHeader field of oracle-serialised messages lands where include/lcv.h says, through the
host decoder (csrc/lcv_wire.cpp) and the host simulation of the device decoder and encoder.  The same checks run on the
MI355X in test_wire_layout_gpu.py; both live in wire_layout_cases.py."""
import pytest

import wire_layout_cases as WL


@pytest.mark.parametrize("fork", WL.FORKS)
@pytest.mark.parametrize("kind", WL.KINDS)
def test_fields(sim_verifier, kind, fork):
    WL.check_fields(sim_verifier, kind, fork)
