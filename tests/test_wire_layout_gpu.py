"""MI355X: every ExecutionPayloadHeader field of oracle-serialised messages lands where include/lcv.h says, through the
host decoder of liblcv.so and its F_wire_dec and F_wire_enc kernels: the checks of wire_layout_cases.py, which
test_wire_layout_hostsim.py runs on the host simulation of the same code."""
import pytest

import wire_layout_cases as WL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fork", WL.FORKS)
@pytest.mark.parametrize("kind", WL.KINDS)
def test_fields_gpu(gpu_verifier, kind, fork):
    WL.check_fields(gpu_verifier, kind, fork)
