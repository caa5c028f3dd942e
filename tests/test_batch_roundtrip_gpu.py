"""MI355X: upload -> download of a batch whose bytes name their place, through liblcv.so
(batch_roundtrip_cases.py, the cases of test_batch_roundtrip_hostsim.py)."""
import pytest

import batch_roundtrip_cases as BR

pytestmark = pytest.mark.gpu


def test_roundtrip_gpu(gpu_verifier):
    BR.check_roundtrip(gpu_verifier)


def test_roundtrip_with_store_index_gpu(gpu_verifier):
    BR.check_roundtrip(gpu_verifier, store_index=BR.STORE_INDEX)
