"""CPU: upload -> download of a batch whose bytes name their place, on the host simulation
(batch_roundtrip_cases.py; the same checks run on the MI355X in test_batch_roundtrip_gpu.py)."""
import batch_roundtrip_cases as BR


def test_roundtrip(sim_verifier):
    BR.check_roundtrip(sim_verifier)


def test_roundtrip_with_store_index(sim_verifier):
    BR.check_roundtrip(sim_verifier, store_index=BR.STORE_INDEX)
