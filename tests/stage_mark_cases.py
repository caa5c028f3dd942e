"""Shared cases of the stage-mark tests (tests/test_stage_marks_hostsim.py on the host simulation,
tests/test_stage_marks_gpu.py on the device): which stages Verifier.last_timings reports above zero after each call
shape.  bench.py's per-kernel roofline reads these marks by name, so a stage that loses its mark, or a launch that
lands under another stage's, silently corrupts a reported number.

Every case asserts the exact set: the stages listed are > 0, every other stage is exactly 0.0.  The sets are read from
the driver (csrc/lcv_driver.inc: run_bls, validate_impl).  Rows are the deduplication tests' six
(dedup_cases.basic_rows) and their four-store table batch; the sliced pipeline needs the 300 rows of
tests/test_pipeline_hostsim.py::test_slices_match_serial, generated once.
"""
import dedup_cases as D
import store_serving_cases as SV
import store_table_cases as T

# the two-stream schedule on the fan engine (latency mode: both line walks are inside the fused Miller program) ...
FAN = {"nsc_htr", "pre_checks", "sig_decode", "g1_aggregate", "signing_root", "h2c_sswu", "hash_to_g2", "miller_loop",
       "final_exp", "verdict"}
# ... and on the batch engine, where each walk is a launch of its own
BATCH = FAN | {"miller_lines", "miller_lines_sig"}
FOLD = {"store_rank", "store_fold"}
# a sliced chain has no marks of its own (concurrent kernels would inflate each other's event times), but it ends
# with the Miller accumulation and the final exponentiation every pairing check shares, which carry theirs
SLICED = {"nsc_htr", "miller_loop", "final_exp"}

_cache = {}


def check_marks(v, want):
    t = v.last_timings()
    assert set(want) <= set(t), sorted(set(want) - set(t))
    assert {k for k, ms in t.items() if ms > 0} == set(want), {k: ms for k, ms in t.items() if ms != 0}
    assert all(t[k] == 0.0 for k in t if k not in want)


def check_one_update(v):
    """One update under lcv_init's latency mode (64 rows): the fan engine."""
    case, upd = D.base(v)
    with D.latency(v, 64):
        v.validate(T.take(upd, [0]), case["current_slot"], case["gvr"])
    check_marks(v, FAN)


def check_six_rows_batch_engine(v):
    case, p = D.basic_rows(v)
    with D.latency(v, 0):
        v.validate(p, case["current_slot"], case["gvr"])
    check_marks(v, BATCH)


def check_fold(v, latency_rows):
    """validate_fold and validate_stores_fold: their engine's set, plus the rank records and the fold."""
    from lcv.device import FoldState
    engine = FAN if latency_rows else BATCH
    case, q = D.basic_rows(v)
    cs, gvr = case["current_slot"], case["gvr"]
    with D.latency(v, latency_rows):
        v.validate_fold(q, cs, gvr, FoldState())
        check_marks(v, engine | FOLD)
        case, p, index = D.table_case(v, True)
        v.validate_stores_fold(p, index, cs, gvr, [FoldState() for _ in range(4)])
        check_marks(v, engine | FOLD)


def check_dedup(v, latency_rows):
    """The six rows hold three distinct items: the gather joins the engine's set."""
    case, p = D.basic_rows(v)
    with D.latency(v, latency_rows), D.dedup(v, True):
        v.validate(p, case["current_slot"], case["gvr"])
        assert v.last_dedup() == (6, 3)
    check_marks(v, (FAN if latency_rows else BATCH) | {"dedup_gather"})


def _three_hundred(v):
    key = ("rows300", SV.is_hostsim(v))
    if key not in _cache:
        from lcv import synth
        n = 300  # 2 slices of whole waves (192 + 108)
        _cache[key] = synth.generate(v, n, seed=9, participation="random",
                                     kinds=synth.adversarial_kinds(n, seed=9, bad_fraction=0.2))
    return _cache[key]


def check_sliced_pipeline(v):
    """set_pipeline(2, 2) on 300 rows, without and with a fold (F_rank runs unmarked inside the chains)."""
    from lcv.device import FoldState
    sb = _three_hundred(v)
    v.set_store(sb.store_finalized_slot, sb.current.ssz, sb.next.ssz)
    with SV.pipeline(v, 2, 2):
        v.validate(sb.updates, sb.current_slot, sb.genesis_validators_root)
        check_marks(v, SLICED)
        v.validate_fold(sb.updates, sb.current_slot, sb.genesis_validators_root, FoldState())
        check_marks(v, SLICED | {"store_fold"})


def check_setup(v):
    """The committee build behind set_store_table and set_store.  lcv_set_store resets the timings but never collects
    them, so on the device, where a mark counts only once collected, it reports nothing; the host simulation adds
    a stage's time as its mark closes."""
    case, p, index = D.table_case(v, True)
    check_marks(v, {"setup"})
    c = T.committees(v)
    v.set_store(case["stores"][0][0], c[0].ssz, c[1].ssz)
    check_marks(v, {"setup"} if SV.is_hostsim(v) else set())
