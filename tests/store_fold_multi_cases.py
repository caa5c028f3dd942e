"""Shared cases of the segmented store-fold tests (tests/test_store_fold_multi_hostsim.py on the host simulation,
tests/test_store_fold_multi_gpu.py on the device): one call validates a store-table batch and folds it per store
(include/lcv.h: lcv_validate_stores_fold, lcv_validate_stores_async_fold, lcv_slot_wait_stores_fold,
lcv_debug_fold_stores; lcv.store.fold_light_client_updates_multi).

Expected values never come from the code under test: the kernel's from store_fold_cases.model_fold (the sequential
loop) run on each store's subsequence with its row numbers mapped back to batch rows; the end-to-end runs' from the
committed fixture tests/golden/store_fold.npz and from lcv.store.process_light_client_updates per store."""
import ctypes
from functools import lru_cache

import numpy as np

import helpers as H
import store_cases
import store_fold_cases as SF
import store_table_cases as ST

STORE_FIN = SF.STORE_FIN
LENGTHS = (1, 2, 63, 64, 65, 512, 513, 577)  # stripe length 1 -> 2 at 65; FOLD_BLK = 8 block edges at L = 8 (512), 9 (513, 577)
SENTINEL = 0xA5


# ----------------------------------------------------------------------------- the kernel alone
def interleave(kind, stores, lens, rng):
    """store_index of a batch in which store stores[k] has lens[k] rows."""
    blocked = np.repeat(np.asarray(stores, np.uint32), lens)
    if kind == "blocked":
        return blocked
    if kind == "reversed":
        return np.repeat(np.asarray(stores[::-1], np.uint32), lens[::-1])
    if kind == "random":
        return rng.permutation(blocked)
    assert kind == "round-robin"
    left, out = list(lens), []
    while any(left):
        for k, s in enumerate(stores):
            if left[k]:
                left[k] -= 1
                out.append(s)
    return np.asarray(out, np.uint32)


def model(rec, ver, six, fin, nk, states):
    """Per store: model_fold over the store's rows in batch order, row numbers mapped back to batch rows; None for a
    store without a row."""
    from lcv.device import FoldResult
    out = []
    for s in range(len(states)):
        rows = np.flatnonzero(six == s)
        if rows.size == 0:
            out.append(None)
            continue
        e = SF.model_fold(rec[rows], ver[rows], int(fin[s]), int(nk[s]), states[s])
        back = lambda j: int(rows[j]) if j >= 0 else -1  # noqa: E731
        out.append(FoldResult(e.next, e.rows_consumed, back(e.apply_row), back(e.best_row), back(e.optimistic_row),
                              e.accepted_count))
    return out


def _state(rng, with_best):
    from lcv.device import FoldState
    st = FoldState(optimistic_slot=STORE_FIN + int(rng.integers(90, 103)),
                   previous_max_active_participants=int(rng.choice([0, 300, 512])),
                   current_max_active_participants=int(rng.choice([0, 1, 341, 512])))
    if with_best:
        st.has_best = True
        st.best_key0 = int(rng.choice([341 << 13 | 341, SF.SUPER | SF.FIN | 342, SF.SUPER | SF.REL_SC | 512]))
        st.best_attested_slot = STORE_FIN + 100 + int(rng.integers(0, 3))
        st.best_signature_slot = st.best_attested_slot + 1
    return st


@lru_cache(maxsize=None)
def kernel_cases():
    """[(name, records, verdicts, store_index, finalized slots, next_known, states, expected)] — built once, shared,
    never modified.  Asserts its own coverage."""
    from lcv.device import RANK_DTYPE
    cases = []

    def build(name, nstore, stores, lens, kind, seed, quiet=(), plants=(), fins=None, tie=()):
        """stores[k] has lens[k] rows; stores in `quiet` cannot apply; plants: (store, position in its segment,
        fin_next); tie: stores whose state's best ties their segment's best."""
        rng = np.random.default_rng(seed)
        six = interleave(kind, list(stores), list(lens), rng)
        n = six.size
        assert n == sum(lens) and n <= 4300
        rec, ver = np.zeros(n, RANK_DTYPE), np.zeros(n, np.uint8)
        nk = rng.integers(0, 2, nstore).astype(np.uint8)
        fin = np.full(nstore, STORE_FIN, np.uint64) if fins is None else np.asarray(fins, np.uint64)
        states = [_state(rng, bool((s + seed) % 2)) for s in range(nstore)]
        for s, pos, fin_next in plants:
            if fin_next:
                nk[s] = 0
        for s in stores:
            rows = np.flatnonzero(six == s)
            is_quiet = s in quiet or any(p[0] == s for p in plants)
            r, v = SF.make_records(rng, rows.size, is_quiet, int(nk[s])), (rng.random(rows.size) < 0.7).astype(np.uint8)
            for ps, pos, fin_next in plants:
                if ps == s:
                    SF.plant(r, v, pos, fin_next)
            if s in tie:
                v[0] = 1
                b = SF.model_fold(r, v, int(fin[s]), int(nk[s]), _state(rng, False)).next
                st = states[s]
                st.has_best, st.best_key0 = True, b.best_key0
                st.best_attested_slot, st.best_signature_slot = b.best_attested_slot, b.best_signature_slot
            rec[rows], ver[rows] = r, v
        cases.append((name, rec, ver, six, fin, nk, states, model(rec, ver, six, fin, nk, states)))

    # every segment length in one batch, each interleaving; 8 of 65 store rows present (the rest keep the sentinel),
    # finalized slots that differ (STORE_FIN + 10 is past every record's finalized slot: only the finalized-next
    # rule applies there)
    some = [0, 3, 7, 20, 33, 40, 63, 64]
    fins = [STORE_FIN + (10 if s % 3 == 1 else 0) for s in range(65)]
    for k, kind in enumerate(("round-robin", "blocked", "reversed", "random")):
        build(f"lengths-{kind}-nstore65", 65, some, LENGTHS, kind, 2000 + k, fins=fins)
    # one store: the one-store fold on the same rows (check_kernel_case compares with debug_fold too)
    for ln in LENGTHS:
        build(f"one-store-n{ln}", 1, [0], [ln], "blocked", 2100 + ln)
    # planted applying rows in store 0 — its segment's first row, last row, the first row of a stripe — with and
    # without the finalized-next rule, beside an interleaved store that cannot apply (and a third, anything goes)
    for ln in (65, 513, 577):
        stripe = -(-ln // 64)
        for j, (pos, what) in enumerate(((0, "first"), (ln - 1, "last"), (stripe * (ln // stripe // 2), "stripe"))):
            for fin_next in (False, True):
                nstore = 2 + (j + fin_next) % 2
                kind = ("round-robin", "random")[(j + ln) % 2]
                build(f"apply-{what}{'-finnext' if fin_next else ''}-n{ln}-nstore{nstore}", nstore, list(range(nstore)),
                      [ln, ln] + [64] * (nstore - 2), kind, 2200 + 10 * ln + 2 * j + fin_next, quiet=(1,),
                      plants=((0, pos, fin_next),))
    build("tie-nstore3", 3, [0, 1, 2], [64, 65, 63], "round-robin", 2300, quiet=(0, 1, 2), tie=(0, 2))
    build("300-stores-1-row", 300, list(range(300)), [1] * 300, "random", 2400)
    rng = np.random.default_rng(2500)
    few = sorted(rng.choice(65, 20, replace=False).tolist())
    build("more-stores-than-rows", 65, few, [1] * 20, "random", 2500)
    build("two-stores-blocked", 2, [0, 1], [577, 64], "blocked", 2600)
    build("three-stores-reversed", 3, [0, 1, 2], [513, 2, 65], "reversed", 2700)

    def seg(c, s):
        return np.flatnonzero(c[3] == s)

    every = [(c, s, e) for c in cases for s, e in enumerate(c[7])]
    assert {len(c[6]) for c in cases} >= {1, 2, 3, 65, 300}
    assert {seg(c, s).size for c, s, e in every if e is not None} >= set(LENGTHS)
    assert any(any(e is not None and e.apply_row >= 0 for e in c[7]) and
               any(e is not None and e.apply_row < 0 < e.accepted_count for e in c[7]) for c in cases), \
        "an applying store beside a non-applying one"
    assert any(e is None for _, _, e in every), "an empty store"
    assert any(c[0].startswith("tie") and e is not None and e.best_row == -1 and e.next.has_best and e.accepted_count > 0
               for c, s, e in every), "a tie kept by the old best"
    assert any(e is not None and e.best_row >= 0 and e.best_row != seg(c, s)[0] for c, s, e in every)
    assert any(e is not None and e.optimistic_row >= 0 and e.optimistic_row != seg(c, s)[0] for c, s, e in every)
    for what in ("first", "last", "stripe"):
        for fn in ("-finnext", ""):
            hit = [(c, c[7][0]) for c in cases if c[0].startswith(f"apply-{what}{fn}-n")]
            assert len(hit) == 3
            for c, e in hit:
                rows = seg(c, 0)
                stripe = -(-rows.size // 64)
                pos = int(np.searchsorted(rows, e.apply_row))
                assert e.apply_row >= 0 and rows[pos] == e.apply_row and e.rows_consumed == pos + 1, c[0]
                assert {"first": pos == 0, "last": pos == rows.size - 1, "stripe": pos > 0 and pos % stripe == 0}[what], c[0]
                assert c[7][1].apply_row < 0 < c[7][1].accepted_count, c[0]  # the interleaved neighbour has none
                assert bool(c[5][0]) != bool(fn) or not fn, c[0]
    assert any(len(set(c[4].tolist())) > 1 and len(set(c[5].tolist())) > 1 for c in cases), "per-store values that differ"
    return cases


def kernel_case_names():
    return [c[0] for c in kernel_cases()]


def check_kernel_case(verifier, name):
    """debug_fold_stores == the model, store by store; entries of stores without a row keep the sentinel the test
    wrote; one store: also equal to debug_fold on the same rows."""
    from lcv._native import FoldResultC
    rec, ver, six, fin, nk, states, want = next(c[1:] for c in kernel_cases() if c[0] == name)
    raw = (FoldResultC * len(states))()
    ctypes.memset(raw, SENTINEL, ctypes.sizeof(raw))
    got = verifier.debug_fold_stores(rec, ver, six, fin, nk, states, out=raw)
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, s, g, w)
        if w is None:
            assert bytes(raw[s]) == bytes([SENTINEL]) * ctypes.sizeof(FoldResultC), (name, s)
    if len(states) == 1:
        assert got[0] == verifier.debug_fold(rec, ver, int(fin[0]), bool(nk[0]), states[0]), name


# ----------------------------------------------------------------------------- end to end
def third_store(z, p):
    """A store equal in content to stores(z)'s first (next committee known), with another
    previous_max_active_participants and optimistic header."""
    st = H.store_from(int(z["store_finalized_slot"]), z["current_committee"].tobytes(), z["next_committee"].tobytes())
    st.previous_max_active_participants = 400
    att = np.sort(p.att_beacon[:, :8].copy().view("<u8")[:, 0])
    st.optimistic_header.beacon.slot = int(att[att.size // 2])
    return st


def three_stores(z, p):
    return [st for _, st in SF.stores(z)] + [third_store(z, p)]


def check_multi_sequence(verifier, from_packed=True, stats=None, chunk=None):
    """The golden sequence fed to three stores, rows alternating between them, in one
    fold_light_client_updates_multi call: the fixture's accept flags, reasons and store summaries for the first
    two; process_light_client_updates on an equal fresh store for all three.  chunk: rows per validate chunk
    (lcv_debug_set_chunk) for the call — 64 keeps every device call of the 72-row batch on the fan engine, and
    makes the call carry the stores' states from one chunk to the next."""
    if chunk is not None:
        verifier.debug_set_chunk(chunk)
        try:
            return check_multi_sequence(verifier, from_packed, stats)
        finally:
            verifier.debug_set_chunk(65536)
    from lcv import store as LS
    z, _ = store_cases.load()
    f = SF.fixture()
    p = SF.sequence_rows()
    n = p.n
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    mine = three_stores(z, p)
    rows = SF.take(p, np.repeat(np.arange(n), 3))
    owner = mine * n
    ups = rows if from_packed else [H.update_from(rows, i) for i in range(rows.n)]
    reasons, so = [], {}
    acc = LS.fold_light_client_updates_multi(owner, ups, cs, gvr, verifier, reasons, so)
    assert acc.shape == (3 * n,) and len(reasons) == 3 * n
    assert so["rounds"] >= 3, so
    chunks = -(-3 * n // verifier.chunk_rows)
    assert so["rounds"] <= so["validate_calls"] <= chunks * so["rounds"] and 1 <= so["table_uploads"] <= so["rounds"], so
    if stats is not None:
        stats.append(so)
    objects = [H.update_from(p, i) for i in range(n)]
    for k, (st, fresh) in enumerate(zip(mine, three_stores(z, p))):
        got_acc, got_rs = list(acc[k::3].astype(np.uint8)), reasons[k::3]
        if k < 2:
            assert got_acc == list(f["seq_accepted"][k]), k
            assert got_rs == list(f["seq_reason"][k]), k
            assert store_cases.summary(st) == list(f["seq_summary"][k][n - 1]), (k, store_cases.summary(st))
        want_rs = []
        want_acc = LS.process_light_client_updates(fresh, objects, cs, gvr, verifier, want_rs)
        assert got_acc == list(want_acc.astype(np.uint8)) and got_rs == want_rs, k
        assert store_cases.summary(st) == store_cases.summary(fresh), (k, store_cases.summary(st), store_cases.summary(fresh))


def check_chunk_carry(verifier):
    """84 rows in chunks of 64: two stores, rows alternating, each fed 40 sub-2/3 rows (every fifth invalid), then an
    applying row and one more — no store applies in the first chunk, so each store's `next` is carried into the
    second.  Against process_light_client_updates per store."""
    from lcv import store as LS
    z, p = store_cases.load()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    seq = [0, 1, 4, 8, 3] * 8 + [11, 0]
    rows = SF.take(p, np.repeat(seq, 2))
    mine, fresh = [st for _, st in SF.stores(z)], [st for _, st in SF.stores(z)]
    reasons, so = [], {}
    verifier.debug_set_chunk(64)
    try:
        acc = LS.fold_light_client_updates_multi(mine * len(seq), rows, cs, gvr, verifier, reasons, so)
    finally:
        verifier.debug_set_chunk(65536)
    assert so["validate_calls"] > so["rounds"] >= 2, so
    objects = [H.update_from(p, i) for i in seq]
    for k in range(2):
        want_rs = []
        want = LS.process_light_client_updates(fresh[k], objects, cs, gvr, verifier, want_rs)
        assert list(acc[k::2]) == list(want) and reasons[k::2] == want_rs, k
        assert store_cases.summary(mine[k]) == store_cases.summary(fresh[k]), k
        assert want[-2] and not all(want[:-2]) and any(want[:-2]), k
    assert store_cases.summary(mine[0])[0] > int(z["store_finalized_slot"])  # the planted row applied


def check_different_committees(verifier):
    """Three stores in three sync-committee periods (current committee c0 / c1 / c2; next unknown, known, unknown),
    two rows each from store_table_cases.chain_case's generator, interleaved — against process_light_client_updates
    per store."""
    from lcv import store as LS
    from lcv import synth
    c = ST.committees(verifier)
    parts, owners, fresh = [], [], []
    for k in range(3):
        sb = synth.generate(verifier, 2, seed=30 + k, period=synth.DENEB_PERIOD + k, committees=(c[k], c[k + 1]),
                            kinds=np.zeros(2, np.int64))
        nxt = c[k + 1].ssz if k == 1 else ST.ZERO_SC
        parts.append(sb)
        owners.append(H.store_from(sb.store_finalized_slot, c[k].ssz, nxt))
        fresh.append(H.store_from(sb.store_finalized_slot, c[k].ssz, nxt))
    assert len({sb.genesis_validators_root for sb in parts}) == 1
    cs, gvr = max(sb.current_slot for sb in parts), parts[0].genesis_validators_root
    upd = ST.concat([sb.updates for sb in parts])  # rows 2k, 2k + 1: store k
    order = [0, 2, 4, 1, 3, 5]
    rows = ST.take(upd, order)
    reasons, so = [], {}
    acc = LS.fold_light_client_updates_multi([owners[r // 2] for r in order], rows, cs, gvr, verifier, reasons, so)
    assert so["table_uploads"] >= 1
    for k in range(3):
        want_rs = []
        want = LS.process_light_client_updates(fresh[k], [H.update_from(upd, 2 * k + j) for j in range(2)], cs, gvr,
                                               verifier, want_rs)
        mine = [order.index(2 * k + j) for j in range(2)]
        assert [bool(acc[i]) for i in mine] == [bool(a) for a in want], k
        assert [reasons[i] for i in mine] == want_rs, k
        assert store_cases.summary(owners[k]) == store_cases.summary(fresh[k]), k
    assert acc.any()


def _two_store_table(verifier, z):
    """The golden sequence's store twice: row 0 with its next committee, row 1 without."""
    com = np.stack([z["current_committee"], z["next_committee"]])
    fin = int(z["store_finalized_slot"])
    verifier.set_store_table(com, [fin, fin], [0, 0], [1, ST.UNKNOWN])


def check_async(verifier):
    """A single-store folded batch on slot 0 and a table-folded batch on slot 1 in flight together: each equals its
    synchronous result; each slot refuses the other kind's wait with LCV_ESTATE (status -4), and lcv_slot_wait
    hands out the table-folded slot's verdicts as for any staged batch."""
    import pytest
    from lcv import runtime
    from lcv._native import LcvError
    from lcv.device import FoldState
    z, _ = store_cases.load()
    p = SF.sequence_rows()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    fin = int(z["store_finalized_slot"])
    runtime.ensure_store(verifier, fin, z["current_committee"].tobytes(), z["next_committee"].tobytes())
    _two_store_table(verifier, z)
    one, two = p.slice(0, 9), p.slice(0, 12)
    six = np.arange(two.n, dtype=np.uint32) % 2
    s_one = FoldState(optimistic_slot=fin + 5, current_max_active_participants=200)
    s_two = [FoldState(), FoldState(optimistic_slot=fin + 5, previous_max_active_participants=300)]
    want_one = verifier.validate_fold(one, cs, gvr, s_one)
    want_two = verifier.validate_stores_fold(two, six, cs, gvr, s_two)
    assert all(r is not None for r in want_two[2])
    verifier.validate_async_fold(one, cs, gvr, s_one, 0)
    verifier.validate_stores_async_fold(two, six, cs, gvr, s_two, 1)
    with pytest.raises(LcvError, match="status -4"):
        verifier.slot_wait_stores_fold(0, one.n, 2)
    with pytest.raises(LcvError, match="status -4"):
        verifier.slot_wait_fold(1, two.n)
    ok, rs, res = verifier.slot_wait_stores_fold(1, two.n, 2)
    assert list(ok) == list(want_two[0]) and list(rs) == list(want_two[1]) and res == want_two[2], (res, want_two[2])
    ok, rs, res = verifier.slot_wait_fold(0, one.n)
    assert list(ok) == list(want_one[0]) and list(rs) == list(want_one[1]) and res == want_one[2]
    ok, rs = verifier.slot_wait(1, two.n)
    assert list(ok.astype(bool)) == list(want_two[0]) and list(rs) == list(want_two[1])
    # the synchronous table fold of the same rows under the one-store fold's semantics, store by store
    for s in range(2):
        rows = np.flatnonzero(six == s)
        runtime.ensure_store(verifier, fin, z["current_committee"].tobytes(),
                             z["next_committee"].tobytes() if s == 0 else bytes(24624))
        o, r, e = verifier.validate_fold(SF.take(two, rows), cs, gvr, s_two[s])
        g = want_two[2][s]
        back = lambda j: int(rows[j]) if j >= 0 else -1  # noqa: E731
        assert list(o) == list(want_two[0][rows]) and list(r) == list(want_two[1][rows]), s
        assert (g.next, g.rows_consumed, g.accepted_count) == (e.next, e.rows_consumed, e.accepted_count), s
        assert (g.apply_row, g.best_row, g.optimistic_row) == (back(e.apply_row), back(e.best_row), back(e.optimistic_row)), s


def check_refusals(verifier, fresh_verifier):
    """Every refusal is decided on the host before any launch.  fresh_verifier(): a new context (no table set)."""
    import pytest
    from lcv._native import LcvError
    from lcv.device import FoldState, PackedUpdates, RANK_DTYPE
    z, _ = store_cases.load()
    p = SF.sequence_rows().slice(0, 4)
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    v = fresh_verifier()
    try:
        with pytest.raises(LcvError, match="status -4"):  # LCV_ESTATE: no table
            v.validate_stores_fold(p, [0, 1, 0, 1], cs, gvr, [FoldState(), FoldState()])
        with pytest.raises(LcvError, match="status -4"):
            v.validate_stores_async_fold(p, [0, 1, 0, 1], cs, gvr, [FoldState(), FoldState()], 0)
    finally:
        v.close()
    _two_store_table(verifier, z)
    n = 65537
    zc = lambda w: np.zeros((n, w), np.uint8)  # noqa: E731  (untouched pages: the calls refuse before reading them)
    big = PackedUpdates(att_beacon=zc(112), att_exec=zc(832), att_branch=zc(128), fin_beacon=zc(112), fin_exec=zc(832),
                        fin_branch=zc(128), nsc_pool=np.zeros((1, 24624), np.uint8), nsc_index=np.zeros(n, np.uint32),
                        nsc_branch=zc(160), finality_branch=zc(192), sync_bits=zc(64), sync_signature=zc(96),
                        signature_slot=np.zeros(n, np.uint64))
    with pytest.raises(LcvError, match="status -1"):
        verifier.validate_stores_fold(big, np.zeros(n, np.uint32), 0, bytes(32), [FoldState(), FoldState()])
    with pytest.raises(LcvError, match="status -1"):
        verifier.validate_stores_async_fold(big, np.zeros(n, np.uint32), 0, bytes(32), [FoldState(), FoldState()], 0)
    with pytest.raises(LcvError, match="status -1"):
        verifier.debug_fold_stores(np.zeros(n, RANK_DTYPE), np.zeros(n, np.uint8), np.zeros(n, np.uint32), [0], [1],
                                   [FoldState()])
    # a store_index past the table, named by its row
    with pytest.raises(LcvError, match=r"status -1: .*store_index\[2\] = 2 "):
        verifier.validate_stores_fold(p, [0, 1, 2, 1], cs, gvr, [FoldState(), FoldState()])
    with pytest.raises(LcvError, match=r"status -1: .*store_index\[3\] = 7 "):
        verifier.debug_fold_stores(np.zeros(4, RANK_DTYPE), np.zeros(4, np.uint8), [0, 1, 0, 7], [0, 0], [1, 1],
                                   [FoldState(), FoldState()])
    # a present store's maximum above SYNC_COMMITTEE_SIZE, named by its store row; an absent store's is not read
    bad = [FoldState(), FoldState(previous_max_active_participants=513)]
    with pytest.raises(LcvError, match=r"status -1: .*in\[1\]"):
        verifier.validate_stores_fold(p, [0, 1, 0, 1], cs, gvr, bad)
    bad = [FoldState(current_max_active_participants=513), FoldState()]
    with pytest.raises(LcvError, match=r"status -1: .*in\[0\]"):
        verifier.validate_stores_async_fold(p, [0, 1, 0, 1], cs, gvr, bad, 0)
    got = verifier.debug_fold_stores(np.zeros(2, RANK_DTYPE), np.zeros(2, np.uint8), [1, 1], [0, 0], [1, 1], bad)
    assert got[0] is None and got[1].rows_consumed == 2 and got[1].accepted_count == 0
    # the one-store entries still refuse a batch that carries a store index
    SF.check_table_batch_refused(verifier)
