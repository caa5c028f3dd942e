"""Shared cases of the store-fold tests (tests/test_store_fold_hostsim.py on the host simulation,
tests/test_store_fold_gpu.py on the device): the device fold of process_light_client_update's post-validation
logic (include/lcv.h: lcv_rank_updates, lcv_validate_fold, lcv_debug_fold; lcv.store.fold_light_client_updates).

The committed fixture tests/golden/store_fold.npz (tests/golden/make_store_fold_golden.py) holds what the
reference's OWN exec'd is_better_update / process_light_client_update returned."""
import os
from functools import lru_cache

import numpy as np

import helpers as H
import store_cases

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = store_cases.COLS
SUPER, REL_SC, FIN, FIN_SC, N_MASK = 1 << 23, 1 << 12, 1 << 11, 1 << 10, 0x3FF
SIZES = (1, 2, 63, 64, 65, 127, 129, 4097, 65536)


@lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(HERE, "golden", "store_fold.npz"))


@lru_cache(maxsize=None)
def rank_rows():
    """Fixture (a): the edited rows as a PackedUpdates batch (shared, never modified) and the reference's matrix."""
    from lcv.device import PackedUpdates
    z, (_, p) = fixture(), store_cases.load()
    rows = PackedUpdates(nsc_pool=p.nsc_pool, nsc_index=z["rank_nsc_index"], signature_slot=z["rank_signature_slot"],
                         **{k: z["rank_" + k] for k in COLS})
    return rows, z["rank_better"]


def sequence_rows():
    """Fixture (b): SEQ's rows of store_sequence.npz's batch, in order."""
    _, p = store_cases.load()
    return take(p, fixture()["seq"])


def take(p, idx):
    from lcv.device import PackedUpdates
    idx = np.asarray(idx, np.int64)
    return PackedUpdates(nsc_pool=p.nsc_pool, nsc_index=np.ascontiguousarray(p.nsc_index[idx]),
                         signature_slot=np.ascontiguousarray(p.signature_slot[idx]),
                         **{k: np.ascontiguousarray(getattr(p, k)[idx]) for k in COLS})


def concat(a, b):
    from lcv.device import PackedUpdates
    return PackedUpdates(nsc_pool=a.nsc_pool, nsc_index=np.concatenate([a.nsc_index, b.nsc_index]),
                         signature_slot=np.concatenate([a.signature_slot, b.signature_slot]),
                         **{k: np.concatenate([getattr(a, k), getattr(b, k)]) for k in COLS})


# ----------------------------------------------------------------------------- rank parity
def better_by_rank(a, b) -> bool:
    """The order the header states: (key0, -attested, -signature) lexicographically, equal = not better."""
    ka, kb = (int(a["key0"]), -int(a["attested_slot"]), -int(a["signature_slot"])), \
             (int(b["key0"]), -int(b["attested_slot"]), -int(b["signature_slot"]))
    return ka > kb


def check_rank_matrix(verifier):
    from lcv import store as LS
    rows, better = rank_rows()
    rec = LS.rank_updates(rows, verifier)
    m = rows.n
    assert rec.shape == (m,)
    for a in range(m):
        for b in range(m):
            assert better_by_rank(rec[a], rec[b]) == bool(better[a, b]), (a, b, rec[a], rec[b])


def check_rank_key(verifier):
    """The host's _rank_key (update objects) is the device's record, field for field; update objects in give the
    same records as the packed batch."""
    from lcv import layout as L
    from lcv import store as LS
    rows, _ = rank_rows()
    rec = LS.rank_updates(rows, verifier)
    ups = [L.unpack_update(rows, i) for i in range(rows.n)]
    for i, u in enumerate(ups):
        assert LS._rank_key(u) == rec[i], (i, LS._rank_key(u), rec[i])
    assert (LS.rank_updates(ups[:5], verifier) == rec[:5]).all()


def two_period_rows():
    """The fixture rows (attested in one period, some signed in the next: left out) and a copy moved one period
    on, interleaved so that neither period's rows are contiguous."""
    from lcv.config import MAINNET
    from lcv.device import PackedUpdates
    rows, _ = rank_rows()
    spp = MAINNET.SLOTS_PER_PERIOD
    cols = {k: getattr(rows, k).copy() for k in COLS}
    for k in ("att_beacon", "fin_beacon"):
        slot = cols[k][:, :8].copy().view("<u8")[:, 0] + np.uint64(spp)
        cols[k][:, :8] = slot.reshape(-1, 1).view(np.uint8)
    moved = PackedUpdates(nsc_pool=rows.nsc_pool, nsc_index=rows.nsc_index.copy(),
                          signature_slot=rows.signature_slot + np.uint64(spp), **cols)
    both = concat(rows, moved)
    order = np.random.default_rng(184).permutation(both.n)
    return take(both, order)


def check_best_per_period(verifier):
    from lcv import layout as L
    from lcv import store as LS
    p = two_period_rows()
    got = LS.best_update_per_period(p, verifier)
    ups = [L.unpack_update(p, i) for i in range(p.n)]
    period = LS.compute_sync_committee_period_at_slot
    want, left_out = {}, 0
    for i, u in enumerate(ups):
        per = period(u.attested_header.beacon.slot)
        if period(u.signature_slot) != per:
            left_out += 1
            continue
        if per not in want or LS.is_better_update(u, ups[want[per]]):
            want[per] = i
    assert len(want) == 2 and left_out > 0
    assert got == want


def check_unpack_roundtrip():
    """pack_updates([unpack_update(p, i)]) is row i again, every column."""
    from lcv import layout as L
    from lcv.sync_protocol import pack_updates
    _, p = store_cases.load()
    rows, _ = rank_rows()
    for src, idx in ((p, range(p.n)), (rows, (0, 7, 45))):
        for i in idx:
            q = pack_updates([L.unpack_update(src, i)])
            for k in COLS:
                assert (getattr(q, k)[0] == getattr(src, k)[i]).all(), (i, k)
            assert int(q.signature_slot[0]) == int(src.signature_slot[i])
            assert (q.nsc_pool[0] == src.nsc_pool[int(src.nsc_index[i])]).all()


# ----------------------------------------------------------------------------- the fold kernel alone
STORE_FIN = 1000


def model_better(a, b) -> bool:
    """is_better_update (sync-protocol.md:260-311) on decoded records, level by level as lcv.store.is_better_update
    walks them (not the lexicographic shortcut the kernel uses)."""
    (ka, atta, siga), (kb, attb, sigb) = a, b
    na, nb = ka & N_MASK, kb & N_MASK
    sa, sb = na * 3 >= 512 * 2, nb * 3 >= 512 * 2
    if sa != sb:
        return sa
    if not sa and na != nb:
        return na > nb
    for bit in (REL_SC, FIN):
        if bool(ka & bit) != bool(kb & bit):
            return bool(ka & bit)
    if ka & FIN and bool(ka & FIN_SC) != bool(kb & FIN_SC):
        return bool(ka & FIN_SC)
    if na != nb:
        return na > nb
    if atta != attb:
        return atta < attb
    return siga < sigb


def model_fold(rec, verdict, store_fin, next_known, st):
    """The sequential loop of _apply_valid's rules over the rows (lcv.store._apply_valid, sync-protocol.md:514-553)."""
    from lcv.device import FoldResult, FoldState
    opt, prev, cur = st.optimistic_slot, st.previous_max_active_participants, st.current_max_active_participants
    best = (st.best_key0, st.best_attested_slot, st.best_signature_slot) if st.has_best else None
    best_row = opt_row = apply_row = -1
    acc, consumed = 0, len(rec)
    k0s, fls = rec["key0"].tolist(), rec["flags"].tolist()
    atts, sigs, fins = rec["attested_slot"].tolist(), rec["signature_slot"].tolist(), rec["finalized_slot"].tolist()
    for i in np.flatnonzero(verdict).tolist():
        acc += 1
        k0, n = k0s[i], k0s[i] & N_MASK
        cand = (k0, atts[i], sigs[i])
        if best is None or model_better(cand, best):
            best, best_row = cand, i
        cur = max(cur, n)
        if n > max(prev, cur) // 2 and atts[i] > opt:
            opt, opt_row = atts[i], i
        fin_next = (not next_known) and (fls[i] & 1) and (k0 & FIN) and (k0 & FIN_SC)
        if n * 3 >= 512 * 2 and (fins[i] > store_fin or fin_next):
            apply_row, best, best_row, consumed = i, None, -1, i + 1
            break
    nxt = FoldState(opt, prev, cur, best is not None, *(best if best is not None else (0, 0, 0)))
    return FoldResult(nxt, consumed, apply_row, best_row, opt_row, acc)


def make_records(rng, n, quiet, next_known):
    """Random records from small value sets (ties are common).  quiet: no row can apply."""
    from lcv.device import RANK_DTYPE
    rec = np.zeros(n, RANK_DTYPE)
    cnt = rng.choice([1, 340, 341, 342, 512], n)
    sc, fin, scf = rng.integers(0, 2, n), rng.integers(0, 2, n), rng.integers(0, 2, n)
    rel = sc & rng.integers(0, 2, n)
    att = STORE_FIN + 100 + rng.integers(0, 3, n)
    rec["attested_slot"] = att
    rec["signature_slot"] = att + 1 + rng.integers(0, 2, n)
    rec["finalized_slot"] = np.where(rng.integers(0, 4, n) == 0, STORE_FIN + 7, STORE_FIN - 5)
    if quiet:
        rec["finalized_slot"] = STORE_FIN - 5
        if not next_known:
            sc = np.where(cnt * 3 >= 1024, 0, sc)
            rel = rel & sc
    sup = cnt * 3 >= 1024
    rec["key0"] = (np.where(sup, SUPER, cnt << 13) | rel * REL_SC | fin * FIN | (fin & scf) * FIN_SC | cnt).astype(np.uint32)
    rec["flags"] = sc
    return rec


def plant(rec, verdict, pos, fin_next):
    """Make row `pos` the applying row: a valid supermajority row past the store's finalized slot, or (fin_next)
    one that only the finalized-next rule of a store without a next committee applies."""
    verdict[pos] = 1
    rec["key0"][pos] = SUPER | REL_SC | FIN | FIN_SC | 512
    rec["flags"][pos] = 1
    rec["finalized_slot"][pos] = STORE_FIN - 5 if fin_next else STORE_FIN + 7


@lru_cache(maxsize=None)
def fold_cases():
    """[(name, records, verdicts, next_known, state, expected)] — built once, shared, never modified; `expected`
    is the sequential model's result.  Asserts its own coverage."""
    from lcv.device import FoldState
    cases = []

    def add(name, rec, verdict, next_known, st):
        cases.append((name, rec, verdict, next_known, st, model_fold(rec, verdict, STORE_FIN, next_known, st)))

    def state(rng, with_best):
        st = FoldState(optimistic_slot=STORE_FIN + int(rng.integers(90, 103)),
                       previous_max_active_participants=int(rng.choice([0, 300, 512])),
                       current_max_active_participants=int(rng.choice([0, 1, 341, 512])))
        if with_best:
            st.has_best, st.best_key0 = True, int(rng.choice([341 << 13 | 341, SUPER | FIN | 342, SUPER | REL_SC | 512]))
            st.best_attested_slot = STORE_FIN + 100 + int(rng.integers(0, 3))
            st.best_signature_slot = st.best_attested_slot + 1
        return st

    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        stripe = -(-n // 64)
        reps = 1 if n > 4097 else 2
        for k in range(reps):  # anything goes: applying rows wherever they fall
            nk = k % 2
            add(f"random{k}-n{n}", make_records(rng, n, False, nk), (rng.random(n) < 0.7).astype(np.uint8), nk, state(rng, k == 0))
        add(f"no-valid-n{n}", make_records(rng, n, False, 1), np.zeros(n, np.uint8), 1, state(rng, True))
        # no applying row; the old best ties the batch's best (the batch's best rank is taken from a model run)
        rec, ver = make_records(rng, n, True, 0), (rng.random(n) < 0.7).astype(np.uint8)
        ver[0] = 1
        st = state(rng, False)
        b = model_fold(rec, ver, STORE_FIN, 0, st).next
        st.has_best, st.best_key0 = True, b.best_key0
        st.best_attested_slot, st.best_signature_slot = b.best_attested_slot, b.best_signature_slot
        add(f"quiet-tie-n{n}", rec, ver, 0, st)
        if n > 4097:
            positions = [(stripe * 17, False)]
        else:
            positions = [(0, False), (n - 1, True), (n - 1, False)] + ([(stripe * (n // stripe // 2), True)] if n > 64 else [])
        for pos, fin_next in positions:
            nk = 0 if fin_next else int(rng.integers(0, 2))
            rec, ver = make_records(rng, n, True, nk), (rng.random(n) < 0.7).astype(np.uint8)
            plant(rec, ver, pos, fin_next)
            add(f"apply@{pos}{'-finnext' if fin_next else ''}-n{n}", rec, ver, nk, state(rng, bool(pos % 2)))

    res = [(c[0], len(c[1]), c[3], c[4], c[5]) for c in cases]
    assert any(e.accepted_count == 0 for *_, e in res), "no valid row"
    assert any(e.apply_row < 0 < e.accepted_count for *_, e in res), "no applying row"
    assert any(e.apply_row == 0 for *_, e in res)
    assert any(e.apply_row == n - 1 and n > 64 for _, n, _, _, e in res), "applying row last"
    assert any(n > 64 and e.apply_row > 0 and e.apply_row % -(-n // 64) == 0 for _, n, _, _, e in res), "first row of a stripe"
    assert any("finnext" in name and e.apply_row >= 0 and not nk for name, _, nk, _, e in res)
    assert any(st.has_best for _, _, _, st, _ in res) and any(not st.has_best for _, _, _, st, _ in res)
    assert any(name.startswith("quiet-tie") and e.best_row == -1 and e.next.has_best and e.accepted_count > 0
               for name, _, _, _, e in res), "an old best that ties the batch's best stays"
    assert any(e.best_row >= 0 for *_, e in res) and any(e.optimistic_row >= 0 for *_, e in res)
    assert {n for _, n, *_ in res} == set(SIZES)
    return cases


def fold_case_names():
    return [c[0] for c in fold_cases()]


def check_fold_case(verifier, name):
    rec, ver, nk, st, want = next(c[1:] for c in fold_cases() if c[0] == name)
    got = verifier.debug_fold(rec, ver, STORE_FIN, bool(nk), st)
    assert got == want, (name, got, want)


def check_fold_limits(verifier):
    """n = 65537 through the C entries: LCV_EINVAL (status -1)."""
    import pytest
    from lcv._native import LcvError
    from lcv.device import FoldState, PackedUpdates, RANK_DTYPE
    n = 65537
    with pytest.raises(LcvError, match="status -1"):
        verifier.debug_fold(np.zeros(n, RANK_DTYPE), np.zeros(n, np.uint8), 0, True, FoldState())
    z = lambda w: np.zeros((n, w), np.uint8)  # noqa: E731  (untouched pages: the call refuses before reading them)
    big = PackedUpdates(att_beacon=z(112), att_exec=z(832), att_branch=z(128), fin_beacon=z(112), fin_exec=z(832),
                        fin_branch=z(128), nsc_pool=np.zeros((1, 24624), np.uint8), nsc_index=np.zeros(n, np.uint32),
                        nsc_branch=z(160), finality_branch=z(192), sync_bits=z(64), sync_signature=z(96),
                        signature_slot=np.zeros(n, np.uint64))
    verifier.set_store(0, bytes(24624), bytes(24624))
    verifier._store_key = None  # (lcv.runtime.ensure_store's memo)
    with pytest.raises(LcvError, match="status -1"):
        verifier.validate_fold(big, 0, bytes(32), FoldState())
    with pytest.raises(LcvError, match="status -1"):
        verifier.validate_async_fold(big, 0, bytes(32), FoldState(), 0)


# ----------------------------------------------------------------------------- end to end
def stores(z):
    cur, nxt = z["current_committee"].tobytes(), z["next_committee"].tobytes()
    for case, next_known in enumerate((1, 0)):
        yield case, H.store_from(int(z["store_finalized_slot"]), cur, nxt if next_known else bytes(24624))


def check_sequence(verifier, p, accepted, reason, summary, from_packed, stats=None):
    """fold_light_client_updates over rows p from both starting stores == the reference's recorded run: accept
    flags, reasons, the final store and the store after the force update (the intermediate summaries:
    check_every_prefix).  from_packed: a PackedUpdates batch in (rows rebuilt by unpack_update), else update objects."""
    from lcv import store as LS
    z, _ = store_cases.load()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    n = p.n
    for case, st in stores(z):
        ups = p if from_packed else [H.update_from(p, i) for i in range(n)]
        reasons, so = [], {}
        acc = LS.fold_light_client_updates(st, ups, cs, gvr, verifier, reasons, so)
        assert list(acc.astype(np.uint8)) == list(accepted[case]), case
        assert reasons == list(reason[case]), case
        assert store_cases.summary(st) == list(summary[case][n - 1]), (case, store_cases.summary(st))
        assert so["validate_calls"] == so["segments"], so  # one device call per segment
        if stats is not None:
            stats.append(so)
        LS.process_light_client_store_force_update(st, int(st.finalized_header.beacon.slot) + LS.config.active().UPDATE_TIMEOUT + 1)
        assert store_cases.summary(st) == list(summary[case][n]), (case, store_cases.summary(st))


def check_every_prefix(verifier, p, summary, accepted):
    """Every intermediate store summary of the reference's run: the fold over rows [0, k) for every k."""
    from lcv import store as LS
    z, _ = store_cases.load()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    cur, nxt = z["current_committee"].tobytes(), z["next_committee"].tobytes()
    for case, next_known in enumerate((1, 0)):
        for k in range(1, p.n + 1):
            st = H.store_from(int(z["store_finalized_slot"]), cur, nxt if next_known else bytes(24624))
            acc = LS.fold_light_client_updates(st, p.slice(0, k), cs, gvr, verifier)
            assert list(acc.astype(np.uint8)) == list(accepted[case][:k])
            assert store_cases.summary(st) == list(summary[case][k - 1]), (case, k)


def check_store_sequence(verifier, from_packed=True):
    """The older fixture store_sequence.npz."""
    z, p = store_cases.load()
    check_sequence(verifier, p, z["accepted"], z["reason"], z["summary"], from_packed)


def check_fold_sequence(verifier, from_packed=True, stats=None):
    """Fixture (b): ties, invalid rows, rows after the first apply, a second applying row."""
    f = fixture()
    check_sequence(verifier, sequence_rows(), f["seq_accepted"], f["seq_reason"], f["seq_summary"], from_packed, stats)


def check_equals_sibling(verifier, p):
    """fold_light_client_updates == process_light_client_updates on the same rows (PackedUpdates in, the sibling
    fed with unpack_update's objects): accept flags, reasons, final store."""
    from lcv import layout as L
    from lcv import store as LS
    z, _ = store_cases.load()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    for (case, a), (_, b) in zip(stores(z), stores(z)):
        ra, rb = [], []
        acc_a = LS.fold_light_client_updates(a, p, cs, gvr, verifier, ra)
        acc_b = LS.process_light_client_updates(b, [L.unpack_update(p, i) for i in range(p.n)], cs, gvr, verifier, rb)
        assert list(acc_a) == list(acc_b) and ra == rb, case
        assert store_cases.summary(a) == store_cases.summary(b), case


def check_async_two_slots(verifier):
    """Two folded batches in flight on two slots == the synchronous fold of each; a slot whose batch was enqueued
    without a fold refuses lcv_slot_wait_fold with LCV_ESTATE (status -4)."""
    import pytest
    from lcv import runtime
    from lcv._native import LcvError
    from lcv.device import FoldState
    z, _ = store_cases.load()
    p = sequence_rows()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    runtime.ensure_store(verifier, int(z["store_finalized_slot"]), z["current_committee"].tobytes(), z["next_committee"].tobytes())
    parts = (p.slice(0, 9), p.slice(9, 18))
    states = (FoldState(), FoldState(optimistic_slot=int(z["store_finalized_slot"]) + 5, current_max_active_participants=200))
    want = [verifier.validate_fold(b, cs, gvr, s) for b, s in zip(parts, states)]
    for slot, (b, s) in enumerate(zip(parts, states)):
        verifier.validate_async_fold(b, cs, gvr, s, slot)
    for slot in (1, 0):
        ok, rs, res = verifier.slot_wait_fold(slot, parts[slot].n)
        assert list(ok) == list(want[slot][0]) and list(rs) == list(want[slot][1])
        assert res == want[slot][2], (slot, res, want[slot][2])
    assert want[1][2].apply_row >= 0 and want[0][2].apply_row < 0 and want[0][2].best_row >= 0
    verifier.validate_async(parts[0], cs, gvr, 0)
    with pytest.raises(LcvError, match="status -4"):
        verifier.slot_wait_fold(0, parts[0].n)
    ok, _ = verifier.slot_wait(0, parts[0].n)
    assert list(ok.astype(bool)) == list(want[0][0])


def check_table_batch_refused(verifier):
    import pytest
    from lcv._native import LcvError
    from lcv.device import FoldState
    p = sequence_rows().slice(0, 2)
    with pytest.raises(LcvError, match="status -1"):
        verifier.validate_fold(p, 0, bytes(32), FoldState(), store_index=np.zeros(2, np.uint32))
    with pytest.raises(LcvError, match="status -1"):
        verifier.validate_async_fold(p, 0, bytes(32), FoldState(), 0, store_index=np.zeros(2, np.uint32))
