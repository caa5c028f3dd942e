"""Shared inputs and yardsticks of the store-table tests (tests/test_store_table_hostsim.py on the host simulation,
tests/test_store_table_gpu.py on the device): lcv_set_store_table + lcv_validate_updates_stores validate every
update against its own store row, and lcv.store.sync_light_client_updates uses that to validate a multi-period
catch-up in one call.

The yardstick is always the single-store path the reference-exec'd goldens pin — lcv_set_store + lcv_validate_updates
called once per distinct store — or the goldens themselves.  Everything is exact integers: equality, no tolerance.
"""
import numpy as np

import golden_cases as G
import helpers as H

COLS = G.COLS
UNKNOWN = 0xFFFFFFFF
SC_BYTES = 24624
ZERO_SC = bytes(SC_BYTES)

_cache = {}


# ------------------------------------------------------------------ packed-batch helpers
def concat(parts):
    """Several PackedUpdates back to back, their next_sync_committee pools merged by content."""
    from lcv.device import PackedUpdates
    pool, row_of, index = [], {}, []
    for p in parts:
        remap = np.zeros(p.nsc_pool.shape[0], np.uint32)
        for k in range(p.nsc_pool.shape[0]):
            b = p.nsc_pool[k].tobytes()
            if b not in row_of:
                row_of[b] = len(pool)
                pool.append(p.nsc_pool[k])
            remap[k] = row_of[b]
        index.append(remap[p.nsc_index])
    return PackedUpdates(nsc_pool=np.ascontiguousarray(np.stack(pool)), nsc_index=np.concatenate(index).astype(np.uint32),
                         signature_slot=np.concatenate([p.signature_slot for p in parts]),
                         **{k: np.ascontiguousarray(np.concatenate([getattr(p, k) for p in parts])) for k in COLS})


def take(p, rows):
    """Rows `rows` of p (any order, repeats allowed); the pool is shared."""
    from lcv.device import PackedUpdates
    rows = np.asarray(rows, np.int64)
    return PackedUpdates(nsc_pool=p.nsc_pool, nsc_index=p.nsc_index[rows].copy(), signature_slot=p.signature_slot[rows].copy(),
                         **{k: np.ascontiguousarray(getattr(p, k)[rows]) for k in COLS})


def yardstick(verifier, p, row_store, current_slot, gvr):
    """Reasons of the single-store path: row i of p under the store row_store[i] = (finalized slot, current bytes,
    next bytes), by lcv_set_store + lcv_validate_updates once per distinct store."""
    out = np.full(p.n, 255, np.uint8)
    for store in sorted(set(row_store)):
        rows = [i for i in range(p.n) if row_store[i] == store]
        verifier.set_store(*store)
        ok, reason = verifier.validate(take(p, rows), current_slot, gvr)
        assert np.array_equal(ok, reason == 0)
        out[rows] = reason
    return out


def committees(verifier):
    """c0 .. c3 (lcv.synth.make_committee: the same keys on every backend), made once."""
    if "committees" not in _cache:
        from lcv import synth
        _cache["committees"] = [synth.make_committee(verifier, k) for k in range(4)]
    return _cache["committees"]


# ------------------------------------------------------------------ test 1: the goldens in fewer calls
def run_golden_cases(verifier):
    """The lc_updates golden cases grouped by current_slot only: each case's (store_finalized_slot,
    store_next_known) is a store row.  Returns (reasons, expected, number of validate calls)."""
    g = G.load_updates()
    n = len(g["expected_reason"])
    gvr = g["genesis_validators_root"].tobytes()
    stores = sorted({(int(g["store_finalized_slot"][i]), int(g["store_next_known"][i])) for i in range(n)})
    verifier.set_store_table(g["nsc_pool"][:2], [s[0] for s in stores], [0] * len(stores),
                             [1 if s[1] else UNKNOWN for s in stores])
    from lcv.device import PackedUpdates
    p = PackedUpdates(nsc_pool=g["nsc_pool"], nsc_index=g["nsc_index"], signature_slot=g["signature_slot"],
                      **{k: g[k] for k in COLS})
    index = np.array([stores.index((int(g["store_finalized_slot"][i]), int(g["store_next_known"][i]))) for i in range(n)],
                     np.uint32)
    out = np.full(n, 255, np.uint8)
    slots = sorted({int(s) for s in g["current_slot"]})
    for cs in slots:
        rows = [i for i in range(n) if int(g["current_slot"][i]) == cs]
        ok, reason = verifier.validate_stores(take(p, rows), index[rows], cs, gvr)
        assert np.array_equal(ok, reason == 0)
        out[rows] = reason
    return out, g["expected_reason"], len(slots)


# ------------------------------------------------------------------ test 2: per-row semantics in one batch
# (update, store) of the 10 rows and what sync-protocol.md says of each
SEM_ROWS = [("A", 0), ("A", 1),                      # (a) signed by the store's current: valid; another current: :464
            ("B", 0), ("B", 2), ("B", 3), ("B", 4),  # (b) :442 next equal / byte 0 / byte 24,623 differs / unknown (has_next)
            ("C", 4), ("C", 0),                      # (c) next-period signature, next unknown: :404; (d) next = signer: valid
            ("B", 5), ("C", 5)]                      # (e) an all-zero committee row as next = unknown
SEM_EXPECTED = [0, 14, 0, 12, 12, 0, 5, 0, 0, 5]


def semantics_case(verifier):
    """One 10-row batch over a committee table of 5 rows — c0, c1, c1 with byte 0 changed, c1 with byte 24,623 (the
    last byte of aggregate_pubkey) changed, all-zero — and 6 stores (the issue's 4 committees and 5 stores, and
    one of each more for case (e)).  A and B are same-period updates signed by c0 that carry c1; C is signed in
    the next period by c1 (sign_next)."""
    if "sem" in _cache:
        return _cache["sem"]
    from lcv import synth
    c = committees(verifier)
    ab = synth.generate(verifier, 2, seed=21, committees=(c[0], c[1]))
    nx = synth.generate(verifier, 1, seed=22, committees=(c[0], c[1]), sign_next=True)
    assert ab.genesis_validators_root == nx.genesis_validators_root
    upd = concat([ab.updates, nx.updates])  # rows A, B, C
    assert int(upd.nsc_index[0]) == int(upd.nsc_index[1])  # A and B share a pool row
    fin = ab.store_finalized_slot
    c1 = c[1].ssz
    c1_first = bytes([c1[0] ^ 1]) + c1[1:]
    c1_last = c1[:-1] + bytes([c1[-1] ^ 1])
    table = [c[0].ssz, c1, c1_first, c1_last, ZERO_SC]
    stores = [(fin, 0, 1), (fin, 1, 1), (fin, 0, 2), (fin, 0, 3), (fin, 0, UNKNOWN), (fin, 0, 4)]
    urow = {"A": 0, "B": 1, "C": 2}
    case = dict(
        updates=upd, committees=np.frombuffer(b"".join(table), np.uint8).reshape(len(table), SC_BYTES), table=table,
        stores=stores, rows=[(urow[u], s) for u, s in SEM_ROWS],
        current_slot=max(ab.current_slot, nx.current_slot), gvr=ab.genesis_validators_root)
    _cache["sem"] = case
    return case


def store_key(case, s):
    """(finalized slot, current bytes, next bytes) of store row s: what lcv_set_store takes."""
    fin, cur, nxt = case["stores"][s]
    return (fin, case["table"][cur], ZERO_SC if nxt == UNKNOWN else case["table"][nxt])


def set_table(verifier, case):
    st = case["stores"]
    return verifier.set_store_table(case["committees"], [s[0] for s in st], [s[1] for s in st], [s[2] for s in st])


def run_semantics(verifier):
    """(reasons of the 10-row batch through the store table, reasons of the per-store yardstick)."""
    case = semantics_case(verifier)
    p = take(case["updates"], [u for u, _ in case["rows"]])
    want = yardstick(verifier, p, [store_key(case, s) for _, s in case["rows"]], case["current_slot"], case["gvr"])
    set_table(verifier, case)
    ok, got = verifier.validate_stores(p, [s for _, s in case["rows"]], case["current_slot"], case["gvr"])
    assert np.array_equal(ok, got == 0)
    return got, want


# ------------------------------------------------------------------ test 4: chunk offset
def run_chunks(verifier):
    """130 rows = 13 tiles of test 2's 10 rows, tile t's store_index rotated by 5 (t % 2) rows, with validate cut
    into chunks of 64 rows: a store_index (or a per-row flag) that is not advanced by the chunk base reads the
    first chunk's entries.  Returns (reasons, per-store yardstick), row for row."""
    case = semantics_case(verifier)
    rows = []
    for t in range(13):
        for j in range(10):
            rows.append((case["rows"][j][0], case["rows"][(j + 5 * (t % 2)) % 10][1]))
    assert len(rows) == 130
    pairs = sorted(set(rows))
    assert len(pairs) <= 16  # the host simulation's time goes with the distinct rows of the yardstick
    assert any(rows[i][1] != rows[i + 64][1] for i in range(64))
    pp = take(case["updates"], [u for u, _ in pairs])
    ref = yardstick(verifier, pp, [store_key(case, s) for _, s in pairs], case["current_slot"], case["gvr"])
    want = np.array([ref[pairs.index(r)] for r in rows], np.uint8)
    set_table(verifier, case)
    assert verifier.lib.lcv_debug_set_chunk(verifier.ctx, 64) == 0
    try:
        ok, got = verifier.validate_stores(take(case["updates"], [u for u, _ in rows]), [s for _, s in rows],
                                           case["current_slot"], case["gvr"])
    finally:
        assert verifier.lib.lcv_debug_set_chunk(verifier.ctx, 65536) == 0
    assert np.array_equal(ok, got == 0)
    return got, want


# ------------------------------------------------------------------ tests 5, 6: range sync over 3 periods
class CountingVerifier:
    """A verifier that counts its device validations (validate / validate_stores) and store uploads."""

    def __init__(self, v):
        self._v = v
        self.validations = 0
        self.uploads = 0

    def __getattr__(self, name):
        return getattr(self._v, name)

    def validate(self, *a, **k):
        self.validations += 1
        return self._v.validate(*a, **k)

    def validate_stores(self, *a, **k):
        self.validations += 1
        return self._v.validate_stores(*a, **k)

    def set_store(self, *a, **k):
        self.uploads += 1
        return self._v.set_store(*a, **k)

    def set_store_table(self, *a, **k):
        self.uploads += 1
        return self._v.set_store_table(*a, **k)


def chain_case(verifier, bad_first_of_second_period=False):
    """Six updates, two per period: period P signed by c0 carrying c1, P + 1 signed by c1 carrying c2, P + 2 signed by
    c2 carrying c3, each with finality and full participation; the store starts at period P with current = c0 and
    the next committee unknown."""
    key = ("chain", bad_first_of_second_period)
    if key in _cache:
        return _cache[key]
    from lcv import synth
    c = committees(verifier)
    parts = []
    for k in range(3):
        gen = lambda kinds: synth.generate(verifier, 2, seed=30 + k, period=synth.DENEB_PERIOD + k,  # noqa: E731
                                           committees=(c[k], c[k + 1]), kinds=kinds)
        sb = gen(np.zeros(2, np.int64))
        att = [int.from_bytes(sb.updates.att_beacon[i, :8].tobytes(), "little") for i in range(2)]
        order = [0, 1] if att[0] < att[1] else [1, 0]  # a period's two updates in slot order, as a server sends them
        if bad_first_of_second_period and k == 1:
            kinds = np.zeros(2, np.int64)
            kinds[order[0]] = synth.K_BAD_SIG_MESSAGE  # (the kind draws no random number: the rows are the same otherwise)
            sb = gen(kinds)
        parts.append((sb, take(sb.updates, order)))
    upd = concat([p for _, p in parts])
    case = dict(updates=[H.update_from(upd, i) for i in range(upd.n)], fin=parts[0][0].store_finalized_slot, cur=c[0].ssz,
                current_slot=max(sb.current_slot for sb, _ in parts), gvr=parts[0][0].genesis_validators_root)
    _cache[key] = case
    return case


def run_sync(verifier, case, updates=None):
    """process_light_client_updates and sync_light_client_updates on equal fresh stores -> (old, new), each
    (accept flags, reasons, store summary, device validations); new also carries stats_out."""
    import store_cases
    from lcv import store as LS
    ups = case["updates"] if updates is None else updates
    out = []
    for fn in (LS.process_light_client_updates, LS.sync_light_client_updates):
        st = H.store_from(case["fin"], case["cur"], ZERO_SC)
        cv = CountingVerifier(verifier)
        reasons, stats = [], {}
        kw = {"stats_out": stats} if fn is LS.sync_light_client_updates else {}
        acc = fn(st, ups, case["current_slot"], case["gvr"], cv, reasons, **kw)
        out.append(dict(accepted=[bool(a) for a in acc], reasons=reasons, summary=store_cases.summary(st),
                        validations=cv.validations, stats=stats))
    return out
