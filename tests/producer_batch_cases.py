"""Cases and checks of the batched producer entries (lcv_create_updates*, lcv_create_bootstraps, lcv_batch_download,
lcv_rank_resident), shared by test_producer_batch_hostsim.py (host simulation of the kernels' code) and
test_producer_batch_gpu.py (the MI355X).

Two sources of expected values:
  * tests/golden/producer.npz: the reference's exec'd full-node.md functions (wire bytes), and
  * lcv/producer.py's per-object functions over a deterministic synthetic chain (`chain()`): about 40 blocks and
    states under a NetworkConfig with small fork epochs, 192 cases that share the views and reach every reason code.
"""
import sys
import traceback
from contextlib import contextmanager
from dataclasses import replace
from functools import lru_cache

import numpy as np

import producer_cases as PC

# 8 slots per epoch, 8 epochs per period: Altair from slot 8, Capella from 24, Deneb from 40, period 1 from 64
SLOTS_PER_EPOCH, EPOCHS_PER_PERIOD = 8, 8
N_CHAIN = 40          # blocks / states of the main chain, block k at slot 2 k
FIN_LAG = 8           # state k's finalized block is block k - 8 (the genesis block up to k = 8)
N_CASES = 192


def small_config():
    from lcv.config import NetworkConfig
    return NetworkConfig(name="producer-batch-test", SLOTS_PER_EPOCH=SLOTS_PER_EPOCH,
                         EPOCHS_PER_SYNC_COMMITTEE_PERIOD=EPOCHS_PER_PERIOD, ALTAIR_FORK_EPOCH=1, BELLATRIX_FORK_EPOCH=2,
                         CAPELLA_FORK_EPOCH=3, DENEB_FORK_EPOCH=5)


@contextmanager
def configured(v, cfg):
    """The verifier under `cfg` (Verifier.set_config), its previous configuration restored afterwards."""
    prev = v.config
    v.set_config(cfg)
    try:
        yield v
    finally:
        v.set_config(prev)


# ------------------------------------------------------------------ the synthetic chain
def _exec_record(rng, extra_len, blob_fields):
    """A well-formed 832-byte execution record (include/lcv.h) with `extra_len` bytes of extra_data."""
    rec = np.zeros(832, np.uint8)
    for k in (0, 2, 3, 5, 12, 13, 14):                       # 32-byte roots / hashes
        rec[32 * k:32 * k + 32] = rng.integers(0, 256, 32)
    rec[32:52] = rng.integers(0, 256, 20)                    # fee_recipient
    for k in (6, 7, 8, 9):                                   # uint64 fields
        rec[32 * k:32 * k + 8] = rng.integers(0, 256, 8)
    rec[320:320 + extra_len] = rng.integers(1, 256, extra_len)
    rec[352:384] = rng.integers(0, 256, 32)                  # base_fee_per_gas
    if blob_fields:                                          # blob_gas_used, excess_blob_gas
        rec[480:488] = rng.integers(1, 256, 8)
        rec[512:520] = rng.integers(1, 256, 8)
    rec[544:800] = rng.integers(0, 256, 256)                 # logs_bloom
    rec[800:804] = np.frombuffer(int(extra_len).to_bytes(4, "little"), np.uint8)
    return rec.tobytes()


class Chain:
    """states / blocks: the view lists; cases: (state, block, attested_state, attested_block, finalized_block)
    rows; intended: the reason each case was built for; tags: what each case covers."""

    def __init__(self, ncomm=3, seed=20241):
        from lcv import producer as PR
        self.cfg = cfg = small_config()
        rng = np.random.default_rng(seed)
        committees = [rng.integers(0, 256, 24624, dtype=np.uint8).tobytes() for _ in range(ncomm)]
        self.states, self.blocks = [], []
        self.extra_lens = []

        def make_pair(slot, parent_root, fin_epoch, fin_root, payload=True, k=0):
            """A consistent (state, block) pair at `slot`: the block's state_root is the state's root, the state's
            latest_block_header is the block's header with state_root zeroed."""
            epoch = cfg.compute_epoch_at_slot(slot)
            execution, deneb = None, True
            if payload and epoch >= cfg.CAPELLA_FORK_EPOCH:
                deneb = epoch >= cfg.DENEB_FORK_EPOCH
                self.extra_lens.append((0, 1, 32)[k % 3])
                execution = _exec_record(rng, self.extra_lens[-1], blob_fields=True)
            blk = PR.BeaconBlockView(slot=slot, proposer_index=int(rng.integers(0, 1 << 20)), parent_root=parent_root,
                                     state_root=bytes(32),
                                     sync_committee_bits=rng.integers(0, 256, 64, dtype=np.uint8).tobytes(),
                                     sync_committee_signature=rng.integers(0, 256, 96, dtype=np.uint8).tobytes(),
                                     execution=execution, execution_deneb=deneb,
                                     body_roots=rng.integers(0, 256, (12, 32), dtype=np.uint8))
            period = cfg.compute_sync_committee_period_at_slot(slot)
            st = PR.BeaconStateView(slot=slot, latest_block_header=blk.header(), finalized_checkpoint_epoch=fin_epoch,
                                    finalized_checkpoint_root=fin_root,
                                    current_sync_committee=committees[period % ncomm],
                                    next_sync_committee=committees[(period + 1) % ncomm],
                                    field_roots=rng.integers(0, 256, (28, 32), dtype=np.uint8))
            blk = replace(blk, state_root=st.hash_tree_root())
            return st, blk

        def fin_of(k):
            f = max(0, k - FIN_LAG)
            return f, (bytes(32) if f == 0 else self.blocks[f].hash_tree_root())

        parent = bytes(32)
        for k in range(N_CHAIN):
            f, froot = fin_of(k)
            st, blk = make_pair(2 * k, parent, cfg.compute_epoch_at_slot(2 * f), froot, k=k)
            self.states.append(st)
            self.blocks.append(blk)
            parent = blk.hash_tree_root()
        add_s = lambda s: (self.states.append(s), len(self.states) - 1)[1]  # noqa: E731
        add_b = lambda b: (self.blocks.append(b), len(self.blocks) - 1)[1]  # noqa: E731

        # a Capella-epoch block WITHOUT a payload (slot 31, child of block 15), and its child (slot 33)
        f, froot = fin_of(15)
        p_st, p_blk = make_pair(31, self.blocks[15].hash_tree_root(), cfg.compute_epoch_at_slot(2 * f), froot, payload=False)
        q_st, q_blk = make_pair(33, p_blk.hash_tree_root(), cfg.compute_epoch_at_slot(2 * f), froot, k=1)
        P_S, P_B, Q_S, Q_B = add_s(p_st), add_b(p_blk), add_s(q_st), add_b(q_blk)
        # ... and a state that finalizes that block, with its block (slot 35, child of Q)
        r_st, r_blk = make_pair(35, q_blk.hash_tree_root(), cfg.compute_epoch_at_slot(31), p_blk.hash_tree_root(), k=2)
        R_S, R_B = add_s(r_st), add_b(r_blk)
        t_st, t_blk = make_pair(37, r_blk.hash_tree_root(), cfg.compute_epoch_at_slot(31), p_blk.hash_tree_root(), k=3)
        T_S, T_B = add_s(t_st), add_b(t_blk)
        # broken copies of chain views
        NOBITS = add_b(replace(self.blocks[21], sync_committee_bits=bytes(64)))
        BADSLOT = add_s(replace(self.states[22], slot=self.states[22].slot + 1))
        BADSLOT_ATT = add_s(replace(self.states[25], slot=self.states[25].slot + 1))

        cases, intended, tags = [], [], []

        def case(st, bk, ast, ab, fb, reason, *tag):
            cases.append((st, bk, ast, ab, fb))
            intended.append(reason)
            tags.append(set(tag))

        def fork_tag(prefix, b):
            e = cfg.compute_epoch_at_slot(self.blocks[b].slot)
            return prefix + ("_deneb" if e >= cfg.DENEB_FORK_EPOCH else "_capella" if e >= cfg.CAPELLA_FORK_EPOCH else "_pre_capella")

        def fork_rank(b):
            e = cfg.compute_epoch_at_slot(self.blocks[b].slot)
            return 2 if e >= cfg.DENEB_FORK_EPOCH else 1 if e >= cfg.CAPELLA_FORK_EPOCH else 0

        # the chain's own updates: block k + 1 signs block k; with its finalized block, without one, and again
        for k in range(N_CHAIN - 1):
            f = max(0, k - FIN_LAG)
            pre_altair = cfg.compute_epoch_at_slot(2 * k) < cfg.ALTAIR_FORK_EPOCH
            base = [fork_tag("att", k)]
            if cfg.compute_sync_committee_period_at_slot(2 * k) != cfg.compute_sync_committee_period_at_slot(2 * k + 2):
                base.append("period_differs")
            if self.blocks[k].execution is not None:
                base.append("extra_%d" % int.from_bytes(self.blocks[k].execution[800:804], "little"))
            with_fin = base + [fork_tag("fin", f)] + (["genesis_finalized"] if f == 0 else [])
            if f and fork_rank(f) < fork_rank(k):
                with_fin.append("fin_earlier_fork")
            case(k + 1, k + 1, k, k, f, 1 if pre_altair else 0, *with_fin)
            case(k + 1, k + 1, k, k, -1, 1 if pre_altair else 0, "no_finalized", *base)
            case(k + 1, k + 1, k, k, f, 1 if pre_altair else 0, *with_fin)
        # :144 no participants
        for fb in (13, -1, 13):
            case(21, NOBITS, 20, 20, fb, 2)
        # :146 state.slot
        for fb in (14, -1):
            case(BADSLOT, 22, 21, 21, fb, 3)
        # :149 the state is not the block's
        for k in (9, 17, 30):
            case(k + 1, k + 2, k, k, max(0, k - FIN_LAG), 4)
            case(k + 2, k + 1, k, k, -1, 4)
        # :152 attested_state.slot
        for fb in (17, -1):
            case(26, 26, BADSLOT_ATT, 25, fb, 5)
        # :155 the attested state is not the attested block's; the block is not the attested block's child
        for k in (10, 18, 33):
            case(k + 1, k + 1, k, k - 1, max(0, k - FIN_LAG), 6)
            case(k + 1, k + 1, k - 1, k, -1, 6)
            case(k + 2, k + 2, k, k, max(0, k - FIN_LAG), 6)
        # :160 the attested block lacks its payload
        for fb in (max(0, 15 - FIN_LAG), -1):
            case(Q_S, Q_B, P_S, P_B, fb, 7)
        # :171 the finalized block lacks its payload (R's and T's states finalize P)
        case(T_S, T_B, R_S, R_B, P_B, 8)
        case(R_S, R_B, Q_S, Q_B, P_B, 8)
        # :172 another finalized block than the checkpoint's
        for k in (12, 24, 36):
            case(k + 1, k + 1, k, k, k - FIN_LAG + 1, 9)
            case(k + 1, k + 1, k, k, k - FIN_LAG - 1, 9)
        # :174 the genesis block given as finalized where the checkpoint names another
        for k in (11, 23, 35):
            case(k + 1, k + 1, k, k, 0, 10)
        # the side chain derives where no header is made of the payload-less block P
        case(R_S, R_B, Q_S, Q_B, -1, 0, "no_finalized", fork_tag("att", Q_B))
        case(T_S, T_B, R_S, R_B, -1, 0, "no_finalized", fork_tag("att", R_B))
        # fill to N_CASES with chain updates at other finalized choices (-1)
        k = 4
        while len(cases) < N_CASES:
            case(k + 1, k + 1, k, k, -1, 0, "no_finalized", fork_tag("att", k))
            k = 4 + (k - 3) % (N_CHAIN - 5)
        assert len(cases) == N_CASES
        order = np.random.default_rng(seed + 1).permutation(N_CASES)  # failures spread over every cut of the list
        self.cases = np.array([cases[i] for i in order], np.int64)
        self.intended = [intended[i] for i in order]
        self.tags = [tags[i] for i in order]

    # -------------------------------------------------------------- expected values: lcv/producer.py, per object
    def expected(self, kind="update"):
        """(rows, raised): UpdateRow per case (UpdateRow() where the per-object function raises) and, per case,
        None or (exception type, line of create_light_client_update the exception passed through)."""
        from lcv import producer as PR
        rows, raised = [], []
        for st, bk, ast, ab, fb in self.cases.tolist():
            try:
                u = PR.create_light_client_update(self.states[st], self.blocks[bk], self.states[ast], self.blocks[ab],
                                                  self.blocks[fb] if fb >= 0 else None, self.cfg)
                if kind == "finality":
                    u = PR.create_light_client_finality_update(u)
                elif kind == "optimistic":
                    u = PR.create_light_client_optimistic_update(u)
                rows.append(u)
                raised.append(None)
            except (AssertionError, ValueError) as e:
                line = [f.lineno for f in traceback.extract_tb(sys.exc_info()[2]) if f.name == "create_light_client_update"][-1]
                rows.append(PR.UpdateRow())
                raised.append((type(e), line))
        return rows, raised

    def expected_reasons(self):
        """The reason code of every case from the per-object function alone: the checks of
        create_light_client_update stand in evaluation order in its source, so the k-th distinct line an
        exception passes through (ascending) is check k.  Needs every check to fail somewhere in the cases."""
        _, raised = self.expected()
        lines = sorted({r[1] for r in raised if r is not None})
        assert len(lines) == 10, lines
        return [0 if r is None else 1 + lines.index(r[1]) for r in raised], raised


@lru_cache(maxsize=None)
def chain(ncomm=3):
    return Chain(ncomm)


@lru_cache(maxsize=None)
def chain_expected(ncomm=3, kind="update"):
    from lcv.producer import pack_updates
    c = chain(ncomm)
    rows, _ = c.expected(kind)
    return pack_updates(rows), c.expected_reasons()[0]


@lru_cache(maxsize=None)
def chain_views(ncomm=3):
    from lcv.producer import pack_views
    c = chain(ncomm)
    return pack_views(c.states, c.blocks)


COLUMNS = ("att_beacon", "att_exec", "att_branch", "fin_beacon", "fin_exec", "fin_branch", "nsc_branch",
           "finality_branch", "sync_bits", "sync_signature", "signature_slot")


def assert_rows_equal(got, exp, rows=None):
    """Packed batches equal row by row; the committee by value (the pools are ordered differently)."""
    idx = range(got.n) if rows is None else rows
    assert got.n == len(idx)
    for name in COLUMNS:
        g, e = getattr(got, name), getattr(exp, name)[list(idx)]
        bad = [i for i in range(got.n) if not np.array_equal(g[i], e[i])]
        assert not bad, f"{name}: rows {bad[:8]} differ"
    for j, i in enumerate(idx):
        assert np.array_equal(got.nsc_pool[int(got.nsc_index[j])], exp.nsc_pool[int(exp.nsc_index[i])]), f"committee of row {j}"


def assert_zero_rows(got, reasons, ncomm):
    for i in np.nonzero(np.asarray(reasons) != 0)[0].tolist():
        for name in COLUMNS:
            assert not np.asarray(getattr(got, name)[i]).any(), f"{name}[{i}] of a failed row is not zero"
        assert int(got.nsc_index[i]) == ncomm and not got.nsc_pool[ncomm].any()


# ------------------------------------------------------------------ checks (one verifier: host simulation or device)
def check_generator_coverage():
    c = chain()
    reasons, raised = c.expected_reasons()
    assert reasons == c.intended
    assert len(c.cases) == N_CASES and 38 <= len(c.blocks) <= 50 and 38 <= len(c.states) <= 50
    assert sorted(set(reasons)) == list(range(11))
    assert reasons.count(0) * 2 >= N_CASES
    assert all((raised[i][0] is ValueError) == (reasons[i] in (7, 8)) for i in range(N_CASES) if reasons[i])
    ok_tags = set().union(*[c.tags[i] for i in range(N_CASES) if reasons[i] == 0])
    need = {"period_differs", "no_finalized", "genesis_finalized", "fin_earlier_fork", "extra_0", "extra_1", "extra_32",
            "att_pre_capella", "att_capella", "att_deneb", "fin_pre_capella", "fin_capella", "fin_deneb"}
    assert need <= ok_tags, need - ok_tags
    assert set(c.extra_lens) == {0, 1, 32}
    # the views are shared: every chain block is `block` of one case and `attested_block` of another
    blocks_as_block, blocks_as_att = set(c.cases[:, 1].tolist()), set(c.cases[:, 3].tolist())
    assert set(range(1, N_CHAIN)) <= blocks_as_block and set(range(N_CHAIN - 1)) <= blocks_as_att
    # a genesis-slot finalized block with a zero root, in a row that succeeds
    assert any(reasons[i] == 0 and c.cases[i, 4] == 0 for i in range(N_CASES))
    v = chain_views()
    assert v.ncomm == 3 and set(v.block_kind.tolist()) == {0, 1, 2}


def fixture_views():
    from lcv.producer import pack_views
    z, cases = PC.load()
    views = pack_views([PC.state_view(z, k) for k in range(len(z["state_slot"]))],
                       [PC.block_view(z, k) for k in range(len(z["block_slot"]))])
    rows = np.array([[c["state"], c["block"], c["attested_state"], c["attested_block"], c["finalized_block"]] for c in cases],
                    np.int64)
    return z, cases, views, rows


def check_reference_fixture(v):
    """The device path against the reference's exec'd functions: wire bytes of the fixture, all three kinds and
    the bootstraps (mainnet configuration, as the fixture was made)."""
    from lcv import wire
    z, cases, views, rows = fixture_views()
    assert views.ns == 10 and views.nb == 15 and len(rows) == 5
    for kind in ("update", "finality", "optimistic"):
        got, reasons = v.create_updates(views, rows, kind)
        assert reasons.tolist() == [0] * 5
        enc = wire.encode_updates(got, kind)
        for i, c in enumerate(cases):
            assert enc[i] == PC.expected(z, kind, i), (kind, c["name"])
    beacon, execution, branch, cidx, cbranch, reasons = v.create_bootstraps(views, rows[:, 2], rows[:, 3])
    assert reasons.tolist() == [0] * 5
    for i, c in enumerate(cases):
        got = wire.encode_bootstrap(beacon[i].tobytes(), execution[i].tobytes(), branch[i].tobytes(),
                                    views.committees[int(cidx[i])].tobytes(), cbranch[i].tobytes())
        assert got == PC.expected(z, "bootstrap", i), c["name"]


def check_differential(v, kind="update", n=N_CASES, ncomm=3):
    """The first n cases of the chain against lcv/producer.py's per-object functions, row by row."""
    c = chain(ncomm)
    exp, exp_reasons = chain_expected(ncomm, kind)
    views = chain_views(ncomm)
    assert views.ncomm == ncomm
    with configured(v, c.cfg):
        got, reasons = v.create_updates(views, c.cases[:n], kind)
    assert reasons.tolist() == exp_reasons[:n]
    assert got.nsc_pool.shape[0] == ncomm + 1 and np.array_equal(got.nsc_pool[:ncomm], views.committees)
    assert_rows_equal(got, exp, rows=range(n))
    assert_zero_rows(got, reasons, ncomm)


def check_single_view(v, n=70):
    """ns = nb = 1: every case points at row 0 (block 10 of the chain and its state)."""
    import pytest
    from lcv.producer import UpdateRow, create_light_client_update, pack_updates, pack_views
    c = chain()
    st, bk = c.states[10], c.blocks[10]
    views = pack_views([st], [bk])
    rows = np.zeros((n, 5), np.int64)
    rows[1::2, 4] = -1
    for fb in (bk, None):  # a block is not its own parent: the :155 assert (reason 6), whatever the finalized block
        with pytest.raises(AssertionError):
            create_light_client_update(st, bk, st, bk, fb, c.cfg)
    with configured(v, c.cfg):
        got, reasons = v.create_updates(views, rows)
    assert reasons.tolist() == [6] * n
    assert_rows_equal(got, pack_updates([UpdateRow()] * n))
    assert_zero_rows(got, reasons, views.ncomm)


def check_bootstraps_differential(v):
    """create_bootstraps over every (state, block) and (attested_state, attested_block) pair of the chain's cases
    against create_light_client_bootstrap, every reason 1..4 included."""
    from lcv import producer as PR
    c = chain()
    views = chain_views()
    pairs = np.concatenate([c.cases[:, 0:2], c.cases[:, 2:4]])
    exp, exp_reason = [], []
    memo = {}
    for st, bk in pairs.tolist():
        if (st, bk) not in memo:
            try:
                memo[(st, bk)] = (PR.create_light_client_bootstrap(c.states[st], c.blocks[bk], c.cfg), None)
            except (AssertionError, ValueError) as e:
                line = traceback.extract_tb(sys.exc_info()[2])[1].lineno
                memo[(st, bk)] = (None, (type(e), line))
        exp.append(memo[(st, bk)])
    lines = sorted({e[1][1] for e in exp if e[1]})
    assert len(lines) == 4, lines
    exp_reason = [0 if e[1] is None else 1 + lines.index(e[1][1]) for e in exp]
    assert sorted(set(exp_reason)) == [0, 1, 2, 3, 4]
    with configured(v, c.cfg):
        beacon, execution, branch, cidx, cbranch, reasons = v.create_bootstraps(views, pairs[:, 0], pairs[:, 1])
    assert reasons.tolist() == exp_reason
    for i, (row, _) in enumerate(exp):
        if row is None:
            assert not (beacon[i].any() or execution[i].any() or branch[i].any() or cbranch[i].any())
            assert int(cidx[i]) == views.ncomm
            continue
        assert beacon[i].tobytes() == row.header.beacon and execution[i].tobytes() == row.header.execution
        assert branch[i].tobytes() == row.header.execution_branch
        assert views.committees[int(cidx[i])].tobytes() == row.current_sync_committee
        assert cbranch[i].tobytes() == row.current_sync_committee_branch


def check_resident_validates(v):
    """The resident batch is validated where it lies: under each fixture case's store, that case's row gives the
    fixture's reason (as test_producer.py::_validate does with the per-object producer)."""
    z, cases, views, rows = fixture_views()
    rb, reasons = v.create_updates_resident(views, rows)
    assert reasons.tolist() == [0] * 5 and rb.n == 5
    cur, nxt = z["current_committee"].tobytes(), z["next_committee"].tobytes()
    gvr = z["genesis_validators_root"].tobytes()
    out = []
    for i, c in enumerate(cases):
        v.set_store(c["store_finalized_slot"], cur, nxt)
        _, reason = v.validate_resident(rb, c["current_slot"], gvr)
        out.append(int(reason[i]))
    rb.free()
    assert out == [c["reason"] for c in cases]


def check_resident_rank_download(v):
    from lcv.store import best_update_per_period
    c = chain()
    views = chain_views()
    with configured(v, c.cfg):
        rb, reasons = v.create_updates_resident(views, c.cases)
        host, reasons_host = v.create_updates(views, c.cases)
        down = v.download(rb)
        assert reasons.tolist() == reasons_host.tolist()
        for name in COLUMNS + ("nsc_index", "nsc_pool"):
            assert np.array_equal(getattr(down, name), getattr(host, name)), name
        assert np.array_equal(v.rank_resident(rb), v.rank(down))
        picked = v.download(rb, rows=[3, 0])
        assert picked.n == 2 and np.array_equal(picked.nsc_pool, down.nsc_pool)
        for name in COLUMNS + ("nsc_index",):
            assert np.array_equal(getattr(picked, name), getattr(down, name)[[3, 0]]), name
        some = [191, 7, 7, 64, 63, 0, 130] * 3  # (more rows than one wave's four teams, with repeats)
        many = v.download(rb, rows=some)
        for name in COLUMNS + ("nsc_index",):
            assert np.array_equal(getattr(many, name), getattr(down, name)[some]), name
        assert v.download(rb, rows=[]).n == 0
        best = best_update_per_period(rb, v)
        assert best == best_update_per_period(down, v) and len(best) >= 1
        rb.free()


def check_refusals(v):
    """Every index column out of range -> LCV_EINVAL before any launch (reason_out untouched); null pointers and
    kind 3 refused; n = 0 fine."""
    import ctypes as C
    import pytest
    from lcv._native import LcvError
    from lcv.device import PackedUpdates
    _, _, views, rows = fixture_views()
    sentinel = np.full(len(rows), 0xEE, np.uint8)

    def refused(views_, rows_, kind=0, resident=False):
        r = sentinel.copy()
        with pytest.raises(LcvError, match="status -1"):
            (v.create_updates_resident if resident else v.create_updates)(views_, rows_, kind, reason=r)
        assert np.array_equal(r, sentinel)
    for col, lim in ((0, views.ns), (1, views.nb), (2, views.ns), (3, views.nb), (4, views.nb)):
        for resident in (False, True):
            bad = rows.copy()
            bad[3, col] = lim
            refused(views, bad, resident=resident)
    bad = rows.copy()
    bad[1, 4] = -2
    refused(views, bad)
    refused(replace(views, state_cur=np.where(np.arange(views.ns) == 4, views.ncomm, views.state_cur).astype(np.uint32)), rows)
    refused(replace(views, state_nxt=np.full(views.ns, views.ncomm, np.uint32)), rows)
    refused(replace(views, block_kind=np.full(views.nb, 3, np.uint8)), rows)
    refused(views, rows, kind=3)
    refused(views, rows, kind=3, resident=True)
    for what in ("state", "block"):
        r = sentinel.copy()
        bad_s, bad_b = rows[:, 2].copy(), rows[:, 3].copy()
        (bad_s if what == "state" else bad_b)[2] = views.ns if what == "state" else views.nb
        with pytest.raises(LcvError, match="status -1"):
            v.create_bootstraps(views, bad_s, bad_b, reason=r)
        assert np.array_equal(r, sentinel)
    # null pointers, straight at the C ABI
    sv, bv, com, keep = views.to_c()
    from lcv.device import _cases_to_c
    uc, cols, n = _cases_to_c(rows)
    r = sentinel.copy()
    rp = r.ctypes.data_as(C.POINTER(C.c_uint8))
    h = C.c_void_p()
    lib, ctx = v.lib, v.ctx
    args = [ctx, C.byref(sv), views.ns, C.byref(bv), views.nb, com, views.ncomm, C.byref(uc), n, 0, rp, C.byref(h)]
    for k in (1, 3, 5, 7, 10, 11):
        a = list(args)
        a[k] = None
        assert lib.lcv_create_updates_resident(*a) == -1 and not h.value
    out, keep_out = PackedUpdates.empty(n, views.ncomm + 1).to_c()
    assert lib.lcv_create_updates(ctx, C.byref(sv), views.ns, C.byref(bv), views.nb, com, views.ncomm, C.byref(uc), n, 0,
                                  None, rp) == -1
    out.sync_bits = None
    assert lib.lcv_create_updates(ctx, C.byref(sv), views.ns, C.byref(bv), views.nb, com, views.ncomm, C.byref(uc), n, 0,
                                  C.byref(out), rp) == -1
    sv_null, _, _, keep2 = views.to_c()
    sv_null.fin_root = None
    a = list(args)
    a[1] = C.byref(sv_null)
    assert lib.lcv_create_updates_resident(*a) == -1 and b"null" in lib.lcv_last_error(ctx)
    assert lib.lcv_batch_download(ctx, None, None, 0, C.byref(out)) == -1
    assert lib.lcv_rank_resident(ctx, None, rp) == -1
    assert lib.lcv_create_bootstraps(ctx, C.byref(sv), views.ns, C.byref(bv), views.nb, com, views.ncomm, None, None, n,
                                     rp, rp, rp, None, rp, rp) == -1
    assert np.array_equal(r, sentinel)
    # n = 0
    got, reasons = v.create_updates(views, np.zeros((0, 5), np.int64))
    assert got.n == 0 and reasons.shape == (0,)
    rb, reasons = v.create_updates_resident(views, np.zeros((0, 5), np.int64))
    assert rb.n == 0 and v.download(rb).n == 0 and v.rank_resident(rb).shape == (0,)
    assert v.create_bootstraps(views, [], [])[5].shape == (0,)
    # a row list out of range
    rb, _ = v.create_updates_resident(views, rows)
    with pytest.raises(LcvError, match="status -1"):
        v.download(rb, rows=[0, 5])
    rb.free()


def check_stage_names(v):
    names = [v.lib.lcv_stage_name(i).decode() for i in range(32)]
    assert names[0] == "nsc_htr" and "produce_views" in names and "produce_rows" in names
    _, _, views, rows = fixture_views()
    v.create_updates(views, rows)
    t = v.last_timings()
    assert t["produce_views"] > 0 and t["produce_rows"] > 0 and t["pre_checks"] == 0
