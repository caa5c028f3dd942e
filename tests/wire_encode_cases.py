"""Cases and checks of the device SSZ encoder (lcv_batch_encode, lcv_encode_updates, lcv.wire.encode_updates_device,
lcv.producer.updates_by_range), shared by test_wire_encode_hostsim.py (host simulation of the kernel's code) and
test_wire_encode_gpu.py (the MI355X).

Expected bytes: the reference-serialised messages of tests/golden/wire.npz, an Altair update serialised by the
oracle's SSZ, and lcv.wire.encode_updates (the Python encoder: the definition) over generated rows.  Every batch has
at most 130 rows of at most 27 KB.
"""
import hashlib
from functools import lru_cache

import numpy as np
import pytest

import helpers as H
import producer_batch_cases as PB
from golden_cases import COLS, load_updates

from lcv import wire
from oracle import spec as S
from oracle.ssz import Container, serialize

KINDS = ("update", "finality", "optimistic")
FORKS = ("deneb", "capella", "altair")
SHAPES = (1, 63, 64, 65, 130)
PITCH = {"update": 26880, "finality": 2096, "optimistic": 1040}
# extra_data lengths in the order the generator deals them: the ends of the range first, then the rest of 0 .. 32
LENS = [0, 1, 31, 32] + list(range(2, 31))


def packed(g=None):
    from lcv.device import PackedUpdates
    g = g if g is not None else load_updates()
    return PackedUpdates(nsc_pool=g["nsc_pool"], nsc_index=g["nsc_index"], signature_slot=g["signature_slot"],
                         **{k: g[k] for k in COLS})


def take(p, idx):
    """Rows idx of p (a copy; the pool shared)."""
    from lcv.device import PackedUpdates
    idx = np.asarray(idx, np.int64)
    return PackedUpdates(**{name: getattr(p, name) if pool else np.ascontiguousarray(getattr(p, name)[idx])
                            for name, (_, _, pool) in PackedUpdates._SPEC.items()})


def set_extra(rec, elen, rng):
    """extra_data of one 832-byte execution record: `elen` bytes (none of them zero) and the length word."""
    rec[320:352] = 0
    rec[320:320 + min(elen, 32)] = rng.integers(1, 256, min(elen, 32))
    rec[800:804] = np.frombuffer(int(elen).to_bytes(4, "little"), np.uint8)


@lru_cache(maxsize=None)
def rows_for(n, fork, seed=7):
    """n golden rows (cycled) made encodable under `fork`: Deneb / Capella rows get extra_data lengths dealt from
    LENS (attested: row j -> LENS[j % 33]; finalized: LENS[(7 j + 3) % 33]) with fresh bytes, so with n >= 33 the
    finalized header starts at every offset modulo 16; Altair rows lose their execution data."""
    rng = np.random.default_rng(seed + n)
    g = packed()
    b = take(g, np.arange(n) % g.n)
    for j in range(n):
        if fork == "altair":
            for name in ("att_exec", "att_branch", "fin_exec", "fin_branch"):
                getattr(b, name)[j] = 0
        else:
            set_extra(b.att_exec[j], LENS[j % 33], rng)
            set_extra(b.fin_exec[j], LENS[(7 * j + 3) % 33], rng)
    return b


def elens(b):
    return (b.att_exec[:, 800:804].copy().view("<u4").reshape(-1).astype(int),
            b.fin_exec[:, 800:804].copy().view("<u4").reshape(-1).astype(int))


def assert_encoded(enc, exp, fork_code=None):
    """Lengths, bytes and zero fill of an EncodedMessages against the expected messages."""
    assert enc.n == len(exp)
    assert enc.status.tolist() == [0] * len(exp)
    assert enc.length.tolist() == [len(m) for m in exp]
    got = enc.messages()
    bad = [i for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, f"rows {bad[:8]} differ"
    for i, m in enumerate(exp):
        assert not enc.buf[i, len(m):].any(), f"row {i}: bytes past the message are not zero"
    if fork_code is not None:
        assert enc.fork.tolist() == [fork_code] * len(exp)


# ------------------------------------------------------------------ the generator itself (CPU, no verifier)
def check_generator():
    """The Python encoder raises for none of the generated rows; every (attested extra_data length mod 16, fork)
    occurs, the lengths 0, 1, 31, 32 among them, and the finalized header starts at all 16 residues."""
    for fork in FORKS:
        for n in SHAPES:
            b = rows_for(n, fork)
            for kind in KINDS:
                assert len(wire.encode_updates(b, kind, fork)) == n
    for fork in ("deneb", "capella"):
        for n in (63, 64, 65, 130):
            att, fin = elens(rows_for(n, fork))
            assert {0, 1, 31, 32} <= set(att.tolist()) and set(att.tolist()) == set(range(33))
            assert {a % 16 for a in att.tolist()} == set(range(16))
            fixed = 828 if fork == "deneb" else 812
            assert {(25152 + fixed + a) % 16 for a in att.tolist()} == set(range(16))  # where the finalized header starts
            assert {0, 32} <= set(fin.tolist())


# ------------------------------------------------------------------ 1. reference bytes
class AltairHeader(Container):  # upstream altair LightClientHeader: beacon only (fixed-size)
    beacon: S.BeaconBlockHeader


class AltairUpdate(Container):
    attested_header: AltairHeader
    next_sync_committee: S.SyncCommittee
    next_sync_committee_branch: S.NextSyncCommitteeBranch
    finalized_header: AltairHeader
    finality_branch: S.FinalityBranch
    sync_aggregate: S.SyncAggregate
    signature_slot: S.Slot


def check_reference_bytes(v):
    import os
    from golden_cases import GOLDEN
    w = dict(np.load(os.path.join(GOLDEN, "wire.npz"), allow_pickle=False))
    for k, kind in enumerate(KINDS):
        sel = np.flatnonzero(w["kind"] == k)
        msgs = [w["buf"][int(w["offsets"][i]):int(w["offsets"][i] + w["lengths"][i])].tobytes() for i in sel]
        assert msgs
        batch = wire.decode_updates(msgs, kind=kind, lib=v.lib)
        enc = v.encode(batch, kind, "deneb")
        assert enc.buf.shape == (len(msgs), PITCH[kind]) and v.encode_pitch(kind) == PITCH[kind]
        assert_encoded(enc, msgs, 0)
        assert wire.encode_updates_device(batch, kind, "deneb", verifier=v) == msgs
    p = packed()
    u = H.update_from(p, 30)  # bellatrix_valid: pre-Capella, empty execution
    alt = serialize(AltairUpdate(attested_header=AltairHeader(beacon=u.attested_header.beacon),
                                 next_sync_committee=u.next_sync_committee,
                                 next_sync_committee_branch=u.next_sync_committee_branch,
                                 finalized_header=AltairHeader(beacon=u.finalized_header.beacon),
                                 finality_branch=u.finality_branch, sync_aggregate=u.sync_aggregate,
                                 signature_slot=u.signature_slot))
    assert len(alt) == 25368
    assert_encoded(v.encode(p.slice(30, 31), "update", "altair"), [alt], 2)


# ------------------------------------------------------------------ 2. differential against encode_updates
def check_differential(v, kind, fork, n):
    b = rows_for(n, fork)
    exp = wire.encode_updates(b, kind, fork)
    enc = v.encode(b, kind, fork)
    assert_encoded(enc, exp, FORKS.index(fork))
    # the version is that of the attested slot's epoch, whatever the fork forced
    ver = [v.config.compute_fork_version(v.config.compute_epoch_at_slot(int(s))) for s in b.att_beacon[:, :8].copy().view("<u8").reshape(-1)]
    assert [enc.version[i].tobytes() for i in range(n)] == ver


# ------------------------------------------------------------------ 3. every byte written
def check_every_byte_written(v):
    from lcv.device import EncodedMessages
    n = 40
    for kind in ("update", "finality"):
        long_rows = take(rows_for(130, "deneb"), [3 + 33 * (j % 3) for j in range(n)])  # attested extra_data: 32 bytes
        assert set(elens(long_rows)[0].tolist()) == {32}
        short_rows = rows_for(n, "altair")
        refused = take(rows_for(n, "deneb"), np.arange(n))
        refused.att_exec[5, 800:804] = np.frombuffer((33).to_bytes(4, "little"), np.uint8)
        refused.fin_exec[n - 1, 800:804] = np.frombuffer((40).to_bytes(4, "little"), np.uint8)
        for b, fork, bad in ((long_rows, "deneb", ()), (short_rows, "altair", ()), (refused, "deneb", (5, n - 1)),
                             (short_rows, "altair", ())):
            out = EncodedMessages.empty(n, PITCH[kind], fill=0xA5)
            out.length[:] = 0xA5A5A5A5
            enc = v.encode(b, kind, fork, out=out)
            assert enc is out
            good = [i for i in range(n) if i not in bad]
            exp = wire.encode_updates(take(b, good), kind, fork)
            for i, m in zip(good, exp):
                assert int(enc.length[i]) == len(m) and enc.status[i] == 0
                assert enc.buf[i, :len(m)].tobytes() == m
                assert not enc.buf[i, len(m):].any(), (kind, fork, i)
            for i in bad:
                assert enc.status[i] == 2 and enc.length[i] == 0 and not enc.buf[i].any(), (kind, i)


# ------------------------------------------------------------------ 4. the fork per row
def auto_batch(cfg):
    """Rows at attested slots one before and exactly at the Capella and Deneb boundaries, in the Bellatrix and Altair
    epochs and before Altair, with the data their fork's container takes."""
    spe = cfg.SLOTS_PER_EPOCH
    cap, den = cfg.CAPELLA_FORK_EPOCH * spe, cfg.DENEB_FORK_EPOCH * spe
    slots = [cap - 1, cap, den - 1, den, cfg.BELLATRIX_FORK_EPOCH * spe, cfg.ALTAIR_FORK_EPOCH * spe, 0, den + 1000,
             cap + 1, den - 1, cap - 1, den]
    forks = ["altair" if s < cap else "capella" if s < den else "deneb" for s in slots]
    b = take(rows_for(len(slots), "deneb"), np.arange(len(slots)))
    for j, (s, f) in enumerate(zip(slots, forks)):
        b.att_beacon[j, :8] = np.frombuffer(int(s).to_bytes(8, "little"), np.uint8)
        if f == "altair":
            for name in ("att_exec", "att_branch", "fin_exec", "fin_branch"):
                getattr(b, name)[j] = 0
    return b, slots, forks


def check_auto_fork(v):
    cfg = PB.small_config()
    b, slots, forks = auto_batch(cfg)
    assert forks[:4] == ["altair", "capella", "capella", "deneb"]
    versions = [cfg.compute_fork_version(cfg.compute_epoch_at_slot(s)) for s in slots]
    assert versions[4] == cfg.BELLATRIX_FORK_VERSION and versions[0] == cfg.BELLATRIX_FORK_VERSION
    assert versions[5] == cfg.ALTAIR_FORK_VERSION and versions[6] == cfg.GENESIS_FORK_VERSION
    with PB.configured(v, cfg):
        for kind in KINDS:
            enc = v.encode(b, kind, "auto")
            exp = [wire.encode_updates(b.slice(i, i + 1), kind, forks[i])[0] for i in range(b.n)]
            assert_encoded(enc, exp)
            assert enc.fork.tolist() == [FORKS.index(f) for f in forks]
            assert [enc.version[i].tobytes() for i in range(b.n)] == versions
            assert wire.encode_updates_device(b, kind, "auto", verifier=v) == exp
        # a forced fork keeps the version of the attested slot
        enc = v.encode(b.slice(3, 4), "optimistic", "capella")
        assert enc.fork.tolist() == [1] and enc.version[0].tobytes() == cfg.DENEB_FORK_VERSION


# ------------------------------------------------------------------ 5. statuses
def check_statuses(v):
    n = 6
    b = take(rows_for(n, "altair"), np.arange(n))
    b.att_exec[1, 700] = 1        # one execution byte of the attested header
    b.att_branch[2, 127] = 0x80   # one execution-branch byte
    b.fin_exec[3, 0] = 9          # the finalized record
    b.fin_branch[4, 64] = 1
    for kind, exp in (("update", [0, 1, 1, 1, 1, 0]), ("finality", [0, 1, 1, 1, 1, 0]), ("optimistic", [0, 1, 1, 0, 0, 0])):
        enc = v.encode(b, kind, "altair")
        assert enc.status.tolist() == exp, kind
        for i in range(n):
            if exp[i]:
                assert enc.length[i] == 0 and not enc.buf[i].any()
            else:  # (the Python encoder looks at the finalized record for kind 2 as well: compare on clean rows)
                assert enc.messages()[i] == wire.encode_updates(rows_for(n, "altair").slice(i, i + 1), kind, "altair")[0]
        with pytest.raises(ValueError, match=r"row\(s\) \[1, 2"):
            wire.encode_updates_device(b, kind, "altair", verifier=v)
    for fork in ("deneb", "capella"):
        d = take(rows_for(n, fork), np.arange(n))
        d.att_exec[2, 800:804] = np.frombuffer((33).to_bytes(4, "little"), np.uint8)
        d.fin_exec[4, 800:804] = np.frombuffer((0x01000000).to_bytes(4, "little"), np.uint8)
        for kind, exp in (("update", [0, 0, 2, 0, 2, 0]), ("finality", [0, 0, 2, 0, 2, 0]), ("optimistic", [0, 0, 2, 0, 0, 0])):
            enc = v.encode(d, kind, fork)
            assert enc.status.tolist() == exp, (fork, kind)
            assert [int(x) for x in enc.length[[2]]] == [0] and not enc.buf[2].any()
            with pytest.raises(ValueError, match="extra_data"):
                wire.encode_updates_device(d, kind, fork, verifier=v)


# ------------------------------------------------------------------ 6. row lists and chunks
def check_rows_and_chunks(v):
    n = 130
    b = rows_for(n, "deneb")
    exp = wire.encode_updates(b, "update", "deneb")
    rb = v.upload(b)
    try:
        assert_encoded(v.encode_resident(rb, "update", "deneb"), exp, 0)
        rev = list(range(n))[::-1]
        assert_encoded(v.encode_resident(rb, "update", "deneb", rows=rev), [exp[i] for i in rev], 0)
        some = [129, 7, 7, 64, 63, 0, 129, 7] * 9
        assert_encoded(v.encode_resident(rb, "update", "deneb", rows=some), [exp[i] for i in some], 0)
        assert v.encode_resident(rb, "update", "deneb", rows=[]).n == 0
        assert wire.encode_updates_device(rb, "update", "deneb") == exp
        v.debug_set_encode_chunk(64)  # 64 + 64 + 2 rows
        try:
            assert_encoded(v.encode_resident(rb, "update", "deneb"), exp, 0)
            assert_encoded(v.encode_resident(rb, "update", "deneb", rows=rev), [exp[i] for i in rev], 0)
            assert_encoded(v.encode_resident(rb, "finality", "capella", rows=some),
                           [wire.encode_updates(b, "finality", "capella")[i] for i in some], 1)
        finally:
            v.debug_set_encode_chunk(0)
    finally:
        rb.free()


# ------------------------------------------------------------------ 7. a batch the producer made on the device
def chain_forks(cfg, batch):
    spe = cfg.SLOTS_PER_EPOCH
    slots = batch.att_beacon[:, :8].copy().view("<u8").reshape(-1)
    return ["altair" if s < cfg.CAPELLA_FORK_EPOCH * spe else "capella" if s < cfg.DENEB_FORK_EPOCH * spe else "deneb"
            for s in slots.tolist()]


def check_resident_producer(v):
    from lcv import producer as PR
    from lcv.store import best_update_per_period
    c = PB.chain()
    views = PB.chain_views()
    gvr = hashlib.sha256(b"genesis validators root").digest()
    with PB.configured(v, c.cfg):
        rb, reasons = v.create_updates_resident(views, c.cases)
        try:
            down = v.download(rb)
            forks = chain_forks(c.cfg, down)
            assert set(forks) == set(FORKS)
            # a row without a next_sync_committee points at the pool's all-zero row, and failed rows are all zero
            assert (down.nsc_index == views.ncomm).any() and (reasons != 0).any()
            exp = [wire.encode_updates(down.slice(i, i + 1), "update", forks[i])[0] for i in range(down.n)]
            enc = v.encode_resident(rb, "update", "auto")
            assert_encoded(enc, exp)
            assert enc.fork.tolist() == [FORKS.index(f) for f in forks]
            zero_pool = [int(i) for i in np.flatnonzero(down.nsc_index == views.ncomm)[:5]]
            assert_encoded(v.encode_resident(rb, "update", "auto", rows=zero_pool), [exp[i] for i in zero_pool])
            # LightClientUpdatesByRange
            best = best_update_per_period(rb, v)
            assert len(best) >= 2
            digest_fork = {wire.fork_digest(ver, gvr): wire.fork_of_digest_version(ver, c.cfg)
                           for ver in c.cfg.fork_versions()[1:]}
            first = min(best)
            for start, count in ((first, 1), (first, 2), (first, 1000), (first + 1, 5), (max(best) + 1, 3), (first, 0)):
                chunks = PR.updates_by_range(rb, start, count, gvr, v)
                periods = [p for p in sorted(best) if start <= p < start + count][:min(128, count)]
                assert len(chunks) == len(periods) <= min(128, count)
                for p, (digest, msg) in zip(periods, chunks):
                    got = wire.decode_updates([msg], "update", digest_fork[digest], lib=v.lib)
                    PB.assert_rows_equal(got, down, rows=[best[p]])
                    att = int.from_bytes(got.att_beacon[0, :8].tobytes(), "little")
                    assert c.cfg.compute_sync_committee_period_at_slot(att) == p
                    assert digest == wire.fork_digest(c.cfg.compute_fork_version(c.cfg.compute_epoch_at_slot(att)), gvr)
        finally:
            rb.free()


# ------------------------------------------------------------------ 8. fork digests (CPU)
def check_fork_digests():
    gvr = bytes.fromhex("4b363db94e286120d76eb905340fdd4e54bfe9f06bf33ff6cf5ad27f511bfe95")  # mainnet
    exp = ["b5303f2a", "afcaaba0", "4a26c58b", "bba4da96", "6a95a1a9"]
    from lcv.config import MAINNET
    assert [wire.fork_digest(ver, gvr).hex() for ver in MAINNET.fork_versions()] == exp
    with pytest.raises(ValueError):
        wire.fork_digest(b"\x00" * 3, gvr)


# ------------------------------------------------------------------ 9. refusals and the stage
def check_refusals_and_stage(v):
    import ctypes as C
    from lcv._native import LcvError, ptr
    from lcv.device import EncodedMessages
    n = 5
    b = rows_for(n, "deneb")
    rb = v.upload(b)
    lib, ctx = v.lib, v.ctx
    try:
        def outs():
            e = EncodedMessages.empty(n, PITCH["update"], fill=0xEE)
            for a in (e.length, e.fork, e.version, e.status):
                a.view(np.uint8)[...] = 0xEE
            return e

        def untouched(e):
            return all((np.asarray(a).view(np.uint8) == 0xEE).all() for a in (e.buf, e.length, e.fork, e.version, e.status))
        rows = np.array([0, 4, 5, 1], np.uint32)
        e = outs()
        args = [ctx, rb.handle, None, 0, 0, 0, ptr(e.buf), ptr(e.length, C.c_uint32), ptr(e.fork), ptr(e.version), ptr(e.status)]
        for k in (0, 1, 6, 7, 8, 9, 10):
            a = list(args)
            a[k] = None
            assert lib.lcv_batch_encode(*a) == -1
        assert b"null" in lib.lcv_last_error(ctx)
        for kind, fork in ((3, 0), (-1, 0), (0, 3), (0, -2)):
            a = list(args)
            a[4], a[5] = kind, fork
            assert lib.lcv_batch_encode(*a) == -1
        a = list(args)
        a[2], a[3] = ptr(rows, C.c_uint32), 4
        assert lib.lcv_batch_encode(*a) == -1 and b"rows[2] = 5" in lib.lcv_last_error(ctx)
        hb, keep = b.to_c()
        hargs = [ctx, C.byref(hb), 0, 0] + args[6:]
        for k in (0, 1, 4, 5, 6, 7, 8):
            a = list(hargs)
            a[k] = None
            assert lib.lcv_encode_updates(*a) == -1
        for kind, fork in ((3, 0), (0, 3)):
            a = list(hargs)
            a[2], a[3] = kind, fork
            assert lib.lcv_encode_updates(*a) == -1
        hb.sync_bits = None
        assert lib.lcv_encode_updates(*([ctx, C.byref(hb)] + hargs[2:])) == -1
        assert untouched(e)
        with pytest.raises(LcvError, match="status -1"):
            v.encode_resident(rb, "update", "deneb", rows=[0, n])
        # no message: fine, nothing written
        a = list(args)
        a[2], a[3] = ptr(rows, C.c_uint32), 0
        assert lib.lcv_batch_encode(*a) == 0 and untouched(e)
        assert lib.lcv_encode_pitch(3) == 0 and lib.lcv_encode_pitch(-1) == 0
        # the stage
        names = [lib.lcv_stage_name(i).decode() for i in range(32)]
        assert names[:22] == ["nsc_htr", "pre_checks", "h2c_sswu", "hash_to_g2", "sig_decode", "g1_aggregate", "miller_loop",
                              "final_exp", "verdict", "setup", "miller_lines", "miller_lines_sig", "signing_root",
                              "store_rank", "store_fold", "produce_views", "produce_rows", "dedup_gather", "rlc_scale",
                              "rlc_product", "rlc_spread", "rlc_retry"]
        assert names[22] == "wire_encode" and names[23] == "?"
        v.encode_resident(rb, "update", "deneb")
        t = v.last_timings()
        assert t["wire_encode"] > 0 and t["produce_rows"] == 0 and t["pre_checks"] == 0
    finally:
        rb.free()
