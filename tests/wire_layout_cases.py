"""Every ExecutionPayloadHeader field lands where include/lcv.h says: cases shared by test_wire_layout_hostsim.py
(host simulation of the kernels' code) and test_wire_layout_gpu.py (the MI355X).

The C++ decoders and the encoder take the containers from one table (csrc/lcv_wire_layout.hpp), so their agreement
with each other says nothing about that table.  Here the messages are serialised by the oracle's SSZ containers, every
field of both headers filled with a byte value of its own, and the offsets inside the 832-byte execution record are
literals taken from the comment in include/lcv.h.  Per kind and fork (Deneb, Capella) four messages: extra_data of 0,
1, 31 and 32 bytes in the attested header (the finalized header then starts at the residues 0, 1, 3, 0 modulo 4: the
dword and the byte path of the kernels' moves) and of 1, 31, 32, 0 bytes in the finalized one.  None is longer than
27 KB.
"""
from functools import lru_cache

import numpy as np

import helpers as H
import wire_encode_cases as WE

from lcv import wire
from oracle import spec as S
from oracle.ssz import Container, serialize

KINDS, FORKS = WE.KINDS, ("deneb", "capella")
EXTRA_LENS = (0, 1, 31, 32)
# SSZ field order: (name, offset in the 832-byte record, bytes) — the comment "Packed ExecutionPayloadHeader record"
# of include/lcv.h: leaf chunks of 32 bytes in field order, leaf 4 unused, logs_bloom at 544, the length word at 800
EXEC_FIELDS = (("parent_hash", 0, 32), ("fee_recipient", 32, 20), ("state_root", 64, 32), ("receipts_root", 96, 32),
               ("logs_bloom", 544, 256), ("prev_randao", 160, 32), ("block_number", 192, 8), ("gas_limit", 224, 8),
               ("gas_used", 256, 8), ("timestamp", 288, 8), ("extra_data", 320, None), ("base_fee_per_gas", 352, 32),
               ("block_hash", 384, 32), ("transactions_root", 416, 32), ("withdrawals_root", 448, 32),
               ("blob_gas_used", 480, 8), ("excess_blob_gas", 512, 8))
EXTRA_LEN_AT = 800
INTS = ("block_number", "gas_limit", "gas_used", "timestamp", "base_fee_per_gas", "blob_gas_used", "excess_blob_gas")
ROW = 0  # the golden row the other fields come from


def fill(header, field):
    """The byte value of field `field` of header 0 (attested) or 1 (finalized): 1 .. 34, each once."""
    return 1 + len(EXEC_FIELDS) * header + field


def containers(execution_cls):
    class Header(Container):
        beacon: S.BeaconBlockHeader
        execution: execution_cls
        execution_branch: S.ExecutionBranch

    class Update(Container):
        attested_header: Header
        next_sync_committee: S.SyncCommittee
        next_sync_committee_branch: S.NextSyncCommitteeBranch
        finalized_header: Header
        finality_branch: S.FinalityBranch
        sync_aggregate: S.SyncAggregate
        signature_slot: S.Slot

    class FinalityUpdate(Container):
        attested_header: Header
        finalized_header: Header
        finality_branch: S.FinalityBranch
        sync_aggregate: S.SyncAggregate
        signature_slot: S.Slot

    class OptimisticUpdate(Container):
        attested_header: Header
        sync_aggregate: S.SyncAggregate
        signature_slot: S.Slot

    return Header, {"update": Update, "finality": FinalityUpdate, "optimistic": OptimisticUpdate}


def exec_header(cls, header, elen):
    names = {n for n, _ in cls._fields}
    kw = {}
    for f, (name, _, size) in enumerate(EXEC_FIELDS):
        if name in names:
            data = bytes([fill(header, f)]) * (elen if size is None else size)
            kw[name] = int.from_bytes(data, "little") if name in INTS else data
    return cls(**kw)


def expected_record(header, fork, elen):
    rec = np.zeros(832, np.uint8)
    for f, (name, off, size) in enumerate(EXEC_FIELDS):
        if fork == "capella" and name in ("blob_gas_used", "excess_blob_gas"):
            continue
        rec[off:off + (elen if size is None else size)] = fill(header, f)
    rec[EXTRA_LEN_AT:EXTRA_LEN_AT + 4] = np.frombuffer(int(elen).to_bytes(4, "little"), np.uint8)
    return rec


@lru_cache(maxsize=None)
def messages(kind, fork):
    """(the four messages, their (attested, finalized) extra_data lengths)."""
    execution_cls = S.ExecutionPayloadHeader if fork == "deneb" else S.CapellaExecutionPayloadHeader
    header_cls, kinds = containers(execution_cls)
    u = H.update_from(WE.packed(), ROW)
    msgs, lens = [], []
    for j, la in enumerate(EXTRA_LENS):
        lf = EXTRA_LENS[(j + 1) % 4]
        att = header_cls(beacon=u.attested_header.beacon, execution=exec_header(execution_cls, 0, la),
                         execution_branch=u.attested_header.execution_branch)
        fin = header_cls(beacon=u.finalized_header.beacon, execution=exec_header(execution_cls, 1, lf),
                         execution_branch=u.finalized_header.execution_branch)
        kw = dict(attested_header=att, sync_aggregate=u.sync_aggregate, signature_slot=u.signature_slot)
        if kind != "optimistic":
            kw.update(finalized_header=fin, finality_branch=u.finality_branch)
        if kind == "update":
            kw.update(next_sync_committee=u.next_sync_committee, next_sync_committee_branch=u.next_sync_committee_branch)
        msgs.append(serialize(kinds[kind](**kw)))
        lens.append((la, lf))
    assert len(msgs) == 4 and max(len(m) for m in msgs) <= 27000
    return tuple(msgs), tuple(lens)


def assert_rows(b, kind, fork, lens, what):
    p = WE.packed()
    zero = np.zeros(832, np.uint8)
    for j, (la, lf) in enumerate(lens):
        assert np.array_equal(b.att_exec[j], expected_record(0, fork, la)), (what, kind, fork, j, "attested record")
        exp_fin = expected_record(1, fork, lf) if kind != "optimistic" else zero
        assert np.array_equal(b.fin_exec[j], exp_fin), (what, kind, fork, j, "finalized record")
        for col in ("att_beacon", "att_branch", "sync_bits", "sync_signature", "signature_slot"):
            assert np.array_equal(getattr(b, col)[j], getattr(p, col)[ROW]), (what, col, j)
        for col in ("fin_beacon", "fin_branch", "finality_branch"):
            exp = getattr(p, col)[ROW] if kind != "optimistic" else np.zeros_like(getattr(p, col)[ROW])
            assert np.array_equal(getattr(b, col)[j], exp), (what, col, j)
        committee = b.nsc_pool[int(b.nsc_index[j])]
        if kind == "update":
            assert np.array_equal(b.nsc_branch[j], p.nsc_branch[ROW]), (what, j)
            assert np.array_equal(committee, p.nsc_pool[int(p.nsc_index[ROW])]), (what, j)
        else:
            assert not b.nsc_branch[j].any() and not committee.any(), (what, j)


def check_fields(v, kind, fork):
    """Host decoder, device decoder and device encoder of verifier v's library over the oracle's messages."""
    msgs, lens = messages(kind, fork)
    host = wire.decode_updates(list(msgs), kind, fork, lib=v.lib)
    assert_rows(host, kind, fork, lens, "host decoder")
    rb, ok = v.decode_resident(list(msgs), kind, fork)
    try:
        assert ok.all()
        assert_rows(v.download(rb), kind, fork, lens, "device decoder")
        enc = v.encode_resident(rb, kind, fork)
    finally:
        rb.free()
    WE.assert_encoded(enc, list(msgs), WE.FORKS.index(fork))
