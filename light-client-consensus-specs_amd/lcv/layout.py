"""Byte layouts of the packed (structure-of-arrays) update batch, and packing of spec objects.

The drop-ins (`lcv.sync_protocol.validate_light_client_update`, ...) accept the reference's own
container objects (`LightClientUpdate`, `LightClientHeader`, `SyncCommittee`,
reference sync-protocol.md:96-133) by duck typing: anything with the same attribute names and
SSZ-serialisable values works (eth2spec/remerkleable objects, or the test oracle's containers).
They are packed here into the row layouts of include/lcv.h:

  beacon      112 B  SSZ BeaconBlockHeader (slot u64, proposer_index u64, parent_root, state_root,
                     body_root)
  execution   832 B  17 leaf chunks of ExecutionPayloadHeader in field order (leaf 4 = logs_bloom
                     is unused/zero, leaf 10 = extra_data zero padded), logs_bloom at 544,
                     extra_data length u32 at 800; all-zero <=> ExecutionPayloadHeader()
  branch      n x 32 B (execution 4, next_sync_committee 5, finality 6)
  bits        64 B   SSZ Bitvector[512]
  signature   96 B   compressed G2
  committee   24624 B SSZ SyncCommittee (512 x 48 B pubkeys, 48 B aggregate_pubkey)

No BLS or SHA arithmetic happens here: packing is pure byte plumbing (the device hashes).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Iterable, List, Sequence, Tuple

import numpy as np

SYNC_COMMITTEE_SIZE = 512
PUBKEY_BYTES = 48
SIGNATURE_BYTES = 96
SYNC_COMMITTEE_BYTES = SYNC_COMMITTEE_SIZE * PUBKEY_BYTES + PUBKEY_BYTES  # 24624
BEACON_BYTES = 112
EXEC_BYTES = 832
EXEC_BLOOM_OFF = 544
EXEC_EXTRALEN_OFF = 800
EXEC_BRANCH_BYTES = 128
NSC_BRANCH_BYTES = 160
FINALITY_BRANCH_BYTES = 192
BITS_BYTES = 64
MAX_EXTRA_DATA_BYTES = 32

# ExecutionPayloadHeader field order (Deneb: 17 fields; Capella: the first 15)
EXEC_FIELDS = ("parent_hash", "fee_recipient", "state_root", "receipts_root", "logs_bloom", "prev_randao",
               "block_number", "gas_limit", "gas_used", "timestamp", "extra_data", "base_fee_per_gas",
               "block_hash", "transactions_root", "withdrawals_root", "blob_gas_used", "excess_blob_gas")
_U64_FIELDS = {"block_number", "gas_limit", "gas_used", "timestamp", "blob_gas_used", "excess_blob_gas"}


def _b(x) -> bytes:
    return bytes(x)


def pack_beacon(beacon) -> bytes:
    """SSZ serialisation of BeaconBlockHeader (fixed 112 bytes)."""
    out = (int(beacon.slot).to_bytes(8, "little") + int(beacon.proposer_index).to_bytes(8, "little")
           + _b(beacon.parent_root) + _b(beacon.state_root) + _b(beacon.body_root))
    if len(out) != BEACON_BYTES:
        raise ValueError("malformed BeaconBlockHeader")
    return out


def pack_execution(execution) -> bytes:
    """Execution record (832 B) of a Deneb or Capella ExecutionPayloadHeader (missing Deneb blob
    fields of a Capella header read as 0)."""
    rec = bytearray(EXEC_BYTES)
    for k, name in enumerate(EXEC_FIELDS):
        v = getattr(execution, name, 0)
        if name == "logs_bloom":
            bloom = _b(v)
            if len(bloom) != 256:
                raise ValueError("logs_bloom must be 256 bytes")
            rec[EXEC_BLOOM_OFF:EXEC_BLOOM_OFF + 256] = bloom
        elif name == "extra_data":
            ed = _b(v)
            if len(ed) > MAX_EXTRA_DATA_BYTES:
                raise ValueError("extra_data longer than 32 bytes")
            rec[32 * k:32 * k + len(ed)] = ed
            rec[EXEC_EXTRALEN_OFF:EXEC_EXTRALEN_OFF + 4] = len(ed).to_bytes(4, "little")
        elif name in _U64_FIELDS:
            rec[32 * k:32 * k + 8] = int(v).to_bytes(8, "little")
        elif name == "base_fee_per_gas":
            rec[32 * k:32 * k + 32] = int(v).to_bytes(32, "little")
        else:
            b = _b(v)
            if len(b) > 32:
                raise ValueError(f"{name} longer than 32 bytes")
            rec[32 * k:32 * k + len(b)] = b
    return bytes(rec)


def pack_branch(branch, depth: int) -> bytes:
    items = [_b(x) for x in branch]
    if len(items) != depth or any(len(x) != 32 for x in items):
        raise ValueError(f"branch must be {depth} x 32 bytes")
    return b"".join(items)


def pack_header(header) -> Tuple[bytes, bytes, bytes]:
    """LightClientHeader (reference sync-protocol.md:96-101) -> (beacon, execution, branch) rows."""
    return pack_beacon(header.beacon), pack_execution(header.execution), pack_branch(header.execution_branch, 4)


def pack_sync_committee(sc) -> bytes:
    pks = [_b(p) for p in sc.pubkeys]
    if len(pks) != SYNC_COMMITTEE_SIZE or any(len(p) != PUBKEY_BYTES for p in pks):
        raise ValueError("SyncCommittee must hold 512 x 48-byte pubkeys")
    agg = _b(sc.aggregate_pubkey)
    if len(agg) != PUBKEY_BYTES:
        raise ValueError("aggregate_pubkey must be 48 bytes")
    return b"".join(pks) + agg


def pack_bits(bits: Sequence) -> bytes:
    """SSZ Bitvector[512]: bit i -> byte i // 8, bit i % 8."""
    arr = np.asarray([bool(x) for x in bits], dtype=np.uint8)
    if arr.shape != (SYNC_COMMITTEE_SIZE,):
        raise ValueError("sync_committee_bits must have 512 entries")
    return np.packbits(arr, bitorder="little").tobytes()


def unpack_bits(b64: bytes) -> List[bool]:
    return [bool(x) for x in np.unpackbits(np.frombuffer(bytes(b64), np.uint8), bitorder="little")]


# ------------------------------------------------------------------ the inverse: packed rows -> duck-typed objects
def unpack_beacon(b: bytes):
    b = bytes(b)
    return SimpleNamespace(slot=int.from_bytes(b[0:8], "little"), proposer_index=int.from_bytes(b[8:16], "little"),
                           parent_root=b[16:48], state_root=b[48:80], body_root=b[80:112])


def unpack_execution(rec: bytes):
    rec = bytes(rec)
    out = {}
    for k, name in enumerate(EXEC_FIELDS):
        chunk = rec[32 * k:32 * k + 32]
        if name == "logs_bloom":
            out[name] = rec[EXEC_BLOOM_OFF:EXEC_BLOOM_OFF + 256]
        elif name == "extra_data":
            out[name] = chunk[:int.from_bytes(rec[EXEC_EXTRALEN_OFF:EXEC_EXTRALEN_OFF + 4], "little")]
        elif name in _U64_FIELDS:
            out[name] = int.from_bytes(chunk[:8], "little")
        elif name == "base_fee_per_gas":
            out[name] = int.from_bytes(chunk, "little")
        elif name == "fee_recipient":
            out[name] = chunk[:20]
        else:
            out[name] = chunk
    return SimpleNamespace(**out)


def unpack_header(beacon: bytes, execution: bytes, branch: bytes):
    branch = bytes(branch)
    return SimpleNamespace(beacon=unpack_beacon(beacon), execution=unpack_execution(execution),
                           execution_branch=[branch[32 * k:32 * k + 32] for k in range(4)])


def unpack_sync_committee(sc: bytes):
    sc = bytes(sc)
    return SimpleNamespace(pubkeys=[sc[PUBKEY_BYTES * j:PUBKEY_BYTES * (j + 1)] for j in range(SYNC_COMMITTEE_SIZE)],
                           aggregate_pubkey=sc[SYNC_COMMITTEE_SIZE * PUBKEY_BYTES:])


def unpack_update(packed, i: int):
    """Row i of a PackedUpdates batch as a duck-typed LightClientUpdate (the reference's field names,
    sync-protocol.md:120-133): the inverse of packing — pack_updates([unpack_update(p, i)]) is row i again."""
    t = lambda a: np.asarray(a[i]).tobytes()  # noqa: E731
    nbr, fbr = t(packed.nsc_branch), t(packed.finality_branch)
    return SimpleNamespace(
        attested_header=unpack_header(t(packed.att_beacon), t(packed.att_exec), t(packed.att_branch)),
        next_sync_committee=unpack_sync_committee(packed.nsc_pool[int(packed.nsc_index[i])].tobytes()),
        next_sync_committee_branch=[nbr[32 * k:32 * k + 32] for k in range(5)],
        finalized_header=unpack_header(t(packed.fin_beacon), t(packed.fin_exec), t(packed.fin_branch)),
        finality_branch=[fbr[32 * k:32 * k + 32] for k in range(6)],
        sync_aggregate=SimpleNamespace(sync_committee_bits=unpack_bits(t(packed.sync_bits)),
                                       sync_committee_signature=t(packed.sync_signature)),
        signature_slot=int(packed.signature_slot[i]))
