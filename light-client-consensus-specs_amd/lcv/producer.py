"""Producer side of the light-client data: full-node.md's helper and
derivation functions over a sparse view of the beacon state and blocks.

    compute_merkle_proof                    full-node.md:35-38 (declared there without a body)
    block_to_light_client_header            full-node.md:43-89
    create_light_client_bootstrap           full-node.md:105-121
    create_light_client_update              full-node.md:138-188
    create_light_client_finality_update     full-node.md:197-205
    create_light_client_optimistic_update   full-node.md:213-219

A full node holds whole BeaconStates (28 fields, millions of validators); light-client data reads
five of them.  `BeaconStateView` keeps those five explicitly (slot, latest_block_header,
finalized_checkpoint, current / next sync committee) and every other field by its hash_tree_root, so
hash_tree_root(state) and the three state proofs (gindices 54, 55, 105) are exact for the real
state.  `BeaconBlockView` likewise keeps a block's header fields, its body's sync_aggregate and
execution payload (as the 832-byte execution record of include/lcv.h, i.e. the payload's header form:
transactions_root / withdrawals_root in place of the lists, which is what its hash_tree_root and
block_to_light_client_header use) and the other body fields by root.  Outputs are the packed rows of
include/lcv.h (`UpdateRow`, `BootstrapRow`; `pack_updates` -> PackedUpdates for the verifier and
lcv.wire.encode_updates / encode_bootstrap for the wire).  The asserts are the reference's.

The per-object functions are host code (hashlib SHA-256), pinned against the reference's exec'd full-node.md
blocks (tests/golden/producer.npz); the 10^4-row synthetic batches of lcv.synth are built through them.  A
backfill over historic blocks (full-node.md:96, :184-188) takes the batched twins at the end of this module
instead: `pack_views` turns lists of views into column tables once, and `create_light_client_updates` /
`Verifier.create_updates_resident` derive every row on the device (csrc/lcv_producer.hpp), with
the per-object functions as their yardstick.

Views are treated as immutable once their roots are first used (roots are memoised per instance;
`dataclasses.replace` makes a fresh view).
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import config as _config
from . import layout as L
from .config import NetworkConfig

# generalized indices (sync-protocol.md:78-81)
FINALIZED_ROOT_GINDEX = 105
CURRENT_SYNC_COMMITTEE_GINDEX = 54
NEXT_SYNC_COMMITTEE_GINDEX = 55
EXECUTION_PAYLOAD_GINDEX = 25
GENESIS_SLOT = 0
MIN_SYNC_COMMITTEE_PARTICIPANTS = 1

STATE_FIELDS = 28        # Deneb BeaconState (Altair 24 .. Deneb 28: one 32-leaf tree either way)
BODY_FIELDS = 12         # Deneb BeaconBlockBody (16-leaf tree)
F_SLOT, F_LATEST_BLOCK_HEADER, F_FINALIZED_CHECKPOINT, F_CURRENT_SC, F_NEXT_SC = 2, 4, 20, 22, 23
B_SYNC_AGGREGATE, B_EXECUTION_PAYLOAD = 8, 9


def sha256(b: bytes, _h=hashlib.sha256) -> bytes:
    return _h(b).digest()


ZERO_HASHES = [bytes(32)]
for _ in range(40):
    ZERO_HASHES.append(sha256(ZERO_HASHES[-1] + ZERO_HASHES[-1]))


# ------------------------------------------------------------------ SSZ merkleization (host)
def merkleize(chunks: Sequence[bytes], depth: int) -> bytes:
    layer = list(chunks)
    assert len(layer) <= 1 << depth
    if not layer:
        return ZERO_HASHES[depth]
    for d in range(depth):
        if len(layer) % 2:
            layer.append(ZERO_HASHES[d])
        layer = [sha256(layer[i] + layer[i + 1]) for i in range(0, len(layer), 2)]
    return layer[0]


def merkle_layers(chunks: Sequence[bytes], depth: int) -> List[List[bytes]]:
    """Every layer of merkleize(chunks, depth), leaves first (odd layers padded with the zero subtree)."""
    layers, layer = [], list(chunks)
    for d in range(depth):
        if len(layer) % 2:
            layer.append(ZERO_HASHES[d])
        layers.append(layer)
        layer = [sha256(layer[i] + layer[i + 1]) for i in range(0, len(layer), 2)]
    layers.append(layer)
    return layers


def layers_path(layers: List[List[bytes]], index: int) -> List[bytes]:
    out = []
    for d, layer in enumerate(layers[:-1]):
        sib = index ^ 1
        out.append(layer[sib] if sib < len(layer) else ZERO_HASHES[d])
        index >>= 1
    return out


def merkle_path(chunks: Sequence[bytes], depth: int, index: int) -> List[bytes]:
    """Sibling roots from leaf `index` of merkleize(chunks, depth) up to the root (bottom-up)."""
    return layers_path(merkle_layers(chunks, depth), index)


def fold_branch(leaf: bytes, branch: Sequence[bytes], index: int) -> bytes:
    v = leaf
    for i, b in enumerate(branch):
        v = sha256(b + v) if (index >> i) & 1 else sha256(v + b)
    return v


def u64_chunk(v: int) -> bytes:
    return int(v).to_bytes(8, "little") + bytes(24)


def htr_beacon(b112: bytes) -> bytes:
    """hash_tree_root(BeaconBlockHeader) of its 112-byte SSZ."""
    chunks = [b112[0:8] + bytes(24), b112[8:16] + bytes(24), b112[16:48], b112[48:80], b112[80:112]]
    return merkleize(chunks, 3)


def htr_exec_record(rec: bytes, deneb: bool) -> bytes:
    """hash_tree_root of the ExecutionPayloadHeader (= of its ExecutionPayload) held in an 832-byte
    execution record (Deneb 17 fields, Capella 15)."""
    bloom = rec[L.EXEC_BLOOM_OFF:L.EXEC_BLOOM_OFF + 256]
    bloom_root = merkleize([bloom[32 * k:32 * k + 32] for k in range(8)], 3)
    ext_len = int.from_bytes(rec[L.EXEC_EXTRALEN_OFF:L.EXEC_EXTRALEN_OFF + 4], "little")
    extra_root = sha256(rec[320:352] + ext_len.to_bytes(8, "little") + bytes(24))
    nf = 17 if deneb else 15
    leaves = [bloom_root if k == 4 else extra_root if k == 10 else rec[32 * k:32 * k + 32] for k in range(nf)]
    return merkleize(leaves, 5 if deneb else 4)


def htr_pubkey(pk: bytes) -> bytes:
    return sha256(pk[:32] + pk[32:48] + bytes(16))


def htr_sync_committee(sc: bytes) -> bytes:
    roots = [htr_pubkey(sc[48 * j:48 * j + 48]) for j in range(L.SYNC_COMMITTEE_SIZE)]
    return sha256(merkleize(roots, 9) + htr_pubkey(sc[L.SYNC_COMMITTEE_SIZE * 48:]))


def htr_sync_aggregate(bits64: bytes, sig96: bytes) -> bytes:
    return sha256(sha256(bits64[:32] + bits64[32:64]) + merkleize([sig96[0:32], sig96[32:64], sig96[64:96]], 2))


def beacon_header(slot: int, proposer_index: int, parent_root: bytes, state_root: bytes, body_root: bytes) -> bytes:
    """112-byte SSZ BeaconBlockHeader."""
    b = (int(slot).to_bytes(8, "little") + int(proposer_index).to_bytes(8, "little") + bytes(parent_root)
         + bytes(state_root) + bytes(body_root))
    assert len(b) == L.BEACON_BYTES
    return b


# ------------------------------------------------------------------ sparse views
_SC_ROOTS: Dict[bytes, bytes] = {}


def _committee_root(sc: bytes) -> bytes:
    """hash_tree_root(SyncCommittee), memoised by content (a committee serves a whole period)."""
    key = sha256(sc)
    r = _SC_ROOTS.get(key)
    if r is None:
        if len(_SC_ROOTS) > (1 << 16):
            _SC_ROOTS.clear()
        r = _SC_ROOTS[key] = htr_sync_committee(sc)
    return r


@dataclass
class BeaconStateView:
    """BeaconState: the fields light-client data reads, plus every field's hash_tree_root.

    field_roots: (28, 32) roots of all fields in BeaconState order; the entries of the explicit fields
    (slot 2, latest_block_header 4, finalized_checkpoint 20, current / next_sync_committee 22 / 23)
    are recomputed from them."""
    slot: int
    latest_block_header: bytes                 # 112 B SSZ
    finalized_checkpoint_epoch: int
    finalized_checkpoint_root: bytes
    current_sync_committee: bytes              # 24,624 B SSZ
    next_sync_committee: bytes
    field_roots: np.ndarray = field(default_factory=lambda: np.zeros((STATE_FIELDS, 32), np.uint8))
    _memo: Optional[list] = field(default=None, init=False, repr=False, compare=False)  # tree layers

    def chunks(self) -> List[bytes]:
        return list(self._layers()[0][:STATE_FIELDS])

    def _layers(self) -> List[List[bytes]]:
        if self._memo is None:
            self._memo = merkle_layers(self._chunks(), 5)
        return self._memo

    def _chunks(self) -> List[bytes]:
        roots = [bytes(r) for r in np.asarray(self.field_roots, np.uint8).reshape(-1, 32)]
        assert len(roots) == STATE_FIELDS
        roots[F_SLOT] = u64_chunk(self.slot)
        roots[F_LATEST_BLOCK_HEADER] = htr_beacon(self.latest_block_header)
        roots[F_FINALIZED_CHECKPOINT] = sha256(u64_chunk(self.finalized_checkpoint_epoch)
                                               + bytes(self.finalized_checkpoint_root))
        roots[F_CURRENT_SC] = _committee_root(bytes(self.current_sync_committee))
        roots[F_NEXT_SC] = _committee_root(bytes(self.next_sync_committee))
        return roots

    def hash_tree_root(self) -> bytes:
        return self._layers()[-1][0]

    def merkle_proof(self, gindex: int) -> List[bytes]:
        layers = self._layers()
        if gindex in (CURRENT_SYNC_COMMITTEE_GINDEX, NEXT_SYNC_COMMITTEE_GINDEX):
            return layers_path(layers, gindex - 32)
        if gindex == FINALIZED_ROOT_GINDEX:  # finalized_checkpoint (field 20) -> its `root` (child 1)
            return [u64_chunk(self.finalized_checkpoint_epoch)] + layers_path(layers, F_FINALIZED_CHECKPOINT)
        raise ValueError(f"no proof for generalized index {gindex} of BeaconState")


@dataclass
class BeaconBlockView:
    """SignedBeaconBlock: the header fields, the body's sync_aggregate and execution payload, and
    every body field's hash_tree_root.

    execution: the payload's 832-byte execution record (header form), needed from Capella on;
    execution_deneb: whether it is a Deneb payload (17 fields) or Capella (15).  body_roots: (12, 32)
    roots of the body fields in BeaconBlockBody order; sync_aggregate (8) and, with an execution
    record, execution_payload (9) are recomputed."""
    slot: int
    proposer_index: int
    parent_root: bytes
    state_root: bytes
    sync_committee_bits: bytes                 # 64 B
    sync_committee_signature: bytes            # 96 B
    execution: Optional[bytes] = None
    execution_deneb: bool = True
    body_roots: np.ndarray = field(default_factory=lambda: np.zeros((BODY_FIELDS, 32), np.uint8))
    _memo: Optional[tuple] = field(default=None, init=False, repr=False, compare=False)  # (body layers, header)

    def _body(self) -> tuple:
        if self._memo is None:
            layers = merkle_layers(self._body_chunks(), 4)
            self._memo = (layers, beacon_header(self.slot, self.proposer_index, self.parent_root, self.state_root,
                                                layers[-1][0]))
        return self._memo

    def body_chunks(self) -> List[bytes]:
        return list(self._body()[0][0][:BODY_FIELDS])

    def _body_chunks(self) -> List[bytes]:
        roots = [bytes(r) for r in np.asarray(self.body_roots, np.uint8).reshape(-1, 32)]
        assert len(roots) == BODY_FIELDS
        roots[B_SYNC_AGGREGATE] = htr_sync_aggregate(bytes(self.sync_committee_bits), bytes(self.sync_committee_signature))
        if self.execution is not None:
            roots[B_EXECUTION_PAYLOAD] = htr_exec_record(bytes(self.execution), self.execution_deneb)
        return roots

    def body_root(self) -> bytes:
        return self.header()[80:112]

    def header(self) -> bytes:
        """BeaconBlockHeader of the block (state_root as the block carries it)."""
        return self._body()[1]

    def hash_tree_root(self) -> bytes:
        """hash_tree_root(block.message) == hash_tree_root of its BeaconBlockHeader."""
        return htr_beacon(self.header())

    def body_merkle_proof(self, gindex: int) -> List[bytes]:
        if gindex != EXECUTION_PAYLOAD_GINDEX:
            raise ValueError(f"no proof for generalized index {gindex} of BeaconBlockBody")
        return layers_path(self._body()[0], gindex - 16)


def compute_merkle_proof(obj, index: int) -> List[bytes]:
    """full-node.md:35-38: the Merkle proof of the node at generalized index `index` (bottom-up)."""
    if isinstance(obj, BeaconStateView):
        return obj.merkle_proof(int(index))
    if isinstance(obj, BeaconBlockView):   # a block's body (the call site passes block.message.body)
        return obj.body_merkle_proof(int(index))
    raise TypeError(f"compute_merkle_proof: unsupported object {type(obj).__name__}")


# ------------------------------------------------------------------ outputs (packed rows)
@dataclass
class HeaderRow:
    """LightClientHeader as include/lcv.h rows."""
    beacon: bytes       # 112
    execution: bytes    # 832
    execution_branch: bytes  # 128


EMPTY_HEADER = HeaderRow(bytes(L.BEACON_BYTES), bytes(L.EXEC_BYTES), bytes(L.EXEC_BRANCH_BYTES))
EMPTY_SYNC_COMMITTEE = bytes(L.SYNC_COMMITTEE_BYTES)


@dataclass
class UpdateRow:
    """LightClientUpdate (sync-protocol.md:120-133); defaults = the reference's LightClientUpdate()."""
    attested_header: HeaderRow = EMPTY_HEADER
    next_sync_committee: bytes = EMPTY_SYNC_COMMITTEE
    next_sync_committee_branch: bytes = bytes(L.NSC_BRANCH_BYTES)
    finalized_header: HeaderRow = EMPTY_HEADER
    finality_branch: bytes = bytes(L.FINALITY_BRANCH_BYTES)
    sync_committee_bits: bytes = bytes(L.BITS_BYTES)
    sync_committee_signature: bytes = bytes(L.SIGNATURE_BYTES)
    signature_slot: int = 0


@dataclass
class BootstrapRow:
    """LightClientBootstrap (sync-protocol.md:109-115)."""
    header: HeaderRow
    current_sync_committee: bytes
    current_sync_committee_branch: bytes  # 160


def block_to_light_client_header(block: BeaconBlockView, cfg: Optional[NetworkConfig] = None) -> HeaderRow:
    """full-node.md:43-89."""
    cfg = cfg or _config.active()
    epoch = cfg.compute_epoch_at_slot(block.slot)
    if epoch >= cfg.CAPELLA_FORK_EPOCH:
        if block.execution is None:
            raise ValueError("a Capella-or-later block needs its execution payload")
        rec = bytearray(block.execution)
        if epoch < cfg.DENEB_FORK_EPOCH:   # the Deneb blob fields exist only from Deneb on
            rec[480:488] = bytes(8)
            rec[512:520] = bytes(8)
        branch = b"".join(compute_merkle_proof(block, EXECUTION_PAYLOAD_GINDEX))
        execution = bytes(rec)
    else:   # pre-Capella: no execution data in light-client headers
        execution, branch = bytes(L.EXEC_BYTES), bytes(L.EXEC_BRANCH_BYTES)
    return HeaderRow(block.header(), execution, branch)


def _state_header_root(state: BeaconStateView) -> bytes:
    """hash_tree_root of state.latest_block_header with state_root = hash_tree_root(state)."""
    h = state.latest_block_header
    return htr_beacon(h[:48] + state.hash_tree_root() + h[80:])


def create_light_client_bootstrap(state: BeaconStateView, block: BeaconBlockView,
                                  cfg: Optional[NetworkConfig] = None) -> BootstrapRow:
    """full-node.md:105-121."""
    cfg = cfg or _config.active()
    assert cfg.compute_epoch_at_slot(state.slot) >= cfg.ALTAIR_FORK_EPOCH
    assert state.slot == int.from_bytes(state.latest_block_header[:8], "little")
    assert _state_header_root(state) == block.hash_tree_root()
    return BootstrapRow(header=block_to_light_client_header(block, cfg),
                        current_sync_committee=bytes(state.current_sync_committee),
                        current_sync_committee_branch=b"".join(
                            compute_merkle_proof(state, CURRENT_SYNC_COMMITTEE_GINDEX)))


def create_light_client_update(state: BeaconStateView, block: BeaconBlockView, attested_state: BeaconStateView,
                               attested_block: BeaconBlockView, finalized_block: Optional[BeaconBlockView],
                               cfg: Optional[NetworkConfig] = None) -> UpdateRow:
    """full-node.md:138-188."""
    cfg = cfg or _config.active()
    assert cfg.compute_epoch_at_slot(attested_state.slot) >= cfg.ALTAIR_FORK_EPOCH
    assert sum(bin(b).count("1") for b in bytes(block.sync_committee_bits)) >= MIN_SYNC_COMMITTEE_PARTICIPANTS

    assert state.slot == int.from_bytes(state.latest_block_header[:8], "little")
    assert _state_header_root(state) == block.hash_tree_root()
    update_signature_period = cfg.compute_sync_committee_period_at_slot(block.slot)

    assert attested_state.slot == int.from_bytes(attested_state.latest_block_header[:8], "little")
    att_root = attested_block.hash_tree_root()
    assert _state_header_root(attested_state) == att_root == bytes(block.parent_root)
    update_attested_period = cfg.compute_sync_committee_period_at_slot(attested_block.slot)

    update = UpdateRow()
    update.attested_header = block_to_light_client_header(attested_block, cfg)

    # next_sync_committee is only useful if the message is signed by the current sync committee
    if update_attested_period == update_signature_period:
        update.next_sync_committee = bytes(attested_state.next_sync_committee)
        update.next_sync_committee_branch = b"".join(compute_merkle_proof(attested_state, NEXT_SYNC_COMMITTEE_GINDEX))

    # indicate finality whenever possible
    if finalized_block is not None:
        if finalized_block.slot != GENESIS_SLOT:
            update.finalized_header = block_to_light_client_header(finalized_block, cfg)
            assert htr_beacon(update.finalized_header.beacon) == bytes(attested_state.finalized_checkpoint_root)
        else:
            assert bytes(attested_state.finalized_checkpoint_root) == bytes(32)
        update.finality_branch = b"".join(compute_merkle_proof(attested_state, FINALIZED_ROOT_GINDEX))

    update.sync_committee_bits = bytes(block.sync_committee_bits)
    update.sync_committee_signature = bytes(block.sync_committee_signature)
    update.signature_slot = int(block.slot)
    return update


def create_light_client_finality_update(update: UpdateRow) -> UpdateRow:
    """full-node.md:197-205: the finality fields of `update` (as an UpdateRow whose next-committee
    fields are the defaults, the form sync-protocol.md:563-571 converts a LightClientFinalityUpdate to)."""
    return UpdateRow(attested_header=update.attested_header, finalized_header=update.finalized_header,
                     finality_branch=update.finality_branch, sync_committee_bits=update.sync_committee_bits,
                     sync_committee_signature=update.sync_committee_signature, signature_slot=update.signature_slot)


def create_light_client_optimistic_update(update: UpdateRow) -> UpdateRow:
    """full-node.md:213-219 (as an UpdateRow with default finality / next-committee fields,
    sync-protocol.md:582-590)."""
    return UpdateRow(attested_header=update.attested_header, sync_committee_bits=update.sync_committee_bits,
                     sync_committee_signature=update.sync_committee_signature, signature_slot=update.signature_slot)


def pack_updates(rows: Sequence[UpdateRow]):
    """UpdateRows -> PackedUpdates (include/lcv.h layouts; next_sync_committee values deduplicated
    into the pool, so HTR(SyncCommittee) runs once per distinct committee on the device)."""
    from .device import PackedUpdates
    n = len(rows)
    pool: Dict[bytes, int] = {}
    idx = np.zeros(n, np.uint32)
    for i, r in enumerate(rows):
        idx[i] = pool.setdefault(bytes(r.next_sync_committee), len(pool))
    pool_arr = np.zeros((max(1, len(pool)), L.SYNC_COMMITTEE_BYTES), np.uint8)
    for sc, k in pool.items():
        pool_arr[k] = np.frombuffer(sc, np.uint8)

    def col(get, width):
        a = np.zeros((n, width), np.uint8)
        for i, r in enumerate(rows):
            a[i] = np.frombuffer(get(r), np.uint8)
        return a
    return PackedUpdates(
        att_beacon=col(lambda r: r.attested_header.beacon, L.BEACON_BYTES),
        att_exec=col(lambda r: r.attested_header.execution, L.EXEC_BYTES),
        att_branch=col(lambda r: r.attested_header.execution_branch, L.EXEC_BRANCH_BYTES),
        fin_beacon=col(lambda r: r.finalized_header.beacon, L.BEACON_BYTES),
        fin_exec=col(lambda r: r.finalized_header.execution, L.EXEC_BYTES),
        fin_branch=col(lambda r: r.finalized_header.execution_branch, L.EXEC_BRANCH_BYTES),
        nsc_branch=col(lambda r: r.next_sync_committee_branch, L.NSC_BRANCH_BYTES),
        finality_branch=col(lambda r: r.finality_branch, L.FINALITY_BRANCH_BYTES),
        sync_bits=col(lambda r: r.sync_committee_bits, L.BITS_BYTES),
        sync_signature=col(lambda r: r.sync_committee_signature, L.SIGNATURE_BYTES),
        nsc_pool=pool_arr, nsc_index=idx,
        signature_slot=np.array([r.signature_slot for r in rows], np.uint64))


# ------------------------------------------------------------------ the batched path (device)
# reason code of the batched entries -> the check of create_light_client_update that fails (include/lcv.h
# lcv_producer_reason): the exception the per-object function raises, and its text
UPDATE_REASONS = {
    1: (AssertionError, "compute_epoch_at_slot(attested_state.slot) >= ALTAIR_FORK_EPOCH"),
    2: (AssertionError, "sum(block.message.body.sync_aggregate.sync_committee_bits) >= MIN_SYNC_COMMITTEE_PARTICIPANTS"),
    3: (AssertionError, "state.slot == state.latest_block_header.slot"),
    4: (AssertionError, "hash_tree_root(header) == hash_tree_root(block.message)"),
    5: (AssertionError, "attested_state.slot == attested_state.latest_block_header.slot"),
    6: (AssertionError, "hash_tree_root(attested_header) == hash_tree_root(attested_block.message) == block.message.parent_root"),
    7: (ValueError, "a Capella-or-later block needs its execution payload"),
    8: (ValueError, "a Capella-or-later block needs its execution payload"),
    9: (AssertionError, "hash_tree_root(update.finalized_header.beacon) == attested_state.finalized_checkpoint.root"),
    10: (AssertionError, "attested_state.finalized_checkpoint.root == Bytes32()"),
}
BOOTSTRAP_REASONS = {
    1: (AssertionError, "compute_epoch_at_slot(state.slot) >= ALTAIR_FORK_EPOCH"),
    2: (AssertionError, "state.slot == state.latest_block_header.slot"),
    3: (AssertionError, "hash_tree_root(header) == hash_tree_root(block.message)"),
    4: (ValueError, "a Capella-or-later block needs its execution payload"),
}


def raise_for_reason(reason: int, table=UPDATE_REASONS) -> None:
    """Raise what the per-object function raises for a non-zero reason of the batched one."""
    if int(reason):
        exc, text = table[int(reason)]
        raise exc(text)


def pack_views(states: Sequence[BeaconStateView], blocks: Sequence[BeaconBlockView]):
    """Lists of views -> lcv.device.PackedViews: the column tables of include/lcv.h (lcv_state_views,
    lcv_block_views) and the pool of the states' distinct SyncCommittee values (deduplicated by content, like
    pack_updates).  A block without a payload gets exec_kind 0, else 1 (Capella) or 2 (execution_deneb)."""
    from .device import PackedViews
    ns, nb = len(states), len(blocks)
    pool: Dict[bytes, int] = {}
    cur, nxt = np.zeros(ns, np.uint32), np.zeros(ns, np.uint32)
    for i, s in enumerate(states):
        cur[i] = pool.setdefault(bytes(s.current_sync_committee), len(pool))
        nxt[i] = pool.setdefault(bytes(s.next_sync_committee), len(pool))
    committees = np.zeros((len(pool), L.SYNC_COMMITTEE_BYTES), np.uint8)
    for sc, k in pool.items():
        committees[k] = np.frombuffer(sc, np.uint8)

    def rows(items, get, width):
        a = np.zeros((len(items), width), np.uint8)
        for i, x in enumerate(items):
            a[i] = np.frombuffer(bytes(get(x)), np.uint8)
        return a
    sroots = np.zeros((ns, STATE_FIELDS, 32), np.uint8)
    for i, s in enumerate(states):
        sroots[i] = np.asarray(s.field_roots, np.uint8).reshape(STATE_FIELDS, 32)
    broots = np.zeros((nb, BODY_FIELDS, 32), np.uint8)
    for i, b in enumerate(blocks):
        broots[i] = np.asarray(b.body_roots, np.uint8).reshape(BODY_FIELDS, 32)
    return PackedViews(
        state_slot=np.array([s.slot for s in states], np.uint64),
        state_header=rows(states, lambda s: s.latest_block_header, L.BEACON_BYTES),
        state_fin_epoch=np.array([s.finalized_checkpoint_epoch for s in states], np.uint64),
        state_fin_root=rows(states, lambda s: s.finalized_checkpoint_root, 32),
        state_roots=sroots, state_cur=cur, state_nxt=nxt,
        block_slot=np.array([b.slot for b in blocks], np.uint64),
        block_proposer=np.array([b.proposer_index for b in blocks], np.uint64),
        block_parent=rows(blocks, lambda b: b.parent_root, 32),
        block_state_root=rows(blocks, lambda b: b.state_root, 32),
        block_bits=rows(blocks, lambda b: b.sync_committee_bits, L.BITS_BYTES),
        block_sig=rows(blocks, lambda b: b.sync_committee_signature, L.SIGNATURE_BYTES),
        block_exec=rows(blocks, lambda b: b.execution if b.execution is not None else bytes(L.EXEC_BYTES), L.EXEC_BYTES),
        block_kind=np.array([0 if b.execution is None else 2 if b.execution_deneb else 1 for b in blocks], np.uint8),
        block_roots=broots, committees=committees)


def create_light_client_updates(states: Sequence[BeaconStateView], blocks: Sequence[BeaconBlockView], cases,
                                kind: str = "update", verifier=None):
    """The batched twin of create_light_client_update (kind "update"), create_light_client_finality_update
    ("finality") and create_light_client_optimistic_update ("optimistic") on the device: `cases` are rows of
    (state, block, attested_state, attested_block, finalized_block or -1) into the two lists -> (PackedUpdates,
    reasons).  reasons[i] is 0, or names the check that fails for row i (raise_for_reason raises what the
    per-object function raises); such a row is UpdateRow().  The fork epochs and periods are the verifier's."""
    from . import runtime
    v = verifier if verifier is not None else runtime.default_verifier()
    return v.create_updates(pack_views(states, blocks), cases, kind)


MAX_REQUEST_LIGHT_CLIENT_UPDATES = 128


def updates_by_range(rb, start_period: int, count: int, genesis_validators_root: bytes, verifier=None) -> list:
    """The response chunks of LightClientUpdatesByRange (p2p-interface.md:177-200) from a resident batch of
    candidate updates -> [(fork digest, SSZ LightClientUpdate)], at most min(128, count) of them (:187): the best
    update (is_better_update; lcv.store.best_update_per_period) of each sync-committee period in [start_period,
    start_period + count) that has one, in consecutive order by period.  The batch is ranked where it lies, and the
    winners are encoded by one lcv_batch_encode call, the container of each chunk chosen from its attested slot
    (:189); the chunk's digest is compute_fork_digest of the fork version at that slot.  Rows without a sync
    committee participant (the all-zero rows of cases the producer refused) are never served."""
    from . import runtime
    from .device import RANK_N_MASK
    from .store import best_update_per_period
    from .wire import fork_digest
    v = verifier if verifier is not None else runtime.default_verifier()
    limit = min(MAX_REQUEST_LIGHT_CLIENT_UPDATES, int(count))
    if limit <= 0 or rb.n == 0:
        return []
    rank = v.rank_resident(rb)
    best = best_update_per_period(rb, v, rank=rank)
    rows = [best[p] for p in sorted(best)
            if start_period <= p < start_period + int(count) and int(rank["key0"][best[p]]) & RANK_N_MASK][:limit]
    if not rows:
        return []
    enc = v.encode_resident(rb, "update", "auto", rows=rows)
    bad = np.flatnonzero(enc.status)
    if bad.size:
        raise ValueError(f"updates_by_range: row {rows[int(bad[0])]} cannot be encoded (status {int(enc.status[bad[0]])})")
    digests = {}
    out = []
    for i, msg in enumerate(enc.messages()):
        ver = enc.version[i].tobytes()
        if ver not in digests:  # at most five distinct versions
            digests[ver] = fork_digest(ver, genesis_validators_root)
        out.append((digests[ver], msg))
    return out
