"""`Verifier`: one device context of liblcv.so and numpy-level wrappers around the C ABI."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import config as _config
from . import layout as L
from ._native import (Lib, LcvError, UpdateBatch, HeaderCols, StoreTable, FoldStateC, FoldResultC, StateViews,
                      BlockViews, UpdateCases, RelayRequest, STORE_NEXT_UNKNOWN, as_u8, load, ptr)

SYNC_COMMITTEE_BYTES = 24624
EXEC_RECORD_BYTES = 832

# the 32-byte rank record of an update (include/lcv.h): is_better_update(a, b) (sync-protocol.md:260-311) iff
# (key0_a, -attested_a, -signature_a) > (key0_b, -attested_b, -signature_b)
RANK_DTYPE = np.dtype([("key0", "<u4"), ("flags", "<u4"), ("attested_slot", "<u8"), ("signature_slot", "<u8"),
                       ("finalized_slot", "<u8")])
RANK_SUPER, RANK_REL_SC, RANK_FIN, RANK_FIN_SC, RANK_N_MASK = 1 << 23, 1 << 12, 1 << 11, 1 << 10, 0x3FF


@dataclass
class FoldState:
    """lcv_fold_state: what the post-validation store logic reads besides validation's own store values."""
    optimistic_slot: int = 0
    previous_max_active_participants: int = 0
    current_max_active_participants: int = 0
    has_best: bool = False
    best_key0: int = 0
    best_attested_slot: int = 0
    best_signature_slot: int = 0

    def to_c(self) -> FoldStateC:
        return FoldStateC(int(self.optimistic_slot), int(self.previous_max_active_participants),
                          int(self.current_max_active_participants), 1 if self.has_best else 0, int(self.best_key0),
                          int(self.best_attested_slot), int(self.best_signature_slot))

    @staticmethod
    def from_c(c: FoldStateC) -> "FoldState":
        return FoldState(int(c.optimistic_slot), int(c.previous_max_active_participants),
                         int(c.current_max_active_participants), bool(c.has_best), int(c.best_key0),
                         int(c.best_attested_slot), int(c.best_signature_slot))


@dataclass
class FoldResult:
    """lcv_fold_result: the state after the consumed rows (maxima and optimistic slot before
    apply_light_client_update of apply_row), and the rows the host needs; -1 = none."""
    next: FoldState
    rows_consumed: int
    apply_row: int
    best_row: int
    optimistic_row: int
    accepted_count: int

    @staticmethod
    def from_c(c: FoldResultC) -> "FoldResult":
        return FoldResult(FoldState.from_c(c.next), int(c.rows_consumed), int(c.apply_row), int(c.best_row),
                          int(c.optimistic_row), int(c.accepted_count))


@dataclass
class PackedUpdates:
    """Structure-of-arrays batch of LightClientUpdates (row i = update i); layouts in include/lcv.h."""
    att_beacon: np.ndarray       # (n, 112) u8
    att_exec: np.ndarray         # (n, 832) u8
    att_branch: np.ndarray       # (n, 128) u8
    fin_beacon: np.ndarray       # (n, 112) u8
    fin_exec: np.ndarray         # (n, 832) u8
    fin_branch: np.ndarray       # (n, 128) u8
    nsc_pool: np.ndarray         # (npool, 24624) u8
    nsc_index: np.ndarray        # (n,) u32
    nsc_branch: np.ndarray       # (n, 160) u8
    finality_branch: np.ndarray  # (n, 192) u8
    sync_bits: np.ndarray        # (n, 64) u8
    sync_signature: np.ndarray   # (n, 96) u8
    signature_slot: np.ndarray   # (n,) u64

    # column -> (dtype, trailing shape, counted by the pool instead of n), in field order = lcv_update_batch's pointers
    _SPEC = dict(att_beacon=(np.uint8, (L.BEACON_BYTES,), False), att_exec=(np.uint8, (L.EXEC_BYTES,), False),
                 att_branch=(np.uint8, (L.EXEC_BRANCH_BYTES,), False), fin_beacon=(np.uint8, (L.BEACON_BYTES,), False),
                 fin_exec=(np.uint8, (L.EXEC_BYTES,), False), fin_branch=(np.uint8, (L.EXEC_BRANCH_BYTES,), False),
                 nsc_pool=(np.uint8, (L.SYNC_COMMITTEE_BYTES,), True), nsc_index=(np.uint32, (), False),
                 nsc_branch=(np.uint8, (L.NSC_BRANCH_BYTES,), False),
                 finality_branch=(np.uint8, (L.FINALITY_BRANCH_BYTES,), False),
                 sync_bits=(np.uint8, (L.BITS_BYTES,), False), sync_signature=(np.uint8, (L.SIGNATURE_BYTES,), False),
                 signature_slot=(np.uint64, (), False))
    _CTYPE = {np.uint8: C.c_uint8, np.uint32: C.c_uint32, np.uint64: C.c_uint64}

    @property
    def n(self) -> int:
        return int(self.att_beacon.shape[0])

    def check(self) -> None:
        n = self.n
        for name, (dt, tail, pool) in self._SPEC.items():
            a = getattr(self, name)
            rows = a.shape[0] if pool and a.ndim else n
            if a.dtype != dt or a.shape != (rows,) + tail or not a.flags.c_contiguous:
                want = ("npool" if pool else n,) + tail
                raise ValueError(f"{name}: need C-contiguous {np.dtype(dt).name} ({', '.join(map(str, want))}"
                                 f"{',' if len(want) == 1 else ''}), got {a.dtype} {a.shape}")
        if n and int(self.nsc_index.max()) >= self.nsc_pool.shape[0]:
            raise ValueError("nsc_index out of range")

    def slice(self, lo: int, hi: int) -> "PackedUpdates":
        return PackedUpdates(**{name: getattr(self, name) if pool else np.ascontiguousarray(getattr(self, name)[lo:hi])
                                for name, (_, _, pool) in self._SPEC.items()})

    def to_c(self) -> Tuple[UpdateBatch, list]:
        """The lcv_update_batch naming this batch's own arrays (check() has required them C-contiguous, so the
        entries that write a batch write through the same pointers), and the arrays to keep alive."""
        self.check()
        keep = [getattr(self, name) for name in self._SPEC]
        p = [ptr(a, self._CTYPE[dt]) for a, (dt, _, _) in zip(keep, self._SPEC.values())]
        return UpdateBatch(HeaderCols(*p[0:3]), HeaderCols(*p[3:6]), *p[6:], self.n, int(self.nsc_pool.shape[0])), keep

    @staticmethod
    def empty(n: int, npool: int) -> "PackedUpdates":
        """An all-zero batch of n rows and npool pool rows (the arrays the download entries write into)."""
        return PackedUpdates(**{name: np.zeros((npool if pool else n,) + tail, dt)
                                for name, (dt, tail, pool) in PackedUpdates._SPEC.items()})


UPDATE_KINDS = {"update": 0, "finality": 1, "optimistic": 2}
WIRE_FORKS = {"deneb": 0, "capella": 1, "altair": 2, "auto": -1}  # lcv_batch_encode's fork codes; -1: LCV_FORK_AUTO


@dataclass
class EncodedMessages:
    """SSZ wire messages as the device wrote them (lcv_batch_encode): message i is buf[i, :length[i]]; the rest of
    its area is zero.  A row with a non-zero status has length 0."""
    buf: np.ndarray      # (m, pitch) u8
    length: np.ndarray   # (m,) u32
    fork: np.ndarray     # (m,) u8  the fork code used: 0 Deneb, 1 Capella, 2 Altair
    version: np.ndarray  # (m, 4) u8  the fork version of the attested slot's epoch (the chunk's ForkDigest context)
    status: np.ndarray   # (m,) u8  0 ok, 1 Altair-format row with execution data, 2 extra_data longer than 32 bytes

    @property
    def n(self) -> int:
        return int(self.buf.shape[0])

    def messages(self) -> list:
        return [self.buf[i, :int(self.length[i])].tobytes() for i in range(self.n)]

    @staticmethod
    def empty(m: int, pitch: int, fill: int = 0) -> "EncodedMessages":
        return EncodedMessages(np.full((m, pitch), fill, np.uint8), np.zeros(m, np.uint32), np.zeros(m, np.uint8),
                               np.zeros((m, 4), np.uint8), np.zeros(m, np.uint8))


@dataclass
class PackedViews:
    """Tables of sparse state / block views (include/lcv.h lcv_state_views, lcv_block_views) and the pool of their
    distinct SyncCommittee values: the input of the batched producer entries (lcv.producer.pack_views)."""
    state_slot: np.ndarray        # (ns,) u64
    state_header: np.ndarray      # (ns, 112) u8  latest_block_header
    state_fin_epoch: np.ndarray   # (ns,) u64
    state_fin_root: np.ndarray    # (ns, 32) u8
    state_roots: np.ndarray       # (ns, 28, 32) u8
    state_cur: np.ndarray         # (ns,) u32  committee row of current_sync_committee
    state_nxt: np.ndarray         # (ns,) u32  committee row of next_sync_committee
    block_slot: np.ndarray        # (nb,) u64
    block_proposer: np.ndarray    # (nb,) u64
    block_parent: np.ndarray      # (nb, 32) u8
    block_state_root: np.ndarray  # (nb, 32) u8
    block_bits: np.ndarray        # (nb, 64) u8
    block_sig: np.ndarray         # (nb, 96) u8
    block_exec: np.ndarray        # (nb, 832) u8
    block_kind: np.ndarray        # (nb,) u8   0 no payload, 1 Capella, 2 Deneb
    block_roots: np.ndarray       # (nb, 12, 32) u8
    committees: np.ndarray        # (ncomm, 24624) u8

    _SPEC = dict(state_slot=(np.uint64, ()), state_header=(np.uint8, (112,)), state_fin_epoch=(np.uint64, ()),
                 state_fin_root=(np.uint8, (32,)), state_roots=(np.uint8, (28, 32)), state_cur=(np.uint32, ()),
                 state_nxt=(np.uint32, ()), block_slot=(np.uint64, ()), block_proposer=(np.uint64, ()),
                 block_parent=(np.uint8, (32,)), block_state_root=(np.uint8, (32,)), block_bits=(np.uint8, (64,)),
                 block_sig=(np.uint8, (96,)), block_exec=(np.uint8, (EXEC_RECORD_BYTES,)), block_kind=(np.uint8, ()),
                 block_roots=(np.uint8, (12, 32)), committees=(np.uint8, (SYNC_COMMITTEE_BYTES,)))

    @property
    def ns(self) -> int:
        return int(self.state_slot.shape[0])

    @property
    def nb(self) -> int:
        return int(self.block_slot.shape[0])

    @property
    def ncomm(self) -> int:
        return int(self.committees.shape[0])

    def to_c(self):
        keep = {}
        for name, (dt, tail) in self._SPEC.items():
            rows = self.ncomm if name == "committees" else self.ns if name.startswith("state_") else self.nb
            a = np.ascontiguousarray(getattr(self, name), dt)
            if a.shape != (rows,) + tail:
                raise ValueError(f"{name}: need {np.dtype(dt).name} {(rows,) + tail}, got {a.shape}")
            keep[name] = a
        P = lambda name, t=C.c_uint8: ptr(keep[name], t)  # noqa: E731
        sv = StateViews(P("state_slot", C.c_uint64), P("state_header"), P("state_fin_epoch", C.c_uint64),
                        P("state_fin_root"), P("state_roots"), P("state_cur", C.c_uint32), P("state_nxt", C.c_uint32))
        bv = BlockViews(P("block_slot", C.c_uint64), P("block_proposer", C.c_uint64), P("block_parent"),
                        P("block_state_root"), P("block_bits"), P("block_sig"), P("block_exec"), P("block_kind"),
                        P("block_roots"))
        return sv, bv, P("committees"), keep


def _cases_to_c(cases):
    """(n, 5) rows of (state, block, attested_state, attested_block, finalized_block or -1) -> lcv_update_cases."""
    a = np.asarray(cases, np.int64).reshape(-1, 5)
    if a.size and (a[:, :4].min() < 0 or a.max() > 0x7FFFFFFF or a[:, 4].min() < -(1 << 31)):
        raise ValueError("cases: rows are (state, block, attested_state, attested_block, finalized_block or -1)")
    cols = [np.ascontiguousarray(a[:, k], np.uint32) for k in range(4)] + [np.ascontiguousarray(a[:, 4], np.int32)]
    uc = UpdateCases(*[ptr(c, C.c_uint32) for c in cols[:4]], ptr(cols[4], C.c_int32))
    return uc, cols, int(a.shape[0])


class ResidentBatch:
    """A device-resident batch (Verifier.upload).  `stores`: it carries its store_index column, so every
    validate_resident* call validates it against the store table instead of the set_store snapshot."""

    def __init__(self, verifier: "Verifier", handle: C.c_void_p, n: int, stores: bool = False,
                 npool: Optional[int] = None):
        self.v = verifier
        self.handle = handle
        self.n = n
        self.stores = stores
        self.npool = npool  # pool rows (Verifier.download sizes its arrays by it)

    def free(self):
        if self.handle:
            self.v.lib.lcv_batch_free(self.v.ctx, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Verifier:
    """A liblcv context on one device.  `lib` defaults to the product HIP library."""

    def __init__(self, device: int = 0, lib: Optional[Lib] = None):
        self.lib = lib if lib is not None else load()
        self.ctx = C.c_void_p()
        rc = self.lib.lcv_init(device, C.byref(self.ctx))
        if rc != 0:
            raise LcvError(f"lcv_init(device={device}) failed with status {rc}")
        self.device = device
        self.config = _config.MAINNET  # the context's network configuration (lcv_init: mainnet)
        self.latency_mode = 64  # lcv_set_latency_mode's value (lcv_init's default: the fan engine up to 64 rows)
        self.pipeline = (1, 1)  # lcv_set_pipeline's (streams, chunks)
        self.chunk_rows = 65536  # rows per validate chunk, and the most one asynchronous call takes (debug_set_chunk)
        self.dedup = False  # lcv_set_dedup's value
        self.rlc_group = 0  # lcv_set_rlc's group (0: off) and the seed of the last call that gave one
        self.rlc_seed: Optional[bytes] = None
        # per work-space slot, what the wait of its last relay_async / validate_stores_async_fold needs to shape its
        # outputs: (messages, pairs, store rows of the fold's result or None, the stores present)
        self._slot_batch = {}

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.lcv_last_error(self.ctx)
            raise LcvError(f"{what}: status {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if self.ctx:
            self.lib.lcv_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, cfg: "_config.NetworkConfig") -> None:
        """The network configuration this context validates under (lcv_set_config; mainnet after init)."""
        epochs = np.array(cfg.fork_epochs(), np.uint64)
        versions = np.frombuffer(b"".join(cfg.fork_versions()), np.uint8).copy()
        dom = np.frombuffer(cfg.DOMAIN_SYNC_COMMITTEE, np.uint8).copy()
        self._check(self.lib.lcv_set_config(self.ctx, int(cfg.SLOTS_PER_EPOCH), int(cfg.EPOCHS_PER_SYNC_COMMITTEE_PERIOD),
                                            ptr(epochs, C.c_uint64), ptr(versions), ptr(dom)), "lcv_set_config")
        self.config = cfg

    def set_pipeline(self, streams: int, chunks: int) -> None:
        """Run validate's per-update stage chain on `chunks` slices over `streams` HIP streams
        (overlapping stages of different slices); (1, 1) = serial stages with per-stage timings."""
        self._check(self.lib.lcv_set_pipeline(self.ctx, int(streams), int(chunks)), "lcv_set_pipeline")
        self.pipeline = (int(streams), int(chunks))

    def set_latency_mode(self, max_rows: int) -> None:
        """Latency mode for small batches (lcv_set_latency_mode): batches of at most max_rows rows run the SOP
        programs (hash_to_G2's tail, final exponentiation) on the fan engine (an op's K products on K lanes, its
        reduction and tail on a 16-lane row, one item per block), both Miller walks and the accumulation as one fan-engine program, and the SSWU
        maps / signature decoding one item per wave (square-root chains spread over the wave) — one update
        6.0 ms on the batch engine -> 2.8 ms.  Results are identical to the batch engine's.  Default 64;
        0 = the batch engine always."""
        self._check(self.lib.lcv_set_latency_mode(self.ctx, int(max_rows)), "lcv_set_latency_mode")
        self.latency_mode = int(max_rows)

    def set_dedup(self, on: bool) -> None:
        """Check each distinct sync-committee signature of a chunk once (lcv_set_dedup; off by default): rows whose
        attested beacon header, signature_slot, sync bits, signature and signing committee are bytewise equal — one
        update relayed to many stores — share one run of the BLS half, and every row keeps its own pre-checks.
        Verdicts and reasons are those of the mode off.  Batches taken (validate*, upload) while the mode is on are
        grouped; a ResidentBatch uploaded with it off, or made on the device (create_updates_resident,
        decode_resident: no host bytes to class), is validated without deduplication until classify_resident has
        classed it.  LcvError (status -1)
        together with a multi-stream pipeline (set_pipeline streams > 1), from whichever call comes second."""
        self._check(self.lib.lcv_set_dedup(self.ctx, 1 if on else 0), "lcv_set_dedup")
        self.dedup = bool(on)

    def last_dedup(self, slot: int = 0) -> Tuple[int, int]:
        """(rows, distinct BLS items) of the last batch enqueued on work-space slot `slot` (lcv_last_dedup);
        synchronous calls use slot 0, summed over the batch's chunks.  items == rows without deduplication."""
        rows, items = C.c_uint64(), C.c_uint64()
        self._check(self.lib.lcv_last_dedup(self.ctx, int(slot), C.byref(rows), C.byref(items)), "lcv_last_dedup")
        return int(rows.value), int(items.value)

    def debug_dedup_hash_bits(self, bits: int) -> None:
        """Test hook (lcv_debug_dedup_hash_bits): set_dedup's host hash truncated to `bits` bits (64: whole; 0:
        every row collides, so only the full compare of the rows' bytes separates them)."""
        self._check(self.lib.lcv_debug_dedup_hash_bits(self.ctx, int(bits)), "lcv_debug_dedup_hash_bits")

    def classify_resident(self, rb: ResidentBatch) -> int:
        """Class a resident batch where it lies (lcv_batch_classify) -> the number of distinct classes.  Any resident
        batch — uploaded, decode_resident's, create_updates_resident's, fan_out's — gets the class column a batch
        uploaded under set_dedup(True) has (two kernels: a 64-bit key per row, then full compares of the rows the keys
        pair up), whatever set_dedup says now; validation with the mode on then checks each distinct signature once."""
        if not rb.handle:
            return 0
        m = C.c_uint64()
        self._check(self.lib.lcv_batch_classify(self.ctx, rb.handle, C.byref(m)), "lcv_batch_classify")
        return int(m.value)

    def last_classify_timings(self) -> Tuple[float, float]:
        """Kernel milliseconds of the last classify_resident (lcv_last_classify_timings): (the keys, the compares)."""
        ms = (C.c_float * 2)()
        self._check(self.lib.lcv_last_classify_timings(self.ctx, ms), "lcv_last_classify_timings")
        return float(ms[0]), float(ms[1])

    def debug_batch_classes(self, rb: ResidentBatch) -> np.ndarray:
        """Test hook (lcv_debug_batch_classes): a batch's class column, cls[i] = the label of row i's class (at upload
        and after classify_resident: the first row with row i's tuple).  LcvError for a batch that has none."""
        out = np.zeros(max(rb.n, 1), np.uint32)
        self._check(self.lib.lcv_debug_batch_classes(self.ctx, rb.handle, ptr(out, C.c_uint32)), "lcv_debug_batch_classes")
        return out[:rb.n]

    def fan_out(self, rb: ResidentBatch, rows=None, store_index=None) -> ResidentBatch:
        """A new resident batch whose row i is row rows[i] of rb (lcv_batch_fan_out; repeats allowed; None: every row
        in order), gathered on the device with rb's whole pool.  With `store_index` (one store-table row per row of the
        result) it is a table batch, as upload(batch, store_index) makes; without, a single-store subset.  The classes
        of a classed rb are inherited."""
        ix = None if rows is None else np.ascontiguousarray(rows, np.uint32).reshape(-1)
        six = None if store_index is None else np.ascontiguousarray(store_index, np.uint32).reshape(-1)
        n = rb.n if ix is None else ix.shape[0]
        if six is not None and six.shape[0] != n:
            raise ValueError("store_index needs one entry per row of the result")
        h = C.c_void_p()
        self._check(self.lib.lcv_batch_fan_out(self.ctx, rb.handle, None if ix is None or not n else ptr(ix, C.c_uint32),
                                               None if six is None or not n else ptr(six, C.c_uint32), n, C.byref(h)),
                    "lcv_batch_fan_out")
        return ResidentBatch(self, h, n, stores=six is not None, npool=rb.npool)

    def set_rlc(self, group: int, seed: Optional[bytes] = None) -> None:
        """Randomised batch verification (lcv_set_rlc; off by default): groups of `group` (2, 4, ... 64) consecutive
        items of a batch-engine chunk pay one final exponentiation, and only the items of a failing group one of their
        own; 0 turns the mode off.  `seed`: 32 bytes that whoever supplies updates cannot predict — by default drawn
        from os.urandom by this call.  A wrong group is accepted with probability about 2^-64; every other verdict and
        every reason is that of the mode off.  LcvError (status -1) for any other group, an all-zero seed, or together
        with a multi-stream pipeline (set_pipeline streams > 1), from whichever call comes second."""
        group = int(group)
        if group and seed is None:
            seed = os.urandom(32)
        if seed is not None and len(bytes(seed)) != 32:
            raise ValueError("the seed must be 32 bytes")
        s = as_u8(bytes(seed)) if seed is not None else None
        self._check(self.lib.lcv_set_rlc(self.ctx, group, ptr(s) if s is not None else None), "lcv_set_rlc")
        self.rlc_group = group
        if seed is not None:
            self.rlc_seed = bytes(seed)

    def last_rlc(self, slot: int = 0) -> Tuple[int, int]:
        """(groups, rows retried after a failing group) of the last batch enqueued on work-space slot `slot`
        (lcv_last_rlc), summed over its chunks; valid once that batch has been waited for.  groups == 0: the mode did
        not act (off, the fan engine, the CPU-baseline build)."""
        groups, retried = C.c_uint64(), C.c_uint64()
        self._check(self.lib.lcv_last_rlc(self.ctx, int(slot), C.byref(groups), C.byref(retried)), "lcv_last_rlc")
        return int(groups.value), int(retried.value)

    def debug_rlc_coeffs(self, counter: int, n: int) -> np.ndarray:
        """Test hook (lcv_debug_rlc_coeffs): the n coefficients the device derives for batch counter `counter` under
        the seed of the last set_rlc."""
        out = np.zeros(int(n), np.uint64)
        self._check(self.lib.lcv_debug_rlc_coeffs(self.ctx, int(counter), int(n), ptr(out, C.c_uint64)),
                    "lcv_debug_rlc_coeffs")
        return out

    def debug_rlc_scale(self, p96: np.ndarray, r: np.ndarray) -> np.ndarray:
        """Test hook (lcv_debug_rlc_scale): r[i] * P[i] for affine G1 points (rows of x || y, 48 big-endian bytes
        each), through the scaling kernel's ladder and shared inversion."""
        p = np.ascontiguousarray(p96, np.uint8).reshape(-1, 96)
        rr = np.ascontiguousarray(r, np.uint64).reshape(-1)
        if rr.shape[0] != p.shape[0]:
            raise ValueError("one coefficient per point")
        out = np.zeros_like(p)
        self._check(self.lib.lcv_debug_rlc_scale(self.ctx, ptr(p), ptr(rr, C.c_uint64), p.shape[0], ptr(out)),
                    "lcv_debug_rlc_scale")
        return out

    def debug_set_chunk(self, rows: int) -> None:
        """Test hook (lcv_debug_set_chunk): rows per validate chunk, 1 up to the default 65536."""
        self._check(self.lib.lcv_debug_set_chunk(self.ctx, int(rows)), "lcv_debug_set_chunk")
        self.chunk_rows = int(rows)

    def engine_log(self, reset: bool = False) -> Dict[str, object]:
        """Which engines ran since the last reset (lcv_debug_engine_log): SOP launches on the fan / batch
        engine, SSWU + signature launches on the one-item-per-wave twins / one lane per item, and the items
        per wave of each SOP program's last batch-engine launch (0 = not launched)."""
        out = np.zeros(8, np.uint64)
        self._check(self.lib.lcv_debug_engine_log(self.ctx, ptr(out, C.c_uint64), 1 if reset else 0),
                    "lcv_debug_engine_log")
        return {"fan": int(out[0]), "batch": int(out[1]), "twin": int(out[2]), "lane": int(out[3]),
                "items": dict(zip(("lines", "miller_acc", "fexp", "h2c"), (int(x) for x in out[4:8])))}

    def last_timings(self) -> Dict[str, float]:
        ms = (C.c_float * 32)()
        n = C.c_int()
        self._check(self.lib.lcv_last_timings(self.ctx, ms, 32, C.byref(n)), "lcv_last_timings")
        return {self.lib.lcv_stage_name(i).decode(): float(ms[i]) for i in range(n.value)}

    # ------------------------------------------------------------------ validation
    def set_store(self, finalized_slot: int, current_sync_committee: bytes, next_sync_committee: bytes) -> np.ndarray:
        cur = as_u8(bytes(current_sync_committee))
        nxt = as_u8(bytes(next_sync_committee))
        if cur.size != SYNC_COMMITTEE_BYTES or nxt.size != SYNC_COMMITTEE_BYTES:
            raise ValueError("committees must be 24624-byte SSZ SyncCommittee values")
        ks = np.zeros(1024, np.uint8)
        self._check(self.lib.lcv_set_store(self.ctx, int(finalized_slot), ptr(cur), ptr(nxt), ptr(ks)), "lcv_set_store")
        return ks

    def validate(self, batch: PackedUpdates, current_slot: int, genesis_validators_root: bytes):
        b, keep = batch.to_c()
        gvr = as_u8(bytes(genesis_validators_root))
        v = np.zeros(batch.n, np.uint8)
        r = np.zeros(batch.n, np.uint8)
        self._check(self.lib.lcv_validate_updates(self.ctx, C.byref(b), int(current_slot), ptr(gvr), ptr(v), ptr(r)),
                    "lcv_validate_updates")
        return v.astype(bool), r

    def set_store_table(self, committees: np.ndarray, finalized_slot, current, next) -> np.ndarray:
        """A store snapshot per row (lcv_set_store_table): `committees` (ncomm, 24624) distinct SSZ SyncCommittee
        values; store s = (finalized_slot[s], committee row current[s], committee row next[s] or
        STORE_NEXT_UNKNOWN — an all-zero committee row means the same).  Every key is decoded and KeyValidated
        once, device resident; returns the key status (ncomm, 512): 0 valid key, 2 invalid.  Independent of
        set_store."""
        com = np.ascontiguousarray(committees, np.uint8).reshape(-1, SYNC_COMMITTEE_BYTES)
        fin = np.ascontiguousarray(finalized_slot, np.uint64).reshape(-1)
        cur = np.ascontiguousarray(current, np.uint32).reshape(-1)
        nxt = np.ascontiguousarray(next, np.uint32).reshape(-1)
        if not (fin.shape == cur.shape == nxt.shape):
            raise ValueError("finalized_slot, current and next need one entry per store")
        t = StoreTable(ptr(com), com.shape[0], ptr(fin, C.c_uint64), ptr(cur, C.c_uint32), ptr(nxt, C.c_uint32),
                       fin.shape[0])
        ks = np.zeros((com.shape[0], 512), np.uint8)
        self._store_table_key = None  # (lcv.runtime.ensure_store_table's memo of the table's content)
        self._check(self.lib.lcv_set_store_table(self.ctx, C.byref(t), ptr(ks)), "lcv_set_store_table")
        return ks

    def validate_stores(self, batch: PackedUpdates, store_index, current_slot: int, genesis_validators_root: bytes):
        """validate_light_client_update of update i against row store_index[i] of the store table
        (lcv_validate_updates_stores) -> (verdicts, reason codes): what set_store(that store) + validate gives."""
        b, keep = batch.to_c()
        six = self._store_index(batch, store_index)
        gvr = as_u8(bytes(genesis_validators_root))
        v = np.zeros(batch.n, np.uint8)
        r = np.zeros(batch.n, np.uint8)
        self._check(self.lib.lcv_validate_updates_stores(self.ctx, C.byref(b), ptr(six, C.c_uint32), int(current_slot),
                                                         ptr(gvr), ptr(v), ptr(r)), "lcv_validate_updates_stores")
        return v.astype(bool), r

    def _store_index(self, batch: PackedUpdates, store_index) -> np.ndarray:
        six = np.ascontiguousarray(store_index, np.uint32).reshape(-1)
        if six.shape[0] != batch.n:
            raise ValueError("store_index needs one entry per update")
        return six

    def upload(self, batch: PackedUpdates, store_index=None) -> ResidentBatch:
        """A device-resident copy of `batch`.  With `store_index` (one store-table row per update:
        lcv_batch_upload_stores) the batch is a table batch: validate_resident, validate_resident_dev,
        validate_resident_async and the sharded calls validate update i against row store_index[i] of the store
        table that is set when they are called (no table is needed yet here)."""
        b, keep = batch.to_c()
        h = C.c_void_p()
        if store_index is None:
            self._check(self.lib.lcv_batch_upload(self.ctx, C.byref(b), C.byref(h)), "lcv_batch_upload")
            return ResidentBatch(self, h, batch.n, npool=int(batch.nsc_pool.shape[0]))
        six = self._store_index(batch, store_index)
        self._check(self.lib.lcv_batch_upload_stores(self.ctx, C.byref(b), ptr(six, C.c_uint32), C.byref(h)),
                    "lcv_batch_upload_stores")
        return ResidentBatch(self, h, batch.n, stores=True, npool=int(batch.nsc_pool.shape[0]))

    # ------------------------------------------------------------------ the producer side, batched (include/lcv.h)
    @staticmethod
    def _kind(kind) -> int:
        k = UPDATE_KINDS.get(kind, kind) if isinstance(kind, str) else kind
        return int(k)

    def create_updates_resident(self, views: PackedViews, cases, kind=0, reason: Optional[np.ndarray] = None):
        """create_light_client_update (kind 0 / "update"; 1 / "finality", 2 / "optimistic": the finality /
        optimistic update made from it) for every row of `cases` — (n, 5) rows of (state, block, attested_state,
        attested_block, finalized_block or -1) into `views` — on the device (lcv_create_updates_resident) ->
        (ResidentBatch, reasons).  reasons[i]: 0, or the first failing check (lcv_producer_reason); such a row is
        LightClientUpdate().  The batch's pool is views.committees and one all-zero row."""
        sv, bv, com, keep = views.to_c()
        uc, cols, n = _cases_to_c(cases)
        r = reason if reason is not None else np.zeros(n, np.uint8)
        h = C.c_void_p()
        self._check(self.lib.lcv_create_updates_resident(self.ctx, C.byref(sv), views.ns, C.byref(bv), views.nb, com,
                                                         views.ncomm, C.byref(uc), n, self._kind(kind), ptr(r),
                                                         C.byref(h)), "lcv_create_updates_resident")
        return ResidentBatch(self, h if n else None, n, npool=views.ncomm + 1), r

    def create_updates(self, views: PackedViews, cases, kind=0, reason: Optional[np.ndarray] = None):
        """The same, copied to the host (lcv_create_updates) -> (PackedUpdates, reasons)."""
        sv, bv, com, keep = views.to_c()
        uc, cols, n = _cases_to_c(cases)
        r = reason if reason is not None else np.zeros(n, np.uint8)
        out = PackedUpdates.empty(n, views.ncomm + 1)
        b, keep_out = out.to_c()
        self._check(self.lib.lcv_create_updates(self.ctx, C.byref(sv), views.ns, C.byref(bv), views.nb, com,
                                                views.ncomm, C.byref(uc), n, self._kind(kind), C.byref(b), ptr(r)),
                    "lcv_create_updates")
        if n == 0:  # nothing ran: the pool is still the committees and the zero row
            out.nsc_pool[:views.ncomm] = keep["committees"]
        return out, r

    def download(self, rb: ResidentBatch, rows=None) -> PackedUpdates:
        """A resident batch back to the host (lcv_batch_download): every row, or `rows` in that order; the pool whole."""
        if rb.npool is None:
            raise ValueError("download: the batch's pool size is not known")
        ix = None if rows is None else np.ascontiguousarray(rows, np.uint32).reshape(-1)
        out = PackedUpdates.empty(rb.n if ix is None else ix.shape[0], rb.npool)
        if not rb.handle:
            return out
        b, keep = out.to_c()
        self._check(self.lib.lcv_batch_download(self.ctx, rb.handle, None if ix is None else ptr(ix, C.c_uint32),
                                                0 if ix is None else ix.shape[0], C.byref(b)), "lcv_batch_download")
        return out

    def rank_resident(self, rb: ResidentBatch) -> np.ndarray:
        """rank() of a resident batch where it lies (lcv_rank_resident): the same kernel, the same records."""
        out = np.zeros(rb.n, RANK_DTYPE)
        if rb.n:
            self._check(self.lib.lcv_rank_resident(self.ctx, rb.handle, ptr(out.view(np.uint8))), "lcv_rank_resident")
        return out

    # ------------------------------------------------------------------ SSZ wire bytes on the device (include/lcv.h)
    @staticmethod
    def _wire_fork(fork) -> int:
        f = WIRE_FORKS.get(fork, fork) if isinstance(fork, str) else fork
        return int(f)

    def encode_pitch(self, kind=0) -> int:
        """Bytes between consecutive messages of an encode call's output (lcv_encode_pitch)."""
        return int(self.lib.lcv_encode_pitch(self._kind(kind)))

    def _encoded_out(self, m: int, kind: int, out: Optional[EncodedMessages]) -> EncodedMessages:
        pitch = int(self.lib.lcv_encode_pitch(kind))
        if out is None:
            return EncodedMessages.empty(m, max(pitch, 16))
        if out.buf.shape != (m, pitch) or out.buf.dtype != np.uint8 or not out.buf.flags.c_contiguous:
            raise ValueError(f"out.buf: need C-contiguous uint8 ({m}, {pitch})")
        return out

    def encode_resident(self, rb: ResidentBatch, kind=0, fork="auto", rows=None,
                        out: Optional[EncodedMessages] = None) -> EncodedMessages:
        """The SSZ wire messages of a resident batch's rows, encoded on the device (lcv_batch_encode): every row, or
        `rows` in that order.  kind 0 / "update", 1 / "finality", 2 / "optimistic"; fork "deneb", "capella", "altair"
        for every row, or "auto": per row from the attested slot under the context's fork epochs.  `out`: arrays to
        write into (EncodedMessages.empty(m, encode_pitch(kind)))."""
        k, f = self._kind(kind), self._wire_fork(fork)
        ix = None if rows is None else np.ascontiguousarray(rows, np.uint32).reshape(-1)
        m = rb.n if ix is None else ix.shape[0]
        if not rb.handle and m == 0 and 0 <= k <= 2 and -1 <= f <= 2:
            return self._encoded_out(0, k, out)  # (an empty resident batch has no handle)
        e = self._encoded_out(m, k, out)
        self._check(self.lib.lcv_batch_encode(self.ctx, rb.handle, None if ix is None else ptr(ix, C.c_uint32),
                                              0 if ix is None else ix.shape[0], k, f, ptr(e.buf),
                                              ptr(e.length, C.c_uint32), ptr(e.fork), ptr(e.version), ptr(e.status)),
                    "lcv_batch_encode")
        return e

    def encode(self, batch: PackedUpdates, kind=0, fork="auto", out: Optional[EncodedMessages] = None) -> EncodedMessages:
        """encode_resident for rows that live on the host (lcv_encode_updates: upload, encode, free)."""
        k, f = self._kind(kind), self._wire_fork(fork)
        b, keep = batch.to_c()
        e = self._encoded_out(batch.n, k, out)
        self._check(self.lib.lcv_encode_updates(self.ctx, C.byref(b), k, f, ptr(e.buf), ptr(e.length, C.c_uint32),
                                                ptr(e.fork), ptr(e.version), ptr(e.status)), "lcv_encode_updates")
        return e

    def debug_set_encode_chunk(self, rows: int) -> None:
        """Test hook (lcv_debug_set_encode_chunk): rows per encode chunk; 0: as many as fit the scratch bound."""
        self._check(self.lib.lcv_debug_set_encode_chunk(self.ctx, int(rows)), "lcv_debug_set_encode_chunk")

    def decode_resident(self, messages, kind="update", fork="deneb") -> Tuple[ResidentBatch, np.ndarray]:
        """SSZ wire messages decoded on the device into a resident batch (lcv_batch_decode) -> (ResidentBatch, ok).
        `messages`, `kind` and `fork` (one name, or one per message) as lcv.wire.decode_updates takes them; the rows
        and ok are lcv.wire.decode_updates_status's (a malformed message: an all-zero row, ok False).  The relay
        path: decode_resident -> validate_resident -> encode_resident(rows=accepted), no row on the host."""
        from . import wire
        if kind not in wire.KINDS:
            raise ValueError(f"kind must be one of {list(wire.KINDS)}")
        buf, offs, lens = wire._flatten(messages)
        n = int(offs.size)
        fcode, forks = wire._fork_codes(fork, n)
        status = np.zeros(max(n, 1), np.uint8)
        src = buf if buf.size else np.zeros(1, np.uint8)
        o = offs if n else np.zeros(1, np.uint64)
        ln = lens if n else np.zeros(1, np.uint64)
        h = C.c_void_p()
        self._check(self.lib.lcv_batch_decode(self.ctx, ptr(src), int(buf.size), ptr(o, C.c_uint64), ptr(ln, C.c_uint64),
                                              n, wire.KINDS[kind], 0 if fcode is None else fcode,
                                              None if forks is None or not n else ptr(forks), ptr(status), C.byref(h)),
                    "lcv_batch_decode")
        if not h:
            return ResidentBatch(self, None, 0, npool=1), status[:0] == 0
        rows, npool = C.c_uint64(), C.c_uint64()
        self._check(self.lib.lcv_batch_shape(self.ctx, h, C.byref(rows), C.byref(npool)), "lcv_batch_shape")
        return ResidentBatch(self, h, n, npool=int(npool.value)), status[:n] == 0

    def last_decode_timings(self) -> Tuple[float, float]:
        """Kernel milliseconds of the last decode_resident (lcv_last_decode_timings): (the decode kernel's passes,
        the committee compares and the pool gather; 0.0 for finality and optimistic messages)."""
        ms = (C.c_float * 2)()
        self._check(self.lib.lcv_last_decode_timings(self.ctx, ms), "lcv_last_decode_timings")
        return float(ms[0]), float(ms[1])

    def debug_decode_hash_bits(self, bits: int) -> None:
        """Test hook (lcv_debug_decode_hash_bits): the committee hash of decode_resident's pool grouping truncated to
        `bits` bits (64: whole; 0: every committee collides, so only the full compares separate them)."""
        self._check(self.lib.lcv_debug_decode_hash_bits(self.ctx, int(bits)), "lcv_debug_decode_hash_bits")

    # ------------------------------------------------------------------ the asynchronous relay (include/lcv.h)
    def relay_async(self, messages, kind, fork, rows, store_index, current_slot: int, genesis_validators_root: bytes,
                    slot: int, fold_in: Optional[Sequence[FoldState]] = None) -> None:
        """Wire messages to per-store verdicts, enqueued on work-space slot `slot` without a wait (lcv_relay_async):
        pair i is message rows[i] for the store of table row store_index[i], validated against the table of
        set_store_table under the verifier's set_dedup / set_rlc settings.  `messages`, `kind` ("finality" or
        "optimistic"), `fork` as lcv.wire.decode_updates takes them.  `fold_in`: one FoldState per store row of the
        table -> the per-store fold as validate_stores_async_fold's.  Collect with slot_wait_relay(slot)."""
        from . import wire
        if kind not in wire.KINDS:
            raise ValueError(f"kind must be one of {list(wire.KINDS)}")
        buf, offs, lens = wire._flatten(messages)
        n = int(offs.size)
        fcode, forks = wire._fork_codes(fork, n)
        ix = np.ascontiguousarray(rows, np.uint32).reshape(-1)
        six = np.ascontiguousarray(store_index, np.uint32).reshape(-1)
        if ix.shape != six.shape:
            raise ValueError("one store_index per row")
        gvr = as_u8(bytes(genesis_validators_root))
        if gvr.size != 32:
            raise ValueError("genesis_validators_root: 32 bytes")
        src = buf if buf.size else np.zeros(1, np.uint8)
        o = offs if n else np.zeros(1, np.uint64)
        ln = lens if n else np.zeros(1, np.uint64)
        pix = ix if ix.size else np.zeros(1, np.uint32)
        psix = six if six.size else np.zeros(1, np.uint32)
        present, st = [], None
        if fold_in is not None:
            present = np.unique(six).tolist()
            self._fold_states_cover(fold_in, present)
            st = self._fold_states(fold_in, 1)
        rq = RelayRequest(ptr(src), int(buf.size), ptr(o, C.c_uint64), ptr(ln, C.c_uint64), n, wire.KINDS[kind],
                          0 if fcode is None else fcode, None if forks is None or not n else ptr(forks),
                          ptr(pix, C.c_uint32), ptr(psix, C.c_uint32), int(ix.size), int(current_slot), ptr(gvr), st)
        self._check(self.lib.lcv_relay_async(self.ctx, C.byref(rq), int(slot)), "lcv_relay_async")
        self._slot_batch[int(slot)] = (n, int(ix.size), None if fold_in is None else len(fold_in), present)

    def slot_wait_relay(self, slot: int):
        """Wait for the relay enqueued on `slot` -> (ok: message j decoded, verdicts, reason codes[, fold results: one
        FoldResult per store row, None for stores without a pair — only for a relay enqueued with fold_in]); LcvError
        (status -4) if the slot's last batch was not a relay."""
        nmsg, npairs, nfold, present = self._slot_batch.get(int(slot), (0, 0, None, []))
        status = np.ones(max(nmsg, 1), np.uint8)
        v = np.zeros(max(npairs, 1), np.uint8)
        r = np.zeros(max(npairs, 1), np.uint8)
        res = None if nfold is None else (FoldResultC * max(1, nfold))()
        self._check(self.lib.lcv_slot_wait_relay(self.ctx, int(slot), ptr(status), ptr(v), ptr(r), res),
                    "lcv_slot_wait_relay")
        out = (status[:nmsg] == 0, v[:npairs].astype(bool), r[:npairs])
        return out if nfold is None else out + (self._fold_results(res, present)[:nfold],)

    def last_relay_timings(self, slot: int) -> Tuple[float, float]:
        """Device milliseconds of the last relay on `slot` (lcv_last_relay_timings; waits for its kernel): (decode +
        fan-out kernel, 0.0)."""
        ms = (C.c_float * 2)()
        self._check(self.lib.lcv_last_relay_timings(self.ctx, int(slot), ms), "lcv_last_relay_timings")
        return float(ms[0]), float(ms[1])

    def create_bootstraps(self, views: PackedViews, state_idx, block_idx, reason: Optional[np.ndarray] = None):
        """create_light_client_bootstrap per (state_idx[i], block_idx[i]) (lcv_create_bootstraps) -> (beacon (n, 112),
        execution (n, 832), exec_branch (n, 128), committee_index (n,), committee_branch (n, 160), reasons): the
        columns bootstrap_check_batch takes, the committee as a row of views.committees (views.ncomm for a failed
        row).  reasons: 0, 1 state before Altair, 2 state slot, 3 header root != block root, 4 missing payload."""
        sv, bv, com, keep = views.to_c()
        si = np.ascontiguousarray(state_idx, np.uint32).reshape(-1)
        bi = np.ascontiguousarray(block_idx, np.uint32).reshape(-1)
        if si.shape != bi.shape:
            raise ValueError("need one block per state")
        n = si.shape[0]
        beacon, execution, branch = np.zeros((n, 112), np.uint8), np.zeros((n, 832), np.uint8), np.zeros((n, 128), np.uint8)
        cidx, cbranch = np.zeros(n, np.uint32), np.zeros((n, 160), np.uint8)
        r = reason if reason is not None else np.zeros(n, np.uint8)
        self._check(self.lib.lcv_create_bootstraps(self.ctx, C.byref(sv), views.ns, C.byref(bv), views.nb, com,
                                                   views.ncomm, ptr(si, C.c_uint32), ptr(bi, C.c_uint32), n, ptr(beacon),
                                                   ptr(execution), ptr(branch), ptr(cidx, C.c_uint32), ptr(cbranch),
                                                   ptr(r)), "lcv_create_bootstraps")
        return beacon, execution, branch, cidx, cbranch, r

    def validate_resident(self, rb: ResidentBatch, current_slot: int, genesis_validators_root: bytes,
                          verdict: Optional[np.ndarray] = None, reason: Optional[np.ndarray] = None):
        gvr = as_u8(bytes(genesis_validators_root))
        v = verdict if verdict is not None else np.zeros(rb.n, np.uint8)
        r = reason if reason is not None else np.zeros(rb.n, np.uint8)
        self._check(self.lib.lcv_validate_resident(self.ctx, rb.handle, int(current_slot), ptr(gvr), ptr(v), ptr(r)),
                    "lcv_validate_resident")
        return v, r

    def validate_resident_dev(self, rb: ResidentBatch, current_slot: int, genesis_validators_root: bytes,
                              verdict_dev_ptr: int):
        gvr = as_u8(bytes(genesis_validators_root))
        self._check(self.lib.lcv_validate_resident_dev(self.ctx, rb.handle, int(current_slot), ptr(gvr),
                                                       C.c_void_p(verdict_dev_ptr)), "lcv_validate_resident_dev")

    def validate_resident_async(self, rb: ResidentBatch, current_slot: int, genesis_validators_root: bytes,
                                slot: int) -> None:
        """Enqueue the whole pipeline for rb on work-space slot 0..7 and return at once (up to eight
        batches in flight); collect the verdicts with slot_wait(slot)."""
        gvr = as_u8(bytes(genesis_validators_root))  # (the call reads it before returning)
        self._check(self.lib.lcv_validate_resident_async(self.ctx, rb.handle, int(current_slot), ptr(gvr), int(slot)),
                    "lcv_validate_resident_async")

    def validate_async(self, batch: PackedUpdates, current_slot: int, genesis_validators_root: bytes,
                       slot: int) -> None:
        """Host-input serving entry (lcv_validate_async): the batch is staged into slot 0..7's pinned buffer,
        uploaded, validated and its verdicts copied back, all enqueued; collect them with slot_wait(slot).
        The batch's arrays may be reused as soon as this returns."""
        b, keep = batch.to_c()
        gvr = as_u8(bytes(genesis_validators_root))
        self._check(self.lib.lcv_validate_async(self.ctx, C.byref(b), int(current_slot), ptr(gvr), int(slot)),
                    "lcv_validate_async")
        del keep

    def validate_stores_async(self, batch: PackedUpdates, store_index, current_slot: int,
                              genesis_validators_root: bytes, slot: int) -> None:
        """validate_async against the store table (lcv_validate_stores_async): update i against store row
        store_index[i].  Every index is checked on the host before anything is enqueued; collect the verdicts
        with slot_wait(slot).  The arrays may be reused as soon as this returns."""
        b, keep = batch.to_c()
        six = self._store_index(batch, store_index)
        gvr = as_u8(bytes(genesis_validators_root))
        self._check(self.lib.lcv_validate_stores_async(self.ctx, C.byref(b), ptr(six, C.c_uint32), int(current_slot),
                                                       ptr(gvr), int(slot)), "lcv_validate_stores_async")
        del keep

    # ------------------------------------------------------------------ store fold (include/lcv.h)
    def rank(self, batch: PackedUpdates) -> np.ndarray:
        """The rank record of every update (lcv_rank_updates) as a RANK_DTYPE array; no store needed."""
        b, keep = batch.to_c()
        out = np.zeros(batch.n, RANK_DTYPE)
        if batch.n:
            self._check(self.lib.lcv_rank_updates(self.ctx, C.byref(b), ptr(out.view(np.uint8))), "lcv_rank_updates")
        return out

    def _no_table_fold(self, store_index, what: str) -> None:
        if store_index is not None:  # the C entries take no store_index: a table batch has no fold
            raise LcvError(f"{what}: status -1: no fold of a store-table batch (a batch with a store_index)")

    def validate_fold(self, batch: PackedUpdates, current_slot: int, genesis_validators_root: bytes,
                      state: FoldState, store_index=None):
        """validate + the device fold of process_light_client_update's post-validation logic over the batch
        (lcv_validate_fold; at most 65,536 rows) -> (verdicts, reason codes, FoldResult)."""
        self._no_table_fold(store_index, "lcv_validate_fold")
        b, keep = batch.to_c()
        gvr = as_u8(bytes(genesis_validators_root))
        v = np.zeros(batch.n, np.uint8)
        r = np.zeros(batch.n, np.uint8)
        st, res = state.to_c(), FoldResultC()
        self._check(self.lib.lcv_validate_fold(self.ctx, C.byref(b), int(current_slot), ptr(gvr), C.byref(st), ptr(v),
                                               ptr(r), C.byref(res)), "lcv_validate_fold")
        return v.astype(bool), r, FoldResult.from_c(res)

    def validate_async_fold(self, batch: PackedUpdates, current_slot: int, genesis_validators_root: bytes,
                            state: FoldState, slot: int, store_index=None) -> None:
        """validate_async with the fold (lcv_validate_async_fold); collect with slot_wait_fold(slot)."""
        self._no_table_fold(store_index, "lcv_validate_async_fold")
        b, keep = batch.to_c()
        gvr = as_u8(bytes(genesis_validators_root))
        st = state.to_c()
        self._check(self.lib.lcv_validate_async_fold(self.ctx, C.byref(b), int(current_slot), ptr(gvr), C.byref(st),
                                                     int(slot)), "lcv_validate_async_fold")
        del keep

    def slot_wait_fold(self, slot: int, n: int):
        """Wait for the folded batch of `slot` -> (verdicts, reason codes, FoldResult); LcvError (status -4) if
        the slot's batch was not enqueued with a fold."""
        v = np.zeros(n, np.uint8)
        r = np.zeros(n, np.uint8)
        res = FoldResultC()
        self._check(self.lib.lcv_slot_wait_fold(self.ctx, int(slot), int(n), ptr(v), ptr(r), C.byref(res)),
                    "lcv_slot_wait_fold")
        return v.astype(bool), r, FoldResult.from_c(res)

    def debug_fold(self, rank: np.ndarray, verdict: np.ndarray, store_finalized_slot: int, next_known: bool,
                   state: FoldState) -> FoldResult:
        """Test hook (lcv_debug_fold): the fold kernel alone on caller-supplied rank records and verdicts."""
        rk = np.ascontiguousarray(rank, RANK_DTYPE)
        vd = np.ascontiguousarray(verdict, np.uint8)
        if rk.shape != vd.shape or rk.ndim != 1:
            raise ValueError("need one verdict per rank record")
        st, res = state.to_c(), FoldResultC()
        self._check(self.lib.lcv_debug_fold(self.ctx, ptr(rk.view(np.uint8)), ptr(vd), rk.shape[0],
                                            int(store_finalized_slot), 1 if next_known else 0, C.byref(st),
                                            C.byref(res)), "lcv_debug_fold")
        return FoldResult.from_c(res)

    # ------------------------------------------------------------------ the fold of a store-table batch, per store
    @staticmethod
    def _fold_states(states, rows: int = 0):
        arr = (FoldStateC * max(len(states), rows))()
        for k, s in enumerate(states):
            arr[k] = s.to_c()
        return arr

    @staticmethod
    def _fold_states_cover(states, present) -> None:
        if present and present[-1] >= len(states):
            raise ValueError(f"store_index names store row {present[-1]} but only {len(states)} fold states were given")

    @staticmethod
    def _fold_results(res, present) -> list:
        """One FoldResult per store row; None for the stores `present` does not name (their entries are not
        written by the C entries)."""
        out = [None] * len(res)
        for s in present:
            out[s] = FoldResult.from_c(res[s])
        return out

    def validate_stores_fold(self, batch: PackedUpdates, store_index, current_slot: int,
                             genesis_validators_root: bytes, states: Sequence[FoldState]):
        """validate_stores + the device fold per store (lcv_validate_stores_fold; at most 65,536 rows): update i is
        validated against store row store_index[i] and folded with that store's other rows, in batch order, from
        states[store_index[i]] -> (verdicts, reason codes, results).  `states`: one FoldState per store row of the
        table; `results`: one FoldResult per store row, None for stores without a row in the batch.  The results'
        apply_row / best_row / optimistic_row are batch rows; row i of store s was consumed iff
        results[s].apply_row < 0 or i <= results[s].apply_row."""
        b, keep = batch.to_c()
        six = self._store_index(batch, store_index)
        gvr = as_u8(bytes(genesis_validators_root))
        v = np.zeros(batch.n, np.uint8)
        r = np.zeros(batch.n, np.uint8)
        present = np.unique(six).tolist()
        rows = max(len(states), present[-1] + 1 if present else 0, 1)  # (the C entry names a store_index out of range)
        st, res = self._fold_states(states, rows), (FoldResultC * rows)()
        self._check(self.lib.lcv_validate_stores_fold(self.ctx, C.byref(b), ptr(six, C.c_uint32), int(current_slot),
                                                      ptr(gvr), st, ptr(v), ptr(r), res), "lcv_validate_stores_fold")
        self._fold_states_cover(states, present)
        return v.astype(bool), r, self._fold_results(res, present)[:len(states)]

    def validate_stores_async_fold(self, batch: PackedUpdates, store_index, current_slot: int,
                                   genesis_validators_root: bytes, states: Sequence[FoldState], slot: int) -> None:
        """validate_stores_async with the fold per store (lcv_validate_stores_async_fold); collect with
        slot_wait_stores_fold(slot, n, nstore)."""
        b, keep = batch.to_c()
        six = self._store_index(batch, store_index)
        gvr = as_u8(bytes(genesis_validators_root))
        present = np.unique(six).tolist()
        self._fold_states_cover(states, present)
        st = self._fold_states(states)
        self._check(self.lib.lcv_validate_stores_async_fold(self.ctx, C.byref(b), ptr(six, C.c_uint32), int(current_slot),
                                                            ptr(gvr), st, int(slot)), "lcv_validate_stores_async_fold")
        self._slot_batch[int(slot)] = (0, 0, None, present)
        del keep

    def slot_wait_stores_fold(self, slot: int, n: int, nstore: int):
        """Wait for the table batch folded on `slot` -> (verdicts, reason codes, results: one FoldResult per store
        row, None for stores without a row); LcvError (status -4) if the slot's batch was not enqueued by
        validate_stores_async_fold."""
        v = np.zeros(n, np.uint8)
        r = np.zeros(n, np.uint8)
        res = (FoldResultC * max(1, int(nstore)))()
        self._check(self.lib.lcv_slot_wait_stores_fold(self.ctx, int(slot), int(n), ptr(v), ptr(r), res),
                    "lcv_slot_wait_stores_fold")
        present = self._slot_batch.get(int(slot), (0, 0, None, []))[3]
        return v.astype(bool), r, self._fold_results(res, present)[:int(nstore)]

    def debug_fold_stores(self, rank: np.ndarray, verdict: np.ndarray, store_index, store_finalized_slot, next_known,
                          states: Sequence[FoldState], out=None) -> list:
        """Test hook (lcv_debug_fold_stores): the segmented fold kernel alone on caller-supplied rank records,
        verdicts and store rows; store s has finalized slot store_finalized_slot[s] and next_known[s].  `out`
        (optional FoldResultC array, one per store) receives the raw results, so a caller can see which entries
        were written."""
        rk = np.ascontiguousarray(rank, RANK_DTYPE)
        vd = np.ascontiguousarray(verdict, np.uint8)
        six = np.ascontiguousarray(store_index, np.uint32).reshape(-1)
        fin = np.ascontiguousarray(store_finalized_slot, np.uint64).reshape(-1)
        nk = np.ascontiguousarray(next_known, np.uint8).reshape(-1)
        if rk.ndim != 1 or rk.shape != vd.shape or rk.shape != six.shape:
            raise ValueError("need one verdict and one store_index per rank record")
        if not (fin.shape[0] == nk.shape[0] == len(states)) or not len(states):
            raise ValueError("need one finalized slot, one next_known and one fold state per store")
        st = self._fold_states(states)
        res = out if out is not None else (FoldResultC * len(states))()
        self._check(self.lib.lcv_debug_fold_stores(self.ctx, ptr(rk.view(np.uint8)), ptr(vd), ptr(six, C.c_uint32),
                                                   rk.shape[0], ptr(fin, C.c_uint64), ptr(nk), fin.shape[0], st, res),
                    "lcv_debug_fold_stores")
        return self._fold_results(res, [s for s in np.unique(six).tolist() if s < len(states)])

    def event_pool(self) -> int:
        """HIP events held for stage timings (test hook: must stay bounded under asynchronous calls)."""
        n = C.c_uint64()
        self._check(self.lib.lcv_debug_event_pool(self.ctx, C.byref(n)), "lcv_debug_event_pool")
        return int(n.value)

    def slot_wait(self, slot: int, n: int, verdict: Optional[np.ndarray] = None, reason: Optional[np.ndarray] = None):
        """Wait for the batch of `slot`; its first n verdicts (bool) and reason codes."""
        v = verdict if verdict is not None else np.zeros(n, np.uint8)
        r = reason if reason is not None else np.zeros(n, np.uint8)
        self._check(self.lib.lcv_slot_wait(self.ctx, int(slot), int(n), ptr(v), ptr(r)), "lcv_slot_wait")
        return v, r

    # ------------------------------------------------------------------ BLS / SSZ primitives
    def fast_aggregate_verify(self, pubkeys: Sequence[bytes], message: bytes, signature: bytes) -> bool:
        pks = as_u8(b"".join(bytes(p) for p in pubkeys)) if len(pubkeys) else np.zeros(1, np.uint8)
        if any(len(bytes(p)) != 48 for p in pubkeys):
            return False
        msg, sig = bytes(message), bytes(signature)
        if len(sig) != 96:
            return False
        m = as_u8(msg) if msg else np.zeros(1, np.uint8)
        res = C.c_int()
        self._check(self.lib.lcv_fast_aggregate_verify(self.ctx, ptr(pks), len(pubkeys), ptr(m), len(msg),
                                                       ptr(as_u8(sig)), C.byref(res)), "lcv_fast_aggregate_verify")
        return bool(res.value)

    def fast_aggregate_verify_batch(self, committees: np.ndarray, committee_id: np.ndarray, bits: np.ndarray,
                                    msgs: np.ndarray, sigs: np.ndarray) -> np.ndarray:
        committees = np.ascontiguousarray(committees, np.uint8).reshape(-1, 512 * 48)
        cid = np.ascontiguousarray(committee_id, np.uint32)
        bits = np.ascontiguousarray(bits, np.uint8).reshape(-1, 64)
        msgs = np.ascontiguousarray(msgs, np.uint8).reshape(-1, 32)
        sigs = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 96)
        n = cid.shape[0]
        out = np.zeros(n, np.uint8)
        self._check(self.lib.lcv_fast_aggregate_verify_batch(self.ctx, ptr(committees), committees.shape[0],
                                                             ptr(cid, C.c_uint32), ptr(bits), ptr(msgs), ptr(sigs), n,
                                                             ptr(out)), "lcv_fast_aggregate_verify_batch")
        return out.astype(bool)

    def merkle_branch_batch(self, leaves: np.ndarray, branches: np.ndarray, depth: int, index: int,
                            roots: np.ndarray) -> np.ndarray:
        leaves = np.ascontiguousarray(leaves, np.uint8).reshape(-1, 32)
        n = leaves.shape[0]
        branches = np.ascontiguousarray(branches, np.uint8).reshape(n, 32 * depth) if depth else np.zeros((n, 0), np.uint8)
        roots = np.ascontiguousarray(roots, np.uint8).reshape(n, 32)
        out = np.zeros(n, np.uint8)
        br = branches if depth else np.zeros(32, np.uint8)
        self._check(self.lib.lcv_merkle_branch_batch(self.ctx, ptr(leaves), ptr(np.ascontiguousarray(br)), int(depth),
                                                     int(index), ptr(roots), n, ptr(out)), "lcv_merkle_branch_batch")
        return out.astype(bool)

    def htr_sync_committee_batch(self, committees: np.ndarray) -> np.ndarray:
        committees = np.ascontiguousarray(committees, np.uint8).reshape(-1, SYNC_COMMITTEE_BYTES)
        n = committees.shape[0]
        out = np.zeros((n, 32), np.uint8)
        self._check(self.lib.lcv_htr_sync_committee_batch(self.ctx, ptr(committees), n, ptr(out)),
                    "lcv_htr_sync_committee_batch")
        return out

    def bootstrap_check_batch(self, beacon: np.ndarray, execution: np.ndarray, exec_branch: np.ndarray,
                              committees: np.ndarray, committee_branch: np.ndarray, trusted_roots: np.ndarray
                              ) -> np.ndarray:
        """initialize_light_client_store's asserts (sync-protocol.md:353-362) per row -> reason codes
        (0 ok, 1 header, 2 trusted root, 3 current_sync_committee branch)."""
        beacon = np.ascontiguousarray(beacon, np.uint8).reshape(-1, 112)
        n = beacon.shape[0]
        cols = [beacon, np.ascontiguousarray(execution, np.uint8).reshape(n, EXEC_RECORD_BYTES),
                np.ascontiguousarray(exec_branch, np.uint8).reshape(n, 128),
                np.ascontiguousarray(committees, np.uint8).reshape(n, SYNC_COMMITTEE_BYTES),
                np.ascontiguousarray(committee_branch, np.uint8).reshape(n, 160),
                np.ascontiguousarray(trusted_roots, np.uint8).reshape(n, 32)]
        out = np.zeros(n, np.uint8)
        self._check(self.lib.lcv_bootstrap_check_batch(self.ctx, *[ptr(c) for c in cols], n, ptr(out)),
                    "lcv_bootstrap_check_batch")
        return out

    def sk_to_pk_batch(self, sks: np.ndarray) -> np.ndarray:
        sks = np.ascontiguousarray(sks, np.uint8).reshape(-1, 32)
        out = np.zeros((sks.shape[0], 48), np.uint8)
        self._check(self.lib.lcv_sk_to_pk_batch(self.ctx, ptr(sks), sks.shape[0], ptr(out)), "lcv_sk_to_pk_batch")
        return out

    def sign_batch(self, sks: np.ndarray, msgs: np.ndarray) -> np.ndarray:
        sks = np.ascontiguousarray(sks, np.uint8).reshape(-1, 32)
        msgs = np.ascontiguousarray(msgs, np.uint8).reshape(-1, 32)
        out = np.zeros((sks.shape[0], 96), np.uint8)
        self._check(self.lib.lcv_sign_batch(self.ctx, ptr(sks), ptr(msgs), sks.shape[0], ptr(out)), "lcv_sign_batch")
        return out

    # ------------------------------------------------------------------ parity-test entry points
    def debug_fp(self, a: np.ndarray, b: np.ndarray):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 48)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 48)
        n = a.shape[0]
        out = np.zeros((n, 288), np.uint8)
        ok = np.zeros(n, np.uint8)
        self._check(self.lib.lcv_debug_fp(self.ctx, ptr(a), ptr(b), n, ptr(out), ptr(ok)), "lcv_debug_fp")
        return out, ok

    def debug_fp_pow(self, a: np.ndarray) -> np.ndarray:
        """(n, 96): a^((p+1)/4) || a^((p-3)/4), canonical big-endian."""
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 48)
        out = np.zeros((a.shape[0], 96), np.uint8)
        self._check(self.lib.lcv_debug_fp_pow(self.ctx, ptr(a), a.shape[0], ptr(out)), "lcv_debug_fp_pow")
        return out

    def debug_hash_to_g2(self, msgs: np.ndarray):
        msgs = np.ascontiguousarray(msgs, np.uint8).reshape(-1, 32)
        n = msgs.shape[0]
        out = np.zeros((n, 192), np.uint8)
        inf = np.zeros(n, np.uint8)
        self._check(self.lib.lcv_debug_hash_to_g2(self.ctx, ptr(msgs), n, ptr(out), ptr(inf)), "lcv_debug_hash_to_g2")
        return out, inf

    def debug_g2_decompress(self, sigs: np.ndarray):
        sigs = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 96)
        n = sigs.shape[0]
        out = np.zeros((n, 192), np.uint8)
        st = np.zeros(n, np.uint8)
        self._check(self.lib.lcv_debug_g2_decompress(self.ctx, ptr(sigs), n, ptr(out), ptr(st)),
                    "lcv_debug_g2_decompress")
        return out, st

    def debug_aggregate(self, committees: np.ndarray, committee_id: np.ndarray, bits: np.ndarray):
        committees = np.ascontiguousarray(committees, np.uint8).reshape(-1, 512 * 48)
        cid = np.ascontiguousarray(committee_id, np.uint32)
        bits = np.ascontiguousarray(bits, np.uint8).reshape(-1, 64)
        n = cid.shape[0]
        out = np.zeros((n, 96), np.uint8)
        st = np.zeros(n, np.uint8)
        self._check(self.lib.lcv_debug_aggregate(self.ctx, ptr(committees), committees.shape[0], ptr(cid, C.c_uint32),
                                                 ptr(bits), n, ptr(out), ptr(st)), "lcv_debug_aggregate")
        return out, st

    def debug_pairing(self, p96: np.ndarray, q192: np.ndarray) -> np.ndarray:
        p96 = np.ascontiguousarray(p96, np.uint8).reshape(-1, 96)
        q192 = np.ascontiguousarray(q192, np.uint8).reshape(-1, 192)
        n = p96.shape[0]
        out = np.zeros((n, 576), np.uint8)
        self._check(self.lib.lcv_debug_pairing(self.ctx, ptr(p96), ptr(q192), n, ptr(out)), "lcv_debug_pairing")
        return out
