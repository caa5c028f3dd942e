#!/usr/bin/env python3
"""Generate tests/golden/lc_boundaries.npz + lc_boundaries.json (run where the reference is available, like
make_golden.py; minutes on the CPU):

    python tests/golden/make_boundary_golden.py

Light-client updates whose slots are CHOSEN to sit on the points where validate_light_client_update changes its
answer, under the small configuration of producer_batch_cases.small_config() (8 slots per epoch, 8 epochs per
period: Altair from slot 8, Bellatrix 16, Capella 24, Deneb 40; periods from 64 and 128).  Every row is
lcv.producer.create_light_client_update over hand-placed block and state views (finalized block <- attested block <-
signature block); the participants sign through the host simulation's signer.  A twin that differs from a derived
row only in its sync aggregate (other participants, or a signing root under another fork version) is that row with
the aggregate of another signature block over the same attested block; a corrupted twin is the row with the named
bytes replaced.

The expected reason of every case is the failing assert of the reference's OWN exec'd validate_light_client_update
(make_golden.load_reference over oracle/spec.py switched to the configuration), and oracle/sync_protocol.py must
agree on every case.  Nothing of the reference is stored: inputs and reason codes only.

Families (tests/boundary_cases.py replays them; the case names state the slots):
  V  fork version of the signing root: (attested, signature) pairs around every fork epoch's first slot, and their
     twins signed under the neighbouring version
  H  is_valid_light_client_header at the Capella and Deneb epochs, attested and finalized header, both shapes of the
     execution root, extra_data lengths 0 / 1 / 31 / 32 (store finalized at slot 1; G at 2, N at 3: the same
     verdicts as at 0, and a store table whose rows differ)
  S  slot ordering: current_slot, signature_slot, attested and finalized slot one apart and equal; slots around 2^63
  P  sync-committee periods: the signature's period against the store's, committee selection, the :442 equality
  R  relevance: attested slot against the store's finalized slot, and the route through has_next
  G  finality: genesis, default and corrupted finalized headers and branches
  N  participation counts 1, 255 .. 258, 511, 512 on the validate path, and 0
"""
from __future__ import annotations

import json
import os
import sys
from dataclasses import replace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import helpers as H  # noqa: E402
import boundary_cases as BC  # noqa: E402
import golden_cases as G  # noqa: E402
import producer_batch_cases as PB  # noqa: E402
from make_golden import load_reference, reference_reason, to_reference_objects  # noqa: E402

from lcv import producer as PR  # noqa: E402
from lcv import synth  # noqa: E402
from oracle import spec as S  # noqa: E402

FULL = b"\xff" * 64
T63 = 1 << 63
CUR = 200  # current_slot of the cases that are not about it (past every small signature slot)
NOTES = [
    "V (7,8) and V0 (0,1): create_light_client_update refuses an attested state before Altair (full-node.md:143), so "
    "these rows are derived with ALTAIR_FORK_EPOCH = 0 for the derivation alone; signing and validation use the "
    "configuration as stored (validate_light_client_update has no Altair check).",
    "P 'store finalized 63 with signature slot 64' cannot be valid: the attested slot would have to lie above 63 and "
    "below 64.  The nearest chain is used: store finalized 62, attested 63, signature 64; store finalized 63 is kept "
    "as the case that fails :411.",
    "P 'attested 63 / signature 64 carrying a next-sync-committee branch': the producer leaves next_sync_committee "
    "out where the attested and signature periods differ (full-node.md:165), so the derived row is completed with "
    "attested_state.next_sync_committee and its proof at gindex 55, as a provider that always sends them would.",
    "G 'finality branch present with a default non-genesis header': a row derived with a real finalized block whose "
    "finalized header is then replaced by the default one; its slot 0 takes the genesis route and the zero leaf "
    "fails the branch.",
]


def poke(b: bytes, off: int, val: int) -> bytes:
    return b[:off] + bytes([val]) + b[off + 1:]


def bits_of(idx) -> bytes:
    b = np.zeros(512, np.uint8)
    b[list(idx)] = 1
    return np.packbits(b, bitorder="little").tobytes()


def version_root(att_beacon: bytes, version: bytes, gvr: bytes, cfg) -> bytes:
    """compute_signing_root(attested beacon, compute_domain(DOMAIN_SYNC_COMMITTEE, version, gvr))."""
    fdr = synth.sha256(version + bytes(28) + gvr)
    return synth.sha256(PR.htr_beacon(att_beacon) + cfg.DOMAIN_SYNC_COMMITTEE + fdr[:28])


class Builder:
    def __init__(self, v):
        self.v, self.cfg = v, PB.small_config()
        self.rng = np.random.default_rng(20251)
        g = G.load_updates()
        self.pool, self.gvr = g["nsc_pool"], g["genesis_validators_root"].tobytes()
        self.com = [synth.make_committee(v, 0), synth.make_committee(v, 1)]
        assert self.pool[0].tobytes() == self.com[0].ssz and self.pool[1].tobytes() == self.com[1].ssz
        assert not self.pool[2].any() and self.pool.shape[0] == 3
        self.row_index, self.rows, self.sig_slots = {}, [], []
        self.cases = []

    # ---------------------------------------------------------------- views
    def block(self, slot, parent=None, bits=FULL, sig=bytes(96), payload=True, deneb=None, extra_len=0, blob=None):
        """A block view at `slot`; from Capella on with an execution record of `extra_len` bytes of extra_data.
        deneb / blob: the shape of the payload's root (17 or 15 leaves) and whether the blob fields are non-zero;
        by default what the slot's fork says."""
        cfg, rng = self.cfg, self.rng
        epoch = cfg.compute_epoch_at_slot(slot)
        is_deneb = epoch >= cfg.DENEB_FORK_EPOCH
        execution = None
        if payload and epoch >= cfg.CAPELLA_FORK_EPOCH:
            execution = PB._exec_record(rng, extra_len, blob_fields=is_deneb if blob is None else blob)
        return PR.BeaconBlockView(slot=slot, proposer_index=int(rng.integers(0, 1 << 20)),
                                  parent_root=parent if parent is not None else rng.bytes(32), state_root=bytes(32),
                                  sync_committee_bits=bits, sync_committee_signature=sig, execution=execution,
                                  execution_deneb=is_deneb if deneb is None else deneb,
                                  body_roots=rng.integers(0, 256, (PR.BODY_FIELDS, 32), dtype=np.uint8))

    def with_state(self, blk, fin_epoch, fin_root, nxt):
        hdr = blk.header()
        st = PR.BeaconStateView(slot=blk.slot, latest_block_header=hdr[:48] + bytes(32) + hdr[80:],
                                finalized_checkpoint_epoch=fin_epoch, finalized_checkpoint_root=fin_root,
                                current_sync_committee=self.com[0].ssz, next_sync_committee=nxt,
                                field_roots=self.rng.integers(0, 256, (PR.STATE_FIELDS, 32), dtype=np.uint8))
        return st, replace(blk, state_root=st.hash_tree_root())

    # ---------------------------------------------------------------- signing and derivation
    def signature(self, att_beacon, sig_slot, signer, bits, version=None) -> bytes:
        """The sync aggregate signature of committee `signer`'s members `bits` over the attested header, under the
        fork version of epoch(max(sig_slot, 1) - 1) (sync-protocol.md:460), or under `version`."""
        cfg = self.cfg
        natural = cfg.compute_fork_version(cfg.compute_epoch_at_slot(max(sig_slot, 1) - 1))
        msg = version_root(att_beacon, version or natural, self.gvr, cfg)
        if version is None:
            assert msg == synth.signing_root(att_beacon, sig_slot, self.gvr, cfg)
        else:
            assert version != natural
        idx = np.flatnonzero(np.unpackbits(np.frombuffer(bits, np.uint8), bitorder="little"))
        sk = sum(self.com[signer].sks[j] for j in idx) % synth.R_ORDER
        assert sk
        return self.v.sign_batch(np.frombuffer(sk.to_bytes(32, "big"), np.uint8), np.frombuffer(msg, np.uint8))[0].tobytes()

    def derive(self, att, sig, signer=0, bits=FULL, fin=None, nsc=1, carry=False, **att_kw):
        """create_light_client_update over the chain [finalized block `fin` (a slot, a view or "genesis")] <-
        attested block at `att` <- signature block at `sig`, signed by committee `signer`; the attested state
        holds pool row `nsc` as its next sync committee."""
        cfg = self.cfg
        fin_blk, fin_epoch, fin_root = None, 0, self.rng.bytes(32)
        if isinstance(fin, str):
            fin_blk, fin_root = self.block(0), bytes(32)
        elif fin is not None:
            fin_blk = fin if isinstance(fin, PR.BeaconBlockView) else self.block(fin)
            fin_epoch, fin_root = cfg.compute_epoch_at_slot(fin_blk.slot), fin_blk.hash_tree_root()
        att_state, att_blk = self.with_state(self.block(att, **att_kw), fin_epoch, fin_root, self.pool[nsc].tobytes())
        signature = self.signature(att_blk.header(), sig, signer, bits)
        blk = self.block(sig, parent=att_blk.hash_tree_root(), bits=bits, sig=signature, payload=False)
        st, blk = self.with_state(blk, fin_epoch, fin_root, att_state.next_sync_committee)
        dcfg = cfg if cfg.compute_epoch_at_slot(att) >= cfg.ALTAIR_FORK_EPOCH else cfg.with_(ALTAIR_FORK_EPOCH=0)
        u = PR.create_light_client_update(st, blk, att_state, att_blk, fin_blk, dcfg)
        same_period = cfg.compute_sync_committee_period_at_slot(att) == cfg.compute_sync_committee_period_at_slot(sig)
        assert (u.next_sync_committee_branch != bytes(160)) == same_period
        if carry:
            assert not same_period
            u = replace(u, next_sync_committee=bytes(att_state.next_sync_committee),
                        next_sync_committee_branch=b"".join(PR.compute_merkle_proof(att_state, PR.NEXT_SYNC_COMMITTEE_GINDEX)))
        return u

    def resigned(self, u, signer=0, bits=None, version=None):
        """u with the aggregate of another signature block over the same attested block."""
        bits = u.sync_committee_bits if bits is None else bits
        return replace(u, sync_committee_bits=bits,
                       sync_committee_signature=self.signature(u.attested_header.beacon, u.signature_slot, signer, bits, version))

    # ---------------------------------------------------------------- cases
    def case(self, family, name, u, store_fin, next_known, current=CUR, pool=None, **over):
        h, f = u.attested_header, u.finalized_header
        cols = dict(att_beacon=h.beacon, att_exec=h.execution, att_branch=h.execution_branch, fin_beacon=f.beacon,
                    fin_exec=f.execution, fin_branch=f.execution_branch, nsc_branch=u.next_sync_committee_branch,
                    finality_branch=u.finality_branch, sync_bits=u.sync_committee_bits,
                    sync_signature=u.sync_committee_signature)
        sig_slot = int(over.pop("signature_slot", u.signature_slot))
        assert set(over) <= set(cols), over.keys()
        cols.update(over)
        key = tuple(bytes(cols[k]) for k in G.COLS) + (sig_slot,)
        if key not in self.row_index:
            self.row_index[key] = len(self.rows)
            self.rows.append(key[:-1])
            self.sig_slots.append(sig_slot)
        if pool is None:
            pool = [self.pool[k].tobytes() for k in range(3)].index(bytes(u.next_sync_committee))
        assert name not in [c["name"] for c in self.cases], name
        self.cases.append(dict(family=family, name=name, row=self.row_index[key], store_fin=store_fin,
                               next_known=int(next_known), current=current, pool=pool))


def build(v) -> Builder:
    b = Builder(v)
    cfg = b.cfg
    versions = cfg.fork_versions()
    vname = ("genesis", "altair", "bellatrix", "capella", "deneb")

    # ---- V: the fork version of the signing root, at every fork epoch's first slot
    pair_rows = {}
    extra = {(24, 25): 0, (39, 40): 1, (40, 41): 31}
    for att, sig in ((7, 8), (8, 9), (15, 16), (16, 17), (23, 24), (24, 25), (39, 40), (40, 41)):
        u = pair_rows[(att, sig)] = b.derive(att, sig, extra_len=extra.get((att, sig), 0))
        b.case("V", f"V_att{att}_sig{sig}", u, 0, 1)
    for k, first in enumerate((8, 16, 24, 40)):  # fork k + 1 starts at slot `first`
        later, earlier = pair_rows[(first, first + 1)], pair_rows[(first - 1, first)]
        b.case("V", f"V_att{first}_sig{first + 1}_signed_{vname[k]}_version", b.resigned(later, version=versions[k]), 0, 1)
        b.case("V", f"V_att{first - 1}_sig{first}_signed_{vname[k + 1]}_version", b.resigned(earlier, version=versions[k + 1]), 0, 1)
    b.case("V", "V_att39_sig41_capella_header_deneb_version", b.derive(39, 41, extra_len=32), 0, 1)
    v0 = b.derive(0, 1)
    b.case("V", "V_att0_sig1_store0_next_unknown_has_next", v0, 0, 0)
    b.case("V", "V_att0_sig1_store0_next_unknown_signed_altair_version", b.resigned(v0, version=versions[1]), 0, 0)
    b.case("V", "V_att0_sig1_store0_next_known", v0, 0, 1)

    # ---- H: header validity at the Capella and Deneb epochs
    a23, a24, a39, a40 = (pair_rows[k] for k in ((23, 24), (24, 25), (39, 40), (40, 41)))
    b.case("H", "H_att23_empty_execution", a23, 1, 1)
    b.case("H", "H_att23_nonempty_execution", a23, 1, 1, att_exec=poke(a23.attested_header.execution, 0, 7))
    b.case("H", "H_att24_capella_payload_extra0", a24, 1, 1)
    b.case("H", "H_att24_empty_execution", a24, 1, 1, att_exec=bytes(832))
    b.case("H", "H_att24_blob_gas_used_nonzero", a24, 1, 1, att_exec=poke(a24.attested_header.execution, 480, 1))
    b.case("H", "H_att39_capella_root_extra1", a39, 1, 1)
    b.case("H", "H_att39_excess_blob_gas_nonzero", a39, 1, 1, att_exec=poke(a39.attested_header.execution, 512, 1))
    b.case("H", "H_att39_root_of_17_leaves", b.derive(39, 40, deneb=True, blob=False), 1, 1)
    b.case("H", "H_att40_deneb_root_blob_fields_nonzero_extra31", a40, 1, 1)
    assert a40.attested_header.execution[480:488] != bytes(8) and a40.attested_header.execution[512:520] != bytes(8)
    a40z = b.derive(40, 41, blob=False, extra_len=32)
    assert a40z.attested_header.execution[480:488] == bytes(8) and a40z.attested_header.execution[512:520] == bytes(8)
    b.case("H", "H_att40_deneb_root_blob_fields_zero_extra32", a40z, 1, 1)
    b.case("H", "H_att40_root_of_15_leaves", b.derive(40, 41, deneb=False, blob=False), 1, 1)
    f39 = b.derive(41, 42, fin=39)
    b.case("H", "H_fin39_capella_under_att41_deneb", f39, 1, 1)
    b.case("H", "H_fin39_under_att41_execution_corrupted", f39, 1, 1, fin_exec=poke(f39.finalized_header.execution, 100, f39.finalized_header.execution[100] ^ 1))
    b.case("H", "H_fin39_under_att41_blob_gas_used_nonzero", f39, 1, 1, fin_exec=poke(f39.finalized_header.execution, 480, 1))
    f23 = b.derive(25, 26, fin=23)
    b.case("H", "H_fin23_empty_execution_under_att25", f23, 1, 1)
    b.case("H", "H_fin23_under_att25_execution_nonempty", f23, 1, 1, fin_exec=poke(bytes(832), 0, 1))
    f40 = b.derive(42, 43, fin=b.block(40, extra_len=1))
    b.case("H", "H_fin40_deneb_under_att42", f40, 1, 1)
    b.case("H", "H_fin40_under_att42_execution_branch_corrupted", f40, 1, 1, fin_branch=poke(f40.finalized_header.execution_branch, 127, f40.finalized_header.execution_branch[127] ^ 0x80))

    # ---- S: slot ordering (:398)
    s = b.derive(50, 51)
    b.case("S", "S_att50_sig51_current51", s, 0, 1, current=51)
    b.case("S", "S_att50_sig51_current50", s, 0, 1, current=50)
    b.case("S", "S_att50_signature_slot50_current51", s, 0, 1, current=51, signature_slot=50)
    b.case("S", "S_att50_sig51_current_2^63", s, 0, 1, current=T63)
    b.case("S", "S_att50_sig51_current_2^64-1", s, 0, 1, current=2 * T63 - 1)
    b.case("S", "S_fin52_att52_sig53", b.derive(52, 53, fin=52), 0, 1, current=53)
    b.case("S", "S_fin53_att52_sig53", b.derive(52, 53, fin=53), 0, 1, current=53)
    x = b.derive(T63 - 1, T63, signer=1)  # across 2^63, which is a period's first slot: signed by the next committee
    b.case("S", "S_att2^63-1_sig2^63_store2^63-64_current2^63", x, T63 - 64, 1, current=T63)
    b.case("S", "S_att2^63-1_sig2^63_store2^63-64_current2^63-1", x, T63 - 64, 1, current=T63 - 1)
    b.case("S", "S_att2^63-1_sig2^63_store2^63-64_next_unknown", x, T63 - 64, 0, current=T63)
    b.case("S", "S_att2^63-1_sig2^63_store2^63-1", x, T63 - 1, 1, current=T63)
    y = b.derive(T63 + 1, T63 + 2)  # just above 2^63
    b.case("S", "S_att2^63+1_sig2^63+2_store2^63_current2^63+2", y, T63, 1, current=T63 + 2)
    b.case("S", "S_att2^63+1_sig2^63+2_store2^63_current2^63+1", y, T63, 1, current=T63 + 1)
    b.case("S", "S_att2^63+1_sig2^63+2_store2^63+1", y, T63 + 1, 1, current=T63 + 2)
    b.case("S", "S_att2^63+1_sig2^63+2_store2^63-1_signed_by_current", y, T63 - 1, 1, current=2 * T63 - 1)
    b.case("S", "S_att2^63+1_sig2^63+2_store2^63-1_signed_by_next", b.resigned(y, signer=1), T63 - 1, 1, current=2 * T63 - 1)

    # ---- P: periods (:402 / :404), committee selection (:452-459), the :442 equality
    p63 = b.derive(63, 64, signer=1)
    b.case("P", "P_att63_sig64_store62_next_known", p63, 62, 1, current=64)
    b.case("P", "P_att63_sig64_store62_next_unknown", p63, 62, 0, current=64)
    b.case("P", "P_att63_sig64_store63_next_known", p63, 63, 1, current=64)
    b.case("P", "P_att63_sig64_store62_committee_without_branch", p63, 62, 1, pool=1)
    b.case("P", "P_att63_sig64_signed_by_current", b.resigned(p63, signer=0), 62, 1)
    p127 = b.derive(126, 127, signer=1)
    b.case("P", "P_att126_sig127_store62", p127, 62, 1)
    b.case("P", "P_att126_sig127_store64_signed_by_next", p127, 64, 1)
    p128 = b.derive(127, 128, signer=1)
    b.case("P", "P_att127_sig128_store62", p128, 62, 1)
    b.case("P", "P_att127_sig128_store64", p128, 64, 1)
    b.case("P", "P_att127_sig128_store64_next_unknown", p128, 64, 0)
    p62 = b.derive(62, 63)
    b.case("P", "P_att62_sig63_store61", p62, 61, 1)
    b.case("P", "P_att62_sig63_store64_next_known", p62, 64, 1)
    b.case("P", "P_att62_sig63_store64_next_unknown", p62, 64, 0)
    b.case("P", "P_att62_sig63_store63", p62, 63, 1)
    c63 = b.derive(63, 64, signer=1, carry=True)
    b.case("P", "P_att63_sig64_with_committee_branch_store62", c63, 62, 1)
    b.case("P", "P_att63_sig64_with_committee_branch_store62_other_committee", c63, 62, 1, pool=0)
    b.case("P", "P_att63_sig64_with_committee_branch_corrupted", c63, 62, 1, nsc_branch=poke(c63.next_sync_committee_branch, 159, c63.next_sync_committee_branch[159] ^ 1))
    p64 = b.derive(64, 65, signer=1, nsc=0)
    b.case("P", "P_att64_sig65_store62_other_committee", p64, 62, 1)
    b.case("P", "P_att64_sig65_store64", p64, 64, 1)
    p65 = b.derive(65, 66, nsc=0)
    b.case("P", "P_att65_sig66_store64_other_committee_next_known", p65, 64, 1)
    b.case("P", "P_att65_sig66_store64_other_committee_next_unknown", p65, 64, 0)

    # ---- R: relevance (:407-414)
    b.case("R", "R_att50_store49", s, 49, 1)
    b.case("R", "R_att50_store50", s, 50, 1)
    b.case("R", "R_att50_store55", s, 55, 1)
    b.case("R", "R_att50_store50_next_unknown_has_next", s, 50, 0)
    b.case("R", "R_att50_store55_next_unknown_has_next", s, 55, 0)
    b.case("R", "R_att50_store49_next_unknown_no_branch", s, 49, 0, pool=2, nsc_branch=bytes(160))
    b.case("R", "R_att50_store50_next_unknown_no_branch", s, 50, 0, pool=2, nsc_branch=bytes(160))
    b.case("R", "R_att63_sig64_with_branch_store64_next_unknown", c63, 64, 0)
    b.case("R", "R_att63_sig64_with_branch_store65_next_unknown", c63, 65, 0)
    b.case("R", "R_att63_sig64_with_branch_store63_next_unknown", c63, 63, 0)

    # ---- G: finality
    g0 = b.derive(44, 45, fin="genesis")
    assert g0.finalized_header == PR.EMPTY_HEADER and g0.finality_branch != bytes(192)
    b.case("G", "G_genesis_finalized_header", g0, 2, 1)
    b.case("G", "G_genesis_finalized_header_proposer_index_1", g0, 2, 1, fin_beacon=poke(bytes(112), 8, 1))
    b.case("G", "G_genesis_finalized_header_execution_nonempty", g0, 2, 1, fin_exec=poke(bytes(832), 352, 1))
    g30 = b.derive(46, 47, fin=30)
    b.case("G", "G_fin30_att46", g30, 2, 1)
    b.case("G", "G_fin30_att46_default_finalized_header", g30, 2, 1, fin_beacon=bytes(112), fin_exec=bytes(832), fin_branch=bytes(128))
    b.case("G", "G_fin30_att46_no_finality_branch", g30, 2, 1, finality_branch=bytes(192))
    b.case("G", "G_fin30_att46_finality_branch_corrupted", g30, 2, 1, finality_branch=poke(g30.finality_branch, 0, g30.finality_branch[0] ^ 1))
    b.case("G", "G_fin30_att46_finalized_slot_0", g30, 2, 1, fin_beacon=bytes(8) + g30.finalized_header.beacon[8:])

    # ---- N: participation on the validate path (one attested block, one signature block per set)
    order = np.random.default_rng(7).permutation(512).tolist()
    base = b.derive(54, 55, bits=bits_of([0]))
    sets = {"bit0": [0], "bit511": [511], "255": order[:255], "256": order[:256], "257": order[:257],
            "258": order[:258], "511": order[:511], "512": order}
    nrows = {}
    for name, idx in sets.items():
        nrows[name] = b.resigned(base, bits=bits_of(idx))
        b.case("N", f"N_popcount_{name}", nrows[name], 3, 1)
    b.case("N", "N_popcount_0", base, 3, 1, sync_bits=bytes(64))
    b.case("N", "N_popcount_257_with_signature_of_256", nrows["256"], 3, 1, sync_bits=bits_of(sets["257"]))
    b.case("N", "N_popcount_256_with_signature_of_257", nrows["257"], 3, 1, sync_bits=bits_of(sets["256"]))
    b.case("N", "N_popcount_511_with_signature_of_512", nrows["512"], 3, 1, sync_bits=bits_of(sets["511"]))
    b.case("N", "N_bit511_with_signature_of_bit0", nrows["bit0"], 3, 1, sync_bits=bits_of([511]))
    return b


def fixture(b: Builder) -> dict:
    fx = {k: np.stack([np.frombuffer(r[j], np.uint8) for r in b.rows]) for j, k in enumerate(G.COLS)}
    fx["signature_slot"] = np.array(b.sig_slots, np.uint64)
    fx["case_row"] = np.array([c["row"] for c in b.cases], np.uint32)
    fx["case_store_finalized_slot"] = np.array([c["store_fin"] for c in b.cases], np.uint64)
    fx["case_next_known"] = np.array([c["next_known"] for c in b.cases], np.uint8)
    fx["case_current_slot"] = np.array([c["current"] for c in b.cases], np.uint64)
    fx["case_pool_row"] = np.array([c["pool"] for c in b.cases], np.uint32)
    fx["genesis_validators_root"] = np.frombuffer(b.gvr, np.uint8)
    return fx


def main():
    v = H.hostsim_verifier()
    b = build(v)
    fx = fixture(b)
    run = dict(fx, pool=b.pool, cfg=b.cfg, names=[c["name"] for c in b.cases], families=[c["family"] for c in b.cases])
    cur, nxt, zero = (b.pool[k].tobytes() for k in range(3))
    reasons = []
    with S.use_config(**BC.oracle_config(b.cfg)):
        ns, assert_lines = load_reference()
        for i, c in enumerate(b.cases):
            p = BC.batch(run, [i])
            nxt_bytes = nxt if c["next_known"] else zero
            r_oracle = H.O.validate_light_client_update(H.store_from(c["store_fin"], cur, nxt_bytes), H.update_from(p, 0),
                                                        c["current"], b.gvr)
            store_r, u_r = to_reference_objects(ns, p, 0, c["store_fin"], cur, nxt_bytes)
            r_ref = reference_reason(ns, assert_lines, store_r, u_r, c["current"], b.gvr)
            assert r_oracle == r_ref, (c["name"], r_oracle, r_ref)
            reasons.append(r_ref)
            print(f"{i:3d} {c['name']:64s} reason {r_ref}", flush=True)
    run["expected_reason"] = fx["expected_reason"] = np.array(reasons, np.uint8)
    BC.check_coverage(run)
    path = os.path.join(HERE, "lc_boundaries.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    assert size < 256 * 1024, size
    cfgj = {k: (x.hex() if isinstance(x, bytes) else x) for k, x in vars(b.cfg).items()}
    json.dump({"config": cfgj, "cases": [dict(name=c["name"], family=c["family"]) for c in b.cases],
               "expected_reason": reasons, "reference_assert_lines": assert_lines, "notes": NOTES},
              open(os.path.join(HERE, "lc_boundaries.json"), "w"), indent=1)
    valid = sum(1 for r in reasons if r == 0)
    print(f"{len(b.cases)} cases ({valid} valid) over {len(b.rows)} rows, {size} B")


if __name__ == "__main__":
    main()
