#!/usr/bin/env python3
"""Generate tests/golden/store_fold.npz (run on the build machine only; needs the reference's markdown, which
make_golden.py exec's).  Data only: inputs and what the reference's OWN exec'd functions returned.

    python tests/golden/make_store_fold_golden.py

(a) rank rows — RANK_M update rows made by editing slots, participation bits and branches of one committed row of
    store_sequence.npz (no signatures needed: is_better_update reads none), and the RANK_M x RANK_M matrix
    better[a][b] = is_better_update(row a, row b) of the reference's exec'd function (sync-protocol.md:260-311).
    Asserted here: every one of the eight comparison levels decides at least one pair, at least one pair of
    distinct rows is a full tie, and the participation counts include 341, 342 and 512.
(b) sequence — SEQ, rows of store_sequence.npz's synth.generate batch selected and REPEATED (a repeated row is
    an exact tie of its earlier copy), run through the reference's exec'd process_light_client_update from both
    starting stores (next committee known / unknown), then one process_light_client_store_force_update: accept
    flag, validation reason and store summary per step, as store_sequence.npz holds them.  Asserted here: at
    least 12 valid sub-2/3 rows before the first applying row, two exact ties and three invalid rows among
    them, rows after the first apply, and a second applying row.
"""
from __future__ import annotations

import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import helpers as H  # noqa: E402
import make_golden as MG  # noqa: E402

from lcv import synth  # noqa: E402
from lcv.config import MAINNET  # noqa: E402
from lcv.device import PackedUpdates  # noqa: E402

SPP = MAINNET.SLOTS_PER_PERIOD
RANK_BASE_ROW = 2  # a valid row with finality and next-committee branches
SEQ = [0, 1, 0, 3, 4, 8, 1, 6, 4, 0, 8, 10, 1, 4, 8, 0, 11, 5, 1, 9, 0, 7, 2, 4]


def load_sequence_batch():
    z = np.load(os.path.join(HERE, "store_sequence.npz"))
    p = PackedUpdates(nsc_pool=z["nsc_pool"], nsc_index=z["nsc_index"], signature_slot=z["signature_slot"],
                      **{k: z[k] for k in MG.COLS})
    return z, p


# ----------------------------------------------------------------------------- (a) rank rows
def rank_rows(p: PackedUpdates):
    """(PackedUpdates of the edited rows, their features)."""
    rng = np.random.default_rng(260311)
    b = RANK_BASE_ROW
    period0 = int.from_bytes(p.att_beacon[b][:8].tobytes(), "little") // SPP * SPP
    feats = []
    for n in (1, 340, 341, 342, 512):  # every participation, both sides of the 2/3 bound
        feats.append(dict(n=n, sc=1, fin=1, att=period0 + 301, dsig=1, sig_next=0, fin_prev=0))
    while len(feats) < 46:
        feats.append(dict(n=int(rng.choice([1, 340, 341, 342, 512])), sc=int(rng.integers(0, 2)),
                          fin=int(rng.integers(0, 2)), att=period0 + 300 + int(rng.integers(0, 3)),
                          dsig=int(rng.integers(1, 3)), sig_next=int(rng.integers(0, 4) == 0),
                          fin_prev=int(rng.integers(0, 3) == 0)))
    feats += [dict(feats[7]), dict(feats[20])]  # two exact copies: full ties of distinct rows
    m = len(feats)
    cols = {k: np.repeat(getattr(p, k)[b:b + 1], m, axis=0).copy() for k in MG.COLS}
    sig = np.zeros(m, np.uint64)
    for i, f in enumerate(feats):
        bits = np.zeros(512, np.uint8)
        bits[rng.permutation(512)[:f["n"]]] = 1
        cols["sync_bits"][i] = np.packbits(bits, bitorder="little")
        if not f["sc"]:
            cols["nsc_branch"][i] = 0
        if not f["fin"]:
            cols["finality_branch"][i] = 0
        cols["att_beacon"][i][:8] = np.frombuffer(int(f["att"]).to_bytes(8, "little"), np.uint8)
        fin_slot = period0 - 40 if f["fin_prev"] else period0 + 10
        cols["fin_beacon"][i][:8] = np.frombuffer(int(fin_slot).to_bytes(8, "little"), np.uint8)
        sig[i] = period0 + SPP + 5 if f["sig_next"] else f["att"] + f["dsig"]
    rows = PackedUpdates(nsc_pool=p.nsc_pool, nsc_index=np.repeat(p.nsc_index[b:b + 1], m), signature_slot=sig, **cols)
    return rows, feats


def deciding_level(u, w) -> int:
    """Which comparison of sync-protocol.md:260-311 decides is_better_update(u, w): 1 supermajority, 2 participants
    below it, 3 relevant sync committee, 4 finality, 5 sync-committee finality, 6 participants, 7 attested slot,
    8 signature slot; 0 = a full tie.  (Used only to assert the fixture's coverage.)"""
    period = lambda s: int(s) // SPP  # noqa: E731
    n = lambda x: sum(bool(b) for b in x.sync_aggregate.sync_committee_bits)  # noqa: E731
    zero = lambda br: not any(any(bytes(c)) for c in br)  # noqa: E731
    att = lambda x: int(x.attested_header.beacon.slot)  # noqa: E731
    sup = lambda x: n(x) * 3 >= 512 * 2  # noqa: E731
    if sup(u) != sup(w):
        return 1
    if not sup(u) and n(u) != n(w):
        return 2
    rel = lambda x: (not zero(x.next_sync_committee_branch)) and period(att(x)) == period(x.signature_slot)  # noqa: E731
    if rel(u) != rel(w):
        return 3
    fin = lambda x: not zero(x.finality_branch)  # noqa: E731
    if fin(u) != fin(w):
        return 4
    if fin(u):
        scf = lambda x: period(x.finalized_header.beacon.slot) == period(att(x))  # noqa: E731
        if scf(u) != scf(w):
            return 5
    if n(u) != n(w):
        return 6
    if att(u) != att(w):
        return 7
    if int(u.signature_slot) != int(w.signature_slot):
        return 8
    return 0


def make_rank(ns, z, p):
    rows, feats = rank_rows(p)
    m = rows.n
    cur, nxt = z["current_committee"].tobytes(), z["next_committee"].tobytes()
    us = [MG.to_reference_objects(ns, rows, i, 0, cur, nxt)[1] for i in range(m)]
    better = np.zeros((m, m), np.uint8)
    levels = np.zeros((m, m), np.uint8)
    for a in range(m):
        for b in range(m):
            better[a, b] = 1 if ns["is_better_update"](us[a], us[b]) else 0
            levels[a, b] = deciding_level(us[a], us[b])
    decided = {int(x) for x in np.unique(levels)}
    assert decided >= set(range(1, 9)), f"comparison levels deciding no pair: {set(range(1, 9)) - decided}"
    ties = [(a, b) for a in range(m) for b in range(m) if a != b and levels[a, b] == 0]
    assert ties and all(not better[a, b] and not better[b, a] for a, b in ties), "need a full tie of distinct rows"
    counts = {int(np.unpackbits(rows.sync_bits[i]).sum()) for i in range(m)}
    assert {341, 342, 512} <= counts, counts
    print(f"rank rows: {m}, levels {sorted(decided)}, {len(ties) // 2} tied pairs, participation {sorted(counts)}", flush=True)
    out = {"rank_" + k: getattr(rows, k) for k in MG.COLS}
    out.update(rank_nsc_index=rows.nsc_index, rank_signature_slot=rows.signature_slot, rank_better=better)
    return out


# ----------------------------------------------------------------------------- (b) sequence
def reference_step(ns, assert_lines, store, update, current_slot, gvr):
    """process_light_client_update -> (accepted, reason): the reason is the failing assert of the validation the
    call itself ran (its traceback), 0 when it returned."""
    try:
        ns["process_light_client_update"](store, update, current_slot, gvr)
        return 1, 0
    except AssertionError:
        lines = [f.lineno for f in traceback.extract_tb(sys.exc_info()[2]) if f.filename == "sync-protocol.md"]
        return 0, next(k for k, (a, b) in enumerate(assert_lines) if a <= lines[-1] <= b) + 1


def make_sequence(ns, assert_lines, z, p):
    cur, nxt = z["current_committee"].tobytes(), z["next_committee"].tobytes()
    cs, gvr = int(z["current_slot"]), z["genesis_validators_root"].tobytes()
    fin0 = int(z["store_finalized_slot"])
    out = {"accepted": [], "reason": [], "summary": []}
    for next_known in (1, 0):
        nb = nxt if next_known else bytes(24624)
        store, _ = MG.to_reference_objects(ns, p, 0, fin0, cur, nb)
        acc, rea, summ = [], [], []
        for step, i in enumerate(SEQ):
            _, u = MG.to_reference_objects(ns, p, i, fin0, cur, nb)
            a, r = reference_step(ns, assert_lines, store, u, cs, gvr)
            acc.append(a)
            rea.append(r)
            summ.append(MG.store_summary(store))
            print(f"next_known={next_known} step {step:2d} row {i:2d} reason {r} store {summ[-1]}", flush=True)
        force = int(store.finalized_header.beacon.slot) + ns["UPDATE_TIMEOUT"] + 1
        ns["process_light_client_store_force_update"](store, force)
        summ.append(MG.store_summary(store))
        # the shape the fold tests rely on
        moved = [k for k in range(len(SEQ)) if acc[k] and summ[k][2] == -1]  # an accepted row leaving no best: applied
        assert len(moved) >= 2 and moved[0] < len(SEQ) - 1, moved
        head = range(moved[0])
        low_valid = [k for k in head if acc[k] and int(z["kinds"][SEQ[k]]) == synth.K_LOW_PARTICIPATION]
        assert len(low_valid) >= 12, low_valid
        assert sum(1 for k in low_valid if SEQ[k] in [SEQ[j] for j in low_valid if j < k]) >= 2, "two exact ties"
        assert sum(1 for k in head if not acc[k]) >= 3, "three invalid rows before the first apply"
        out["accepted"].append(acc)
        out["reason"].append(rea)
        out["summary"].append(summ)
    return {"seq": np.array(SEQ, np.uint32), "seq_accepted": np.array(out["accepted"], np.uint8),
            "seq_reason": np.array(out["reason"], np.uint8), "seq_summary": np.array(out["summary"], np.int64)}


def main():
    ns, assert_lines = MG.load_reference()
    z, p = load_sequence_batch()
    out = make_rank(ns, z, p)
    out.update(make_sequence(ns, assert_lines, z, p))
    np.savez_compressed(os.path.join(HERE, "store_fold.npz"), **out)


if __name__ == "__main__":
    main()
