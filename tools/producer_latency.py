#!/usr/bin/env python3
"""What deriving a backfill of light-client updates costs on one device (lcv_create_updates_resident,
lcv.producer.create_light_client_updates) against the per-object host path of lcv/producer.py.

Workload: a synthetic chain of --n + 1 consecutive Deneb blocks and their post-states (mainnet configuration, the
slots cross sync-committee period boundaries: 3 committees), one update per block: block k + 1 signs block k, the
finalized block lies --fin-lag blocks back.  Every update derives (reason 0).
  stages   lcv_last_timings' produce_views and produce_rows of synchronous create_updates_resident calls, median of 5
  device   the whole create_updates_resident call on the host clock (view tables in host arrays -> resident batch
           and reasons), --warmup warm-ups, median of --runs; pack_views (view objects -> the tables) apart
  host     create_light_client_update per case + pack_updates + upload over the same views, on fresh view objects
           (no memoised roots), median of --host-runs; rows and reasons must equal the device's
Prints the JSON and writes it to --out.  LCV_BENCH_HOSTSIM=1 runs on the host simulation (a dry run)."""
import argparse
import json
import os
import statistics
import sys
import time
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-client-consensus-specs_amd"))


def build_chain(n, fin_lag, seed, cfg):
    from lcv import producer as PR
    rng = np.random.default_rng(seed)
    spp = cfg.SLOTS_PER_PERIOD
    slot0 = (cfg.DENEB_FORK_EPOCH * cfg.SLOTS_PER_EPOCH // spp + 2) * spp - n // 3  # a boundary a third of the way in
    committees = {}
    states, blocks, roots = [], [], []
    parent = bytes(32)
    for k in range(n + 1):
        slot = slot0 + k
        rec = np.zeros(832, np.uint8)
        rec[:544] = rng.integers(0, 256, 544)
        rec[128:160] = 0
        rec[544:800] = rng.integers(0, 256, 256)
        rec[320 + 7:352] = 0
        rec[800] = 7
        blk = PR.BeaconBlockView(slot=slot, proposer_index=k, parent_root=parent, state_root=bytes(32),
                                 sync_committee_bits=rng.integers(0, 256, 64, dtype=np.uint8).tobytes(),
                                 sync_committee_signature=rng.integers(0, 256, 96, dtype=np.uint8).tobytes(),
                                 execution=rec.tobytes(), execution_deneb=True,
                                 body_roots=rng.integers(0, 256, (12, 32), dtype=np.uint8))
        f = k - fin_lag
        period = slot // spp
        for p in (period, period + 1):
            if p not in committees:
                committees[p] = rng.integers(0, 256, 24624, dtype=np.uint8).tobytes()
        st = PR.BeaconStateView(slot=slot, latest_block_header=blk.header(),
                                finalized_checkpoint_epoch=(slot0 + max(f, 0)) // cfg.SLOTS_PER_EPOCH,
                                finalized_checkpoint_root=roots[f] if f >= 0 else bytes(32),
                                current_sync_committee=committees[period], next_sync_committee=committees[period + 1],
                                field_roots=rng.integers(0, 256, (28, 32), dtype=np.uint8))
        blk = replace(blk, state_root=st.hash_tree_root())
        parent = blk.hash_tree_root()
        states.append(st)
        blocks.append(blk)
        roots.append(parent)
    cases = np.array([[k + 1, k + 1, k, k, k - fin_lag if k >= fin_lag else -1] for k in range(n)], np.int64)
    return states, blocks, cases


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000, help="updates (one per block)")
    ap.add_argument("--fin-lag", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default="producer_latency.json")
    args = ap.parse_args()
    from lcv import producer as PR
    from lcv._native import Lib
    from lcv.device import Verifier
    hostsim = os.environ.get("LCV_BENCH_HOSTSIM") == "1"
    lib = Lib(os.path.join(ROOT, "light-client-consensus-specs_amd", "build", "liblcv_hostsim.so")) if hostsim else None
    v = Verifier(0, lib=lib)
    cfg = v.config
    n = args.n
    t = time.perf_counter()
    states, blocks, cases = build_chain(n, args.fin_lag, 7, cfg)
    build_s = time.perf_counter() - t
    out = {"tool": "tools/producer_latency.py", "library": os.path.basename(v.lib.path), "build": v.lib.build_id(),
           "updates": n, "state_views": len(states), "block_views": len(blocks), "chain_build_s": round(build_s, 2)}

    def med(xs):
        return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
                "runs": [round(x, 3) for x in xs]}

    t = time.perf_counter()
    views = PR.pack_views(states, blocks)
    out["pack_views_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    out["committees"] = views.ncomm

    # ---- device: stage times of synchronous calls, then the whole call on the host clock
    rb, reasons = v.create_updates_resident(views, cases)
    if reasons.any():
        raise SystemExit(f"rows failed to derive: {np.flatnonzero(reasons)[:8].tolist()}")
    dev = v.download(rb)
    rb.free()
    stage = {"produce_views": [], "produce_rows": []}
    for _ in range(5):
        rb, _ = v.create_updates_resident(views, cases)
        tm = v.last_timings()
        rb.free()
        for k in stage:
            stage[k].append(tm[k])
    out["stage_ms"] = {k: med(x) for k, x in stage.items()}
    out["stage_ms"]["sum_of_medians"] = round(sum(out["stage_ms"][k]["median"] for k in stage), 3)
    ms = []
    for k in range(args.warmup + args.runs):
        t = time.perf_counter()
        rb, _ = v.create_updates_resident(views, cases)
        dt = time.perf_counter() - t
        rb.free()
        if k >= args.warmup:
            ms.append(dt * 1e3)
    out["create_updates_resident_ms"] = med(ms)

    # ---- host: the per-object functions over the same views (fresh objects: nothing memoised), pack, upload
    parts = {"create": [], "pack": [], "upload": [], "total": []}
    host = None
    for _ in range(args.host_runs):
        ss, bb = [replace(s) for s in states], [replace(b) for b in blocks]
        t0 = time.perf_counter()
        rows = [PR.create_light_client_update(ss[a], bb[b], ss[c], bb[d], bb[e] if e >= 0 else None, cfg)
                for a, b, c, d, e in cases.tolist()]
        t1 = time.perf_counter()
        host = PR.pack_updates(rows)
        t2 = time.perf_counter()
        hb = v.upload(host)
        t3 = time.perf_counter()
        hb.free()
        for name, dt in (("create", t1 - t0), ("pack", t2 - t1), ("upload", t3 - t2), ("total", t3 - t0)):
            parts[name].append(dt * 1e3)
    out["host_path_ms"] = {k: med(x) for k, x in parts.items()}
    for name in ("att_beacon", "att_exec", "att_branch", "fin_beacon", "fin_exec", "fin_branch", "nsc_branch",
                 "finality_branch", "sync_bits", "sync_signature", "signature_slot"):
        if not np.array_equal(getattr(dev, name), getattr(host, name)):
            raise SystemExit(f"device and host rows differ: {name}")
    for d, h in sorted(set(zip(dev.nsc_index.tolist(), host.nsc_index.tolist()))):  # (the pools are ordered differently)
        if not np.array_equal(dev.nsc_pool[d], host.nsc_pool[h]):
            raise SystemExit("device and host rows differ: next_sync_committee")
    out["rows_equal_host_path"] = True
    out["host_over_device"] = round(out["host_path_ms"]["total"]["median"] / out["create_updates_resident_ms"]["median"], 1)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
