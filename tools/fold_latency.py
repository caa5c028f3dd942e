#!/usr/bin/env python3
"""Latency of lcv.store.fold_light_client_updates against process_light_client_updates, and what the fold costs
the serving rate, on one device.

Rows: --distinct synthetic updates of lcv.synth, all K_LOW_PARTICIPATION (valid, below 2/3: none applies, so the
whole batch is ONE segment and the fold walks every row), tiled to --n.
  latency   the whole call on the host clock from a fresh store, --warmup warm-ups, median of --runs:
            fold_light_client_updates (PackedUpdates in) and, with --process-runs > 0, process_light_client_updates
            on the same rows as update objects (built outside the timed region); the two final stores must agree
  kernels   lcv_last_timings of one synchronous validate_fold: store_rank, store_fold and the whole pipeline
  serving   --depth batches in flight, --steps batches per pass: validate_async against validate_async_fold,
            alternated --serving-rounds times, and in each round a second plain pass — the spread of the box
Prints the JSON and writes it to --out.  LCV_BENCH_HOSTSIM=1 runs on the host simulation (a dry run)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

# a hardware queue per stream of the eight work-space slots, as bench.py sets it (before the HIP runtime loads)
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-client-consensus-specs_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000, help="rows per batch")
    ap.add_argument("--distinct", type=int, default=200, help="distinct rows generated (tiled to --n)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--process-runs", type=int, default=3, help="timed runs of process_light_client_updates (0 = skip)")
    ap.add_argument("--depth", type=int, default=8, help="batches in flight (serving)")
    ap.add_argument("--steps", type=int, default=40, help="batches per serving pass")
    ap.add_argument("--serving-rounds", type=int, default=3)
    ap.add_argument("--out", default="fold_latency.json")
    args = ap.parse_args()
    from lcv import layout as L
    from lcv import store as LS
    from lcv import synth
    from lcv._native import Lib
    from lcv.device import FoldState, Verifier
    hostsim = os.environ.get("LCV_BENCH_HOSTSIM") == "1"
    lib = Lib(os.path.join(ROOT, "light-client-consensus-specs_amd", "build", "liblcv_hostsim.so")) if hostsim else None
    v = Verifier(0, lib=lib)
    n, D = args.n, args.depth
    kinds = np.full(args.distinct, synth.K_LOW_PARTICIPATION)
    base = synth.generate(v, args.distinct, seed=41, participation="random", kinds=kinds)
    sb = synth.tile(base, -(-n // args.distinct))
    p = sb.updates.slice(0, n)
    cs, gvr = sb.current_slot, sb.genesis_validators_root

    def fresh_store():
        fin = LS._default_header()
        fin.beacon.slot = sb.store_finalized_slot
        return LS.LightClientStore(finalized_header=fin, current_sync_committee=L.unpack_sync_committee(sb.current.ssz),
                                   next_sync_committee=L.unpack_sync_committee(sb.next.ssz), best_valid_update=None,
                                   optimistic_header=LS._default_header(), previous_max_active_participants=0,
                                   current_max_active_participants=0)

    def summary(st):
        b = st.best_valid_update
        return [int(st.finalized_header.beacon.slot), int(st.optimistic_header.beacon.slot),
                -1 if b is None else int(b.signature_slot), int(st.previous_max_active_participants),
                int(st.current_max_active_participants)]

    def timed(fn, rows, warmup, runs):
        ms, last = [], None
        for k in range(warmup + runs):
            st = fresh_store()
            stats = {}
            t = time.perf_counter()
            acc = fn(st, rows, cs, gvr, v, None, stats) if fn is LS.fold_light_client_updates else fn(st, rows, cs, gvr, v)
            dt = time.perf_counter() - t
            if not acc.all():
                raise SystemExit("a valid update was rejected")
            if k >= warmup:
                ms.append(dt * 1e3)
            last = (summary(st), stats)
        return ms, last

    out = {"tool": "tools/fold_latency.py", "library": os.path.basename(v.lib.path), "build": v.lib.build_id(),
           "rows": n, "distinct_rows": args.distinct, "GPU_MAX_HW_QUEUES": os.environ["GPU_MAX_HW_QUEUES"]}
    fold_ms, (fold_store, fold_stats) = timed(LS.fold_light_client_updates, p, args.warmup, args.runs)
    out["fold_light_client_updates_ms"] = {"median": round(statistics.median(fold_ms), 3), "runs": [round(x, 3) for x in fold_ms],
                                           "stats": fold_stats}
    if args.process_runs > 0:
        ups = [L.unpack_update(p, i) for i in range(n)]
        proc_ms, (proc_store, _) = timed(LS.process_light_client_updates, ups, 1, args.process_runs)
        if proc_store != fold_store:
            raise SystemExit(f"final stores differ: fold {fold_store}, process {proc_store}")
        out["process_light_client_updates_ms"] = {"median": round(statistics.median(proc_ms), 3),
                                                  "runs": [round(x, 3) for x in proc_ms]}
        out["speedup"] = round(statistics.median(proc_ms) / statistics.median(fold_ms), 1)

    # kernel times of one synchronous folded call (serial stages)
    v.set_store(sb.store_finalized_slot, sb.current.ssz, sb.next.ssz)
    runs = []
    for _ in range(5):
        v.validate_fold(p, cs, gvr, FoldState())
        runs.append(v.last_timings())
    out["validate_fold_stage_ms"] = {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0] if any(r[k] for r in runs)}

    # serving: D batches in flight, plain against folded, alternating; a second plain pass gives the box's spread
    def plain(steps):
        for k in range(steps):
            s = k % D
            if k >= D:
                v.slot_wait(s, n)
            v.validate_async(p, cs, gvr, s)
        for k in range(max(0, steps - D), steps):
            v.slot_wait(k % D, n)

    def folded(steps):
        st = FoldState()
        for k in range(steps):
            s = k % D
            if k >= D:
                v.slot_wait_fold(s, n)
            v.validate_async_fold(p, cs, gvr, st, s)
        for k in range(max(0, steps - D), steps):
            v.slot_wait_fold(k % D, n)

    rates = {"plain": [], "plain_again": [], "fold": []}
    for rnd in range(args.serving_rounds + 1):  # round 0 warms up and is not counted
        for name, fn in (("plain", plain), ("fold", folded), ("plain_again", plain)):
            t = time.perf_counter()
            fn(args.steps)
            dt = time.perf_counter() - t
            if rnd:
                rates[name].append(n * args.steps / dt)
    med = {k: statistics.median(x) for k, x in rates.items()}
    out["serving"] = {"batches_in_flight": D, "steps": args.steps,
                      "updates_per_s_runs": {k: [round(x, 1) for x in xs] for k, xs in rates.items()},
                      "updates_per_s_median": {k: round(x, 1) for k, x in med.items()},
                      "fold_over_plain": round(med["fold"] / med["plain"], 4),
                      "plain_again_over_plain": round(med["plain_again"] / med["plain"], 4)}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
