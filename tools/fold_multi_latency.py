#!/usr/bin/env python3
"""What folding a store-table batch per store costs on one device (lcv_validate_stores_fold,
lcv.store.fold_light_client_updates_multi), beside the one-store fold tools/fold_latency.py measures.

Rows: --distinct synthetic updates of lcv.synth, all K_LOW_PARTICIPATION (valid, below 2/3: none applies, so every
row of every store is walked), tiled to --n.  The stores of a shape share one validation key (the same finalized
slot and committees): S store rows of the table, row i of the batch for store i % S.
  stages    lcv_last_timings' store_fold (and store_rank, the whole pipeline) of synchronous calls, median of 5:
            validate_stores_fold for each --shapes entry (stores per batch) against the one-store validate_fold on
            the same rows
  latency   the whole call on the host clock from fresh stores, --warmup warm-ups, median of --runs, for
            --latency-stores stores: fold_light_client_updates_multi; fold_light_client_updates once per store;
            with --process-runs > 0, process_light_client_updates once per store (update objects built outside the
            timed region); the final stores must agree
  serving   --depth table batches in flight from host buffers, --steps batches per pass: validate_stores_async,
            validate_stores_async_fold, validate_stores_async again (the spread of the box), --serving-rounds times
            after a warm-up round; and the host time of the enqueueing call alone, plain against folded (the
            grouping runs inside it).  Once per --serving-stores entry: the first is the headline; one store (the
            longest fold, rows already grouped) and many stores (short folds, a sort) tell the kernel's share of a
            difference from the grouping's
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
    ap.add_argument("--shapes", default="1,16,10000", help="stores per batch of the stage timings")
    ap.add_argument("--latency-stores", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--process-runs", type=int, default=3, help="timed runs of process_light_client_updates (0 = skip)")
    ap.add_argument("--depth", type=int, default=8, help="batches in flight (serving)")
    ap.add_argument("--steps", type=int, default=40, help="batches per serving pass")
    ap.add_argument("--serving-rounds", type=int, default=3)
    ap.add_argument("--serving-stores", default="16,1,256",
                    help="stores per batch of the serving passes: the first is the headline, the others tell the kernel's "
                         "share of a difference (one store: the longest fold, no sort) from the grouping's (many: a sort)")
    ap.add_argument("--out", default="fold_multi_latency.json")
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
    committees = np.stack([np.frombuffer(sb.current.ssz, np.uint8), np.frombuffer(sb.next.ssz, np.uint8)])

    def set_table(nstore):
        v.set_store_table(committees, [sb.store_finalized_slot] * nstore, [0] * nstore, [1] * nstore)

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

    out = {"tool": "tools/fold_multi_latency.py", "library": os.path.basename(v.lib.path), "build": v.lib.build_id(),
           "rows": n, "distinct_rows": args.distinct, "GPU_MAX_HW_QUEUES": os.environ["GPU_MAX_HW_QUEUES"]}

    # ---- stage times of synchronous calls (serial stages): the one-store fold, then each shape of the table fold
    def stages(call):
        runs = []
        for _ in range(5):
            call()
            runs.append(v.last_timings())
        return {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0] if any(r[k] for r in runs)}

    v.set_store(sb.store_finalized_slot, sb.current.ssz, sb.next.ssz)
    v.validate_fold(p, cs, gvr, FoldState())
    out["validate_fold_stage_ms"] = stages(lambda: v.validate_fold(p, cs, gvr, FoldState()))
    out["validate_stores_fold_stage_ms"] = {}
    for S in (int(x) for x in args.shapes.split(",")):
        S = min(S, n)
        set_table(S)
        six = (np.arange(n) % S).astype(np.uint32)
        states = [FoldState() for _ in range(S)]
        _, _, res = v.validate_stores_fold(p, six, cs, gvr, states)
        if sum(r.rows_consumed for r in res) != n or any(r.apply_row >= 0 for r in res):
            raise SystemExit("the table fold did not walk every row")
        out["validate_stores_fold_stage_ms"][f"{S}x{n // S}"] = stages(lambda: v.validate_stores_fold(p, six, cs, gvr, states))

    # ---- the whole call on the host clock
    S = args.latency_stores
    owner_ix = np.arange(n) % S
    per_store = [LS._take_rows(p, np.flatnonzero(owner_ix == s)) for s in range(S)]

    def run_multi(_):
        st = [fresh_store() for _ in range(S)]
        stats = {}
        t = time.perf_counter()
        acc = LS.fold_light_client_updates_multi([st[k] for k in owner_ix], p, cs, gvr, v, None, stats)
        return time.perf_counter() - t, acc.all(), [summary(x) for x in st], stats

    def run_loop(fn, rows):
        def go(_):
            st = [fresh_store() for _ in range(S)]
            t = time.perf_counter()
            ok = all(fn(st[s], rows[s], cs, gvr, v).all() for s in range(S))
            return time.perf_counter() - t, ok, [summary(x) for x in st], {}
        return go

    def timed(go, warmup, runs):
        ms, last = [], None
        for k in range(warmup + runs):
            dt, ok, stores, stats = go(k)
            if not ok:
                raise SystemExit("a valid update was rejected")
            if k >= warmup:
                ms.append(dt * 1e3)
            last = (stores, stats)
        return {"median": round(statistics.median(ms), 3), "runs": [round(x, 3) for x in ms]}, last

    lat = {"stores": S, "rows_per_store": n // S}
    lat["fold_light_client_updates_multi_ms"], (multi_stores, multi_stats) = timed(run_multi, args.warmup, args.runs)
    lat["fold_light_client_updates_multi_ms"]["stats"] = multi_stats
    lat["fold_light_client_updates_per_store_ms"], (loop_stores, _) = timed(run_loop(LS.fold_light_client_updates, per_store),
                                                                          args.warmup, args.runs)
    if loop_stores != multi_stores:
        raise SystemExit("final stores differ: multi against the per-store fold")
    lat["per_store_fold_over_multi"] = round(lat["fold_light_client_updates_per_store_ms"]["median"] /
                                             lat["fold_light_client_updates_multi_ms"]["median"], 2)
    if args.process_runs > 0:
        objects = [[L.unpack_update(b, i) for i in range(b.n)] for b in per_store]
        lat["process_light_client_updates_per_store_ms"], (proc_stores, _) = timed(
            run_loop(LS.process_light_client_updates, objects), 1, args.process_runs)
        if proc_stores != multi_stores:
            raise SystemExit("final stores differ: multi against process_light_client_updates")
        lat["process_over_multi"] = round(lat["process_light_client_updates_per_store_ms"]["median"] /
                                          lat["fold_light_client_updates_multi_ms"]["median"], 1)
    out["latency"] = lat

    # ---- serving: D table batches in flight, plain against folded, alternating; a second plain pass = the box's spread
    def serving(S):
        set_table(S)
        six = (np.arange(n) % S).astype(np.uint32)
        states = [FoldState() for _ in range(S)]
        enqueue = {"plain": [], "fold": []}
        counted = [False]

        def plain(steps):
            for k in range(steps):
                s = k % D
                if k >= D:
                    v.slot_wait(s, n)
                t = time.perf_counter()
                v.validate_stores_async(p, six, cs, gvr, s)
                if counted[0]:
                    enqueue["plain"].append(time.perf_counter() - t)
            for k in range(max(0, steps - D), steps):
                v.slot_wait(k % D, n)

        def folded(steps):
            for k in range(steps):
                s = k % D
                if k >= D:
                    v.slot_wait_stores_fold(s, n, S)
                t = time.perf_counter()
                v.validate_stores_async_fold(p, six, cs, gvr, states, s)
                if counted[0]:
                    enqueue["fold"].append(time.perf_counter() - t)
            for k in range(max(0, steps - D), steps):
                v.slot_wait_stores_fold(k % D, n, S)

        rates = {"plain": [], "plain_again": [], "fold": []}
        for rnd in range(args.serving_rounds + 1):  # round 0 warms up and is not counted
            for name, fn in (("plain", plain), ("fold", folded), ("plain_again", plain)):
                counted[0] = rnd > 0
                t = time.perf_counter()
                fn(args.steps)
                dt = time.perf_counter() - t
                if rnd:
                    rates[name].append(n * args.steps / dt)
        med = {k: statistics.median(x) for k, x in rates.items()}
        lo, hi = min(rates["plain"] + rates["plain_again"]), max(rates["plain"] + rates["plain_again"])
        return {"batches_in_flight": D, "steps": args.steps, "stores": S,
                "updates_per_s_runs": {k: [round(x, 1) for x in xs] for k, xs in rates.items()},
                "updates_per_s_median": {k: round(x, 1) for k, x in med.items()},
                "plain_spread": [round(lo, 1), round(hi, 1)],
                "fold_median_within_plain_spread": bool(lo <= med["fold"] <= hi),
                "fold_over_plain": round(med["fold"] / med["plain"], 4),
                "plain_again_over_plain": round(med["plain_again"] / med["plain"], 4),
                "enqueue_call_ms_median": {k: round(statistics.median(x) * 1e3, 3) for k, x in enqueue.items() if x}}

    shapes = [int(x) for x in args.serving_stores.split(",")]
    out["serving"] = serving(shapes[0])
    out["serving_other_shapes"] = {str(S): serving(S) for S in shapes[1:]}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
