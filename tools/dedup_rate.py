#!/usr/bin/env python3
"""Serving rate of table batches with and without deduplicated signatures (Verifier.set_dedup), on one device.

The loop is bench.py --full's host-buffer leg: host batches of --n rows, --depth in flight, each handed to
lcv_validate_stores_async on its work-space slot (staging, one DMA, every kernel, verdicts back to pinned memory)
and collected with lcv_slot_wait.  Rows come from lcv.synth (valid, full participation, finality and next
committee): --n distinct updates are generated once, and for every repeat factor d of --repeats a batch holds the
first n / d of them d times each (d = n: one update n times), permuted differently per batch, every row pointing at
one of --stores store rows that hold the same committees — one update relayed to many light clients.

Per d: rows/s with the mode off and on (median of --runs runs of --steps batches, the two modes alternating
inside each run), their ratio, and lcv_last_dedup of the last batch.  d = 1 with the mode on is the cost of the mode
where nothing repeats (host hashing, the gather, the BLS side waiting for the pre-checks).

--package DIR runs the same loop on another build of the package (its lcv/ and liblcv.so), e.g. the parent commit's:
the off leg needs no symbol of this mode, and a package without set_dedup is measured with the mode off only.
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
COLS = ("att_beacon", "att_exec", "att_branch", "fin_beacon", "fin_exec", "fin_branch", "nsc_branch",
        "finality_branch", "sync_bits", "sync_signature")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000, help="rows per batch")
    ap.add_argument("--repeats", default="1,8,64,n", help="repeat factors d, comma separated; n = one update per batch")
    ap.add_argument("--stores", type=int, default=16, help="store rows of the table (all hold the same committees)")
    ap.add_argument("--depth", type=int, default=8, help="batches in flight")
    ap.add_argument("--steps", type=int, default=40, help="batches per timed run")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--package", default=os.path.join(ROOT, "light-client-consensus-specs_amd"),
                    help="directory that holds the lcv package to measure")
    ap.add_argument("--out", default="dedup_rate.json")
    args = ap.parse_args()
    pkg = os.path.abspath(args.package)
    sys.path.insert(0, pkg)
    from lcv import synth
    from lcv._native import Lib
    from lcv.device import PackedUpdates, Verifier
    hostsim = os.environ.get("LCV_BENCH_HOSTSIM") == "1"
    v = Verifier(0, lib=Lib(os.path.join(pkg, "build", "liblcv_hostsim.so")) if hostsim else None)
    has_mode = hasattr(v, "set_dedup")
    n, D, K = args.n, args.depth, args.stores
    t0 = time.perf_counter()
    sb = synth.generate(v, n, seed=2)
    print(f"generated {n} distinct rows in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    u, gvr, cs = sb.updates, sb.genesis_validators_root, sb.current_slot
    v.set_store_table(np.frombuffer(sb.current.ssz + sb.next.ssz, np.uint8).reshape(2, -1), [sb.store_finalized_slot] * K,
                      [0] * K, [1] * K)

    def take(rows):
        return PackedUpdates(nsc_pool=u.nsc_pool, nsc_index=u.nsc_index[rows].copy(), signature_slot=u.signature_slot[rows].copy(),
                             **{k: np.ascontiguousarray(getattr(u, k)[rows]) for k in COLS})

    out_v = [np.zeros(n, np.uint8) for _ in range(D)]
    out_r = [np.zeros(n, np.uint8) for _ in range(D)]

    def serve(batches, steps):
        ok = True
        for k in range(steps):
            s = k % D
            if k >= D:
                v.slot_wait(s, n, out_v[s], out_r[s])
                ok &= bool(out_v[s].all())
            v.validate_stores_async(batches[s][0], batches[s][1], cs, gvr, s)
        for k in range(max(0, steps - D), steps):
            v.slot_wait(k % D, n, out_v[k % D], out_r[k % D])
            ok &= bool(out_v[k % D].all())
        return ok

    rng = np.random.default_rng(7)
    results = {}
    for tok in args.repeats.split(","):
        d = n if tok.strip() == "n" else int(tok)
        distinct = max(1, n // d)
        batches = [(take(rng.permutation(np.arange(n) % distinct)), rng.integers(0, K, n).astype(np.uint32)) for _ in range(D)]
        rates = {"off": [], "on": []}
        last = None
        for run in range(args.runs + 1):  # run 0 warms up (work spaces, staging buffers, scratch) and is not counted
            for mode in ("off", "on") if has_mode else ("off",):
                if has_mode:
                    v.set_dedup(mode == "on")
                t = time.perf_counter()
                ok = serve(batches, args.steps)
                dt = time.perf_counter() - t
                if not ok:
                    raise SystemExit(f"d = {d}, mode {mode}: a valid update was rejected")
                if run:
                    rates[mode].append(n * args.steps / dt)
                if mode == "on":
                    last = v.last_dedup((args.steps - 1) % D)
        if has_mode:
            v.set_dedup(False)
        med = {m: round(statistics.median(x), 1) for m, x in rates.items() if x}
        results[str(d)] = {"distinct_updates_per_batch": distinct, "rows_per_s_median": med,
                           "rows_per_s_runs": {m: [round(y, 1) for y in x] for m, x in rates.items() if x},
                           "on_over_off": round(med["on"] / med["off"], 4) if "on" in med else None,
                           "last_dedup_rows_items": list(last) if last else None}
        print(f"d = {d}: {results[str(d)]['rows_per_s_median']} last_dedup {last}", file=sys.stderr)
    out = {"tool": "tools/dedup_rate.py", "package": os.path.relpath(pkg, ROOT), "library": os.path.basename(v.lib.path), "build": v.lib.build_id(),
           "rows_per_batch": n, "stores": K, "batches_in_flight": D, "steps": args.steps, "runs": args.runs,
           "GPU_MAX_HW_QUEUES": os.environ["GPU_MAX_HW_QUEUES"], "by_repeat_factor": results}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
