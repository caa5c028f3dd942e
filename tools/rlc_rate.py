#!/usr/bin/env python3
"""Serving rate with and without randomised batch verification (Verifier.set_rlc), on one device.

The loop is bench.py --full's host-buffer leg: host batches of --n rows, --depth in flight, each handed to
lcv_validate_async on its work-space slot (staging, one DMA, every kernel, verdicts back to pinned memory) and collected
with lcv_slot_wait.  Rows come from lcv.synth (valid, full participation, finality and next committee), --n distinct
updates generated once; for every share of --bad a fixed random set of rows gets another row's signature (a G2 point
that is no signature of the row: reason 14), and every batch is a different permutation of those rows.

Per share and per group size G of --groups: rows/s with the mode off and on (median and min-max of --runs runs of
--steps batches, the two modes alternating inside each run), their ratio, lcv_last_rlc of the last batch, and the
per-stage kernel times of one synchronous batch with the mode off and on (lcv_last_timings, median of 3 calls): rlc_scale,
rlc_product, the shrunken final_exp, rlc_spread, rlc_retry.  Every verdict is checked against the rows' construction.

--package DIR runs the same loop on another build of the package (its lcv/ and liblcv.so), e.g. the parent commit's: a
package without set_rlc is measured with the mode off only.
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
STAGES = ("sig_decode", "g1_aggregate", "rlc_scale", "miller_lines", "miller_lines_sig", "miller_loop", "rlc_product",
          "final_exp", "rlc_spread", "rlc_retry", "verdict")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000, help="rows per batch")
    ap.add_argument("--groups", default="4,8,16,32", help="group sizes G, comma separated")
    ap.add_argument("--bad", default="0,0.01,1", help="shares of rows with a wrong signature, comma separated")
    ap.add_argument("--depth", type=int, default=8, help="batches in flight")
    ap.add_argument("--steps", type=int, default=40, help="batches per timed run")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--package", default=os.path.join(ROOT, "light-client-consensus-specs_amd"),
                    help="directory that holds the lcv package to measure")
    ap.add_argument("--out", default="rlc_rate.json")
    args = ap.parse_args()
    pkg = os.path.abspath(args.package)
    sys.path.insert(0, pkg)
    from lcv import synth
    from lcv._native import Lib
    from lcv.device import PackedUpdates, Verifier
    hostsim = os.environ.get("LCV_BENCH_HOSTSIM") == "1"
    v = Verifier(0, lib=Lib(os.path.join(pkg, "build", "liblcv_hostsim.so")) if hostsim else None)
    has_mode = hasattr(v, "set_rlc")
    n, D = args.n, args.depth
    t0 = time.perf_counter()
    sb = synth.generate(v, n, seed=2)
    print(f"generated {n} distinct rows in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    u, gvr, cs = sb.updates, sb.genesis_validators_root, sb.current_slot
    v.set_store(sb.store_finalized_slot, sb.current.ssz, sb.next.ssz)
    v.set_latency_mode(0)  # the batch engine whatever --n is

    def take(rows, sig):
        kw = {k: np.ascontiguousarray(getattr(u, k)[rows]) for k in COLS}
        kw["sync_signature"] = np.ascontiguousarray(sig[rows])
        return PackedUpdates(nsc_pool=u.nsc_pool, nsc_index=u.nsc_index[rows].copy(),
                             signature_slot=u.signature_slot[rows].copy(), **kw)

    out_v = [np.zeros(n, np.uint8) for _ in range(D)]
    out_r = [np.zeros(n, np.uint8) for _ in range(D)]

    def serve(batches, steps):
        ok = True
        for k in range(steps):
            s = k % D
            if k >= D:
                v.slot_wait(s, n, out_v[s], out_r[s])
                ok &= bool(np.array_equal(out_v[s], batches[s][1]))
            v.validate_async(batches[s][0], cs, gvr, s)
        for k in range(max(0, steps - D), steps):
            v.slot_wait(k % D, n, out_v[k % D], out_r[k % D])
            ok &= bool(np.array_equal(out_v[k % D], batches[k % D][1]))
        return ok

    def stage_times(batch):
        runs = []
        for _ in range(3):
            ok, _ = v.validate(batch[0], cs, gvr)
            assert np.array_equal(np.asarray(ok, np.uint8), batch[1])
            runs.append(v.last_timings())
        return {k: round(statistics.median(r.get(k, 0.0) for r in runs), 4) for k in STAGES if any(r.get(k, 0.0) for r in runs)}

    rng = np.random.default_rng(7)
    results = {}
    for tok in args.bad.split(","):
        share = float(tok)
        nbad = int(round(share * n))
        bad = np.zeros(n, bool)
        bad[rng.choice(n, nbad, replace=False)] = True
        sig = np.array(u.sync_signature, copy=True)
        sig[bad] = u.sync_signature[(np.flatnonzero(bad) + 1) % n]  # the next row's signature: a G2 point, not this row's
        batches = []
        for _ in range(D):
            rows = rng.permutation(n)
            batches.append((take(rows, sig), (~bad[rows]).astype(np.uint8)))
        per_group = {}
        for G in [int(g) for g in args.groups.split(",")] if has_mode else [0]:
            rates = {"off": [], "on": []}
            last = None
            for run in range(args.runs + 1):  # run 0 warms up (work spaces, staging buffers, scratch) and is not counted
                for mode in ("off", "on") if has_mode else ("off",):
                    if has_mode:
                        v.set_rlc(G if mode == "on" else 0)
                    t = time.perf_counter()
                    ok = serve(batches, args.steps)
                    dt = time.perf_counter() - t
                    if not ok:
                        raise SystemExit(f"bad share {share}, G = {G}, mode {mode}: a verdict differs from the rows' construction")
                    if run:
                        rates[mode].append(n * args.steps / dt)
                    if mode == "on":
                        last = v.last_rlc((args.steps - 1) % D)
            stages = {}
            for mode in ("off", "on") if has_mode else ("off",):
                if has_mode:
                    v.set_rlc(G if mode == "on" else 0)
                stages[mode] = stage_times(batches[0])
            if has_mode:
                v.set_rlc(0)
            med = {m: round(statistics.median(x), 1) for m, x in rates.items() if x}
            per_group[str(G)] = {"rows_per_s_median": med,
                                 "rows_per_s_min_max": {m: [round(min(x), 1), round(max(x), 1)] for m, x in rates.items() if x},
                                 "rows_per_s_runs": {m: [round(y, 1) for y in x] for m, x in rates.items() if x},
                                 "on_over_off": round(med["on"] / med["off"], 4) if "on" in med else None,
                                 "last_rlc_groups_retried": list(last) if last else None,
                                 "stage_ms_one_batch": stages}
            print(f"bad {share} G {G}: {med} last_rlc {last}", file=sys.stderr)
        results[tok.strip()] = {"bad_rows_per_batch": nbad, "by_group": per_group}
    out = {"tool": "tools/rlc_rate.py", "package": os.path.relpath(pkg, ROOT), "library": os.path.basename(v.lib.path),
           "build": v.lib.build_id(), "rows_per_batch": n, "batches_in_flight": D, "steps": args.steps, "runs": args.runs,
           "GPU_MAX_HW_QUEUES": os.environ["GPU_MAX_HW_QUEUES"], "by_bad_share": results}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
