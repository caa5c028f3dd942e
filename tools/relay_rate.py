#!/usr/bin/env python3
"""What the relay's device path costs on one device: wire messages decoded, classed and fanned out to the stores of
many clients where they lie (lcv.serving.relay_updates: lcv_batch_decode, lcv_batch_classify, lcv_batch_fan_out,
lcv_validate_resident under lcv_set_dedup) against the same path without deduplication and against the host route.

Workload: --messages distinct valid finality updates (lcv.synth, encoded once by lcv_batch_encode, handed over as one
buffer with offsets and lengths), each relayed to --stores store rows that hold the same committees: pair i is
(message i // stores, store i % stores).  The default shapes are 1,250 x 8 and 1 x 10,000 (--shapes).  Per shape:
  classify      the classify call on the decoded batch (messages rows) and on the fanned-out batch (pairs rows, fanned
                out unclassed), on the host clock, with lcv_last_classify_timings' two marks (keys, compares)
  relay_on      relay_updates(dedup=True), whole call on the host clock
  relay_off     relay_updates(dedup=False)
  host_route    lcv.wire.decode_updates on the host + the rows tiled on the host + Verifier.upload(rows, store_index)
                under set_dedup(True) + validate_resident
  relay_stream  lcv.serving.relay_stream(dedup=True) over --in-flight copies of the shape with as many in flight
                (lcv_relay_async on the slots): the whole loop on the host clock, divided by the copies, so the figure is
                the time per item of a full pipeline; relay_kernel_ms is lcv_last_relay_timings of the last item,
                relay_async_call_ms the host time of one relay_async call (staging, grouping, enqueue) with the slots
                busy, stage_ms_sync lcv_last_timings of one synchronous relay_updates(dedup=True) (the validation's
                kernels, for the split)
The routes must give the same verdicts and reasons.  --warmup warm-ups, median of --runs with min and max, the
routes alternating inside each run.  Prints the JSON and writes it to --out.  LCV_BENCH_HOSTSIM=1 runs on the host
simulation (a dry run)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

# the stream route keeps eight slots (sixteen streams) in flight: a hardware queue per stream, as the other serving tools ask
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-client-consensus-specs_amd"))

COLS = ("att_beacon", "att_exec", "att_branch", "fin_beacon", "fin_exec", "fin_branch", "nsc_branch",
        "finality_branch", "sync_bits", "sync_signature")


def med(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "runs": [round(x, 3) for x in xs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="1250x8,1x10000", help="messages x stores, comma separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--in-flight", type=int, default=8, help="items in flight (and per run) of relay_stream")
    ap.add_argument("--out", default="relay_rate.json")
    args = ap.parse_args()
    from lcv import synth, wire
    from lcv._native import Lib
    from lcv.device import PackedUpdates, Verifier
    from lcv.serving import relay_stream, relay_updates
    hostsim = os.environ.get("LCV_BENCH_HOSTSIM") == "1"
    lib = Lib(os.path.join(ROOT, "light-client-consensus-specs_amd", "build", "liblcv_hostsim.so")) if hostsim else None
    v = Verifier(0, lib=lib)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    sb = synth.generate(v, max(m for m, _ in shapes), seed=2)
    gvr, cs = sb.genesis_validators_root, sb.current_slot
    committees = np.frombuffer(sb.current.ssz + sb.next.ssz, np.uint8).reshape(2, -1)
    out = {"tool": "tools/relay_rate.py", "library": os.path.basename(v.lib.path), "build": v.lib.build_id(),
           "kind": "finality", "fork": "deneb", "warmup": args.warmup, "runs": args.runs, "in_flight": args.in_flight,
           "GPU_MAX_HW_QUEUES": os.environ["GPU_MAX_HW_QUEUES"],
           "shapes": {}}

    def take(p, rows):
        return PackedUpdates(nsc_pool=p.nsc_pool, nsc_index=p.nsc_index[rows].copy(), signature_slot=p.signature_slot[rows].copy(),
                             **{k: np.ascontiguousarray(getattr(p, k)[rows]) for k in COLS})

    for m, k in shapes:
        n = m * k
        v.set_store_table(committees, [sb.store_finalized_slot] * k, [0] * k, [1] * k)
        enc = v.encode(sb.updates.slice(0, m), "finality", "deneb")
        if enc.status.any():
            raise SystemExit(f"rows refused by the encoder: {np.flatnonzero(enc.status)[:8].tolist()}")
        pitch = enc.buf.shape[1]
        msgs = (enc.buf.reshape(-1), np.arange(m, dtype=np.uint64) * np.uint64(pitch), enc.length.astype(np.uint64))
        rows = np.repeat(np.arange(m, dtype=np.uint32), k)
        stores = np.tile(np.arange(k, dtype=np.uint32), m)

        def relay(dedup):
            r = relay_updates(v, msgs, "finality", "deneb", rows, stores, cs, gvr, dedup=dedup)
            r.batch.free()
            return r

        def host_route():
            was = v.dedup
            host = wire.decode_updates(msgs, "finality", "deneb", lib=v.lib)
            tiled = take(host, rows)
            v.set_dedup(True)
            try:
                rb = v.upload(tiled, stores)
                try:
                    verdict, reason = v.validate_resident(rb, cs, gvr)
                    items = v.last_dedup()
                finally:
                    rb.free()
            finally:
                v.set_dedup(was)
            return verdict.astype(bool), reason, items

        def stream():
            item = (msgs, "finality", "deneb", rows, stores)
            got = list(relay_stream(v, (item for _ in range(args.in_flight)), cs, gvr, in_flight=args.in_flight, dedup=True))
            return got[-1], v.last_relay_timings((args.in_flight - 1) % args.in_flight)[0], got

        def enqueue_ms():
            """Host milliseconds of each of in_flight relay_async calls on free slots, under set_dedup(True)."""
            was = v.dedup
            v.set_dedup(True)
            try:
                out = []
                for slot in range(args.in_flight):
                    t = time.perf_counter()
                    v.relay_async(msgs, "finality", "deneb", rows, stores, cs, gvr, slot)
                    out.append((time.perf_counter() - t) * 1e3)
                for slot in range(args.in_flight):
                    v.slot_wait_relay(slot)
            finally:
                v.set_dedup(was)
            return statistics.median(out)

        def classify(fanned):
            """(call ms, keys ms, compares ms, classes) of one classify of the decoded batch, or of its unclassed fan-out."""
            rb, _ = v.decode_resident(msgs, "finality", "deneb")
            target = v.fan_out(rb, rows, stores) if fanned else rb
            try:
                t = time.perf_counter()
                classes = v.classify_resident(target)
                dt = (time.perf_counter() - t) * 1e3
                return (dt,) + v.last_classify_timings() + (classes,)
            finally:
                if fanned:
                    target.free()
                rb.free()

        times = {name: [] for name in ("relay_on", "relay_off", "host_route", "relay_stream")}
        kernel_ms, call_ms = [], []
        cl = {"decoded": [], "fanned": []}
        last = {}
        for run in range(args.warmup + args.runs):
            for name, call in (("relay_on", lambda: relay(True)), ("relay_off", lambda: relay(False)), ("host_route", host_route)):
                t = time.perf_counter()
                last[name] = call()
                if run >= args.warmup:
                    times[name].append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            last["relay_stream"] = stream()
            if run >= args.warmup:
                times["relay_stream"].append((time.perf_counter() - t) * 1e3 / args.in_flight)
                kernel_ms.append(last["relay_stream"][1])
                call_ms.append(enqueue_ms())
            for name in cl:
                c = classify(name == "fanned")
                if run >= args.warmup:
                    cl[name].append(c)
        on, off, host = last["relay_on"], last["relay_off"], last["host_route"]
        if not (np.array_equal(on.verdict, off.verdict) and np.array_equal(on.reason, off.reason) and
                np.array_equal(on.verdict, host[0]) and np.array_equal(on.reason, host[1])):
            raise SystemExit(f"{m} x {k}: the routes disagree")
        for g in last["relay_stream"][2]:
            if not (np.array_equal(on.verdict, g.verdict) and np.array_equal(on.reason, g.reason) and g.ok.all() and
                    tuple(g.dedup) == tuple(on.dedup)):
                raise SystemExit(f"{m} x {k}: relay_stream disagrees with relay_updates")
        r = {"messages": m, "stores": k, "pairs": n, "accepted": int(on.verdict.sum()),
             "last_dedup": {"relay_on": list(on.dedup), "relay_off": list(off.dedup), "host_route": list(host[2])},
             "classify": {name: {"rows": m if name == "decoded" else n, "classes": int(x[0][3]),
                                 "call_ms": med([c[0] for c in x]), "keys_kernel_ms": med([c[1] for c in x]),
                                 "compares_kernel_ms": med([c[2] for c in x])} for name, x in cl.items()},
             "ms": {name: med(x) for name, x in times.items()}, "relay_kernel_ms": med(kernel_ms),
             "relay_async_call_ms": med(call_ms)}
        relay(True)
        r["stage_ms_sync"] = {name: round(x, 3) for name, x in v.last_timings().items() if x}
        ms = {name: r["ms"][name]["median"] for name in times}
        r["relay_off_over_on"] = round(ms["relay_off"] / ms["relay_on"], 3)
        r["host_route_over_relay_on"] = round(ms["host_route"] / ms["relay_on"], 3)
        r["relay_on_over_relay_stream"] = round(ms["relay_on"] / ms["relay_stream"], 3)
        r["pairs_per_s"] = {name: round(n / (x * 1e-3)) for name, x in ms.items()}
        out["shapes"][f"{m}x{k}"] = r
        print(f"{m} x {k}: {ms} last_dedup {r['last_dedup']}", file=sys.stderr)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
