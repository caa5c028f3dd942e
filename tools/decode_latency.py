#!/usr/bin/env python3
"""What decoding SSZ wire messages into a resident batch costs on one device (lcv_batch_decode) against the present
path (lcv.wire.decode_updates on the host's threads + Verifier.upload).

Workload: the synthetic chain of tools/encode_latency.py (--n consecutive Deneb updates, mainnet configuration, 3
committees), derived on the device and encoded once per kind by lcv_batch_encode; the messages are handed over as one
buffer with offsets and lengths, as a received payload is.  Per kind (update, finality, optimistic):
  kernel    lcv_last_decode_timings: [0] the decode kernel's passes, [1] the committee compares and the pool gather
  call      the whole lcv_batch_decode call on the host clock (staging copy, one DMA, kernels, records back)
  host      decode_updates + Verifier.upload on the same messages, --host-runs runs
  host_over_device_call   host / call, as it comes out
  link_ms   the staged bytes over the host-to-device link at --link-gbps (the DMA's share of the call)
The device rows must equal the host rows for every message.  --warmup warm-ups, median of --runs with min and max.
Prints the JSON and writes it to --out.  LCV_BENCH_HOSTSIM=1 runs on the host simulation (a dry run)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-client-consensus-specs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ("update", "finality", "optimistic")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000, help="messages per kind")
    ap.add_argument("--fin-lag", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--link-gbps", type=float, default=52.6, help="host-to-device rate the copy is set against")
    ap.add_argument("--out", default="decode_latency.json")
    args = ap.parse_args()
    from producer_latency import build_chain
    from lcv import producer as PR
    from lcv import wire
    from lcv._native import Lib
    from lcv.device import Verifier
    hostsim = os.environ.get("LCV_BENCH_HOSTSIM") == "1"
    lib = Lib(os.path.join(ROOT, "light-client-consensus-specs_amd", "build", "liblcv_hostsim.so")) if hostsim else None
    v = Verifier(0, lib=lib)
    n = args.n
    states, blocks, cases = build_chain(n, args.fin_lag, 7, v.config)
    views = PR.pack_views(states, blocks)
    rb, reasons = v.create_updates_resident(views, cases)
    if reasons.any():
        raise SystemExit(f"rows failed to derive: {np.flatnonzero(reasons)[:8].tolist()}")
    out = {"tool": "tools/decode_latency.py", "library": os.path.basename(v.lib.path), "build": v.lib.build_id(),
           "messages": n, "fork": "deneb", "committees": views.ncomm, "warmup": args.warmup, "runs": args.runs,
           "link_GBps": args.link_gbps, "kinds": {}}

    def med(xs):
        return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
                "runs": [round(x, 3) for x in xs]}

    for kind in KINDS:
        enc = v.encode_resident(rb, kind, "deneb")
        if enc.status.any():
            raise SystemExit(f"rows refused by the encoder: {np.flatnonzero(enc.status)[:8].tolist()}")
        pitch = enc.buf.shape[1]
        msgs = (enc.buf.reshape(-1), (np.arange(n, dtype=np.uint64) * np.uint64(pitch)), enc.length.astype(np.uint64))
        staged = int(((enc.length.astype(np.int64) + 15) & ~15).sum()) + 16
        r = {"message_bytes": int(enc.length.astype(np.int64).sum()), "staged_bytes": staged}
        # ---- the present path
        parts = {"decode_updates": [], "upload": [], "total": []}
        host = None
        for _ in range(args.host_runs):
            t0 = time.perf_counter()
            host = wire.decode_updates(msgs, kind, "deneb", lib=v.lib)
            t1 = time.perf_counter()
            up = v.upload(host)
            t2 = time.perf_counter()
            up.free()
            for name, dt in (("decode_updates", t1 - t0), ("upload", t2 - t1), ("total", t2 - t0)):
                parts[name].append(dt * 1e3)
        r["host_path_ms"] = {k: med(x) for k, x in parts.items()}
        # ---- the device path
        kernel, pool, call = [], [], []
        got = None
        for k in range(args.warmup + args.runs):
            t = time.perf_counter()
            db, ok = v.decode_resident(msgs, kind, "deneb")
            dt = time.perf_counter() - t
            if not ok.all():
                raise SystemExit(f"{kind}: messages refused: {np.flatnonzero(~ok)[:8].tolist()}")
            if k >= args.warmup:
                call.append(dt * 1e3)
                t0, t1 = v.last_decode_timings()
                kernel.append(t0)
                pool.append(t1)
            if k == args.warmup + args.runs - 1:
                got = v.download(db)
            db.free()
        r["decode_kernel_ms"] = med(kernel)
        r["pool_kernels_ms"] = med(pool)
        r["batch_decode_call_ms"] = med(call)
        from lcv.device import PackedUpdates
        for name, (_, _, is_pool) in PackedUpdates._SPEC.items():
            a, b = getattr(got, name), getattr(host, name)
            if is_pool:
                a, b = a[got.nsc_index], b[host.nsc_index]
            if not np.array_equal(a, b):
                raise SystemExit(f"{kind}: device and host rows differ in {name}")
        r["rows_equal_host_path"] = True
        r["pool_rows"] = int(got.nsc_pool.shape[0])
        c_ms = r["batch_decode_call_ms"]["median"]
        r["host_over_device_call"] = round(r["host_path_ms"]["total"]["median"] / c_ms, 2) if c_ms > 0 else None
        r["link_ms"] = round(staged / (args.link_gbps * 1e9) * 1e3, 3)
        r["link_share_of_call"] = round(r["link_ms"] / c_ms, 3) if c_ms > 0 else None
        r["decodes_per_s_call"] = round(n / (c_ms * 1e-3)) if c_ms > 0 else None
        out["kinds"][kind] = r
    rb.free()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
