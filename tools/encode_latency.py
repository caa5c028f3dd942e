#!/usr/bin/env python3
"""What serialising a resident batch of light-client updates to SSZ wire bytes costs on one device
(lcv_batch_encode) against the present path (lcv_batch_download + lcv.wire.encode_updates, a Python loop).

Workload: the synthetic chain of tools/producer_latency.py (--n + 1 consecutive Deneb blocks, mainnet
configuration, one update per block), derived on the device into a resident batch; kind update, fork "auto".
  kernel    lcv_last_timings' wire_encode stage of whole-batch encode_resident calls (the sum over the call's chunks)
  call      the whole lcv_batch_encode call on the host clock, into a preallocated (n, pitch) array; beside it the
            rate at which the call's time outside the kernel moves the output (the device-to-host copy of n x pitch
            bytes into pageable memory): the bound the call sits at
  python    Verifier.download + lcv.wire.encode_updates over the same rows, --host-runs runs; its messages must equal
            the device's
  by_range  lcv.producer.updates_by_range for 128 periods: rank, best row per period, one 128-row encode, digests.
            The chain spans two mainnet periods, so for this figure alone the verifier is configured with
            --range-epochs epochs per period (the rows stay as they are; only the period of a slot changes)
--warmup warm-ups, median of --runs with min and max.  Prints the JSON and writes it to --out.
LCV_BENCH_HOSTSIM=1 runs on the host simulation (a dry run)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-client-consensus-specs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000, help="updates (one per block)")
    ap.add_argument("--fin-lag", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--range-epochs", type=int, default=2, help="epochs per period for the by-range figure")
    ap.add_argument("--out", default="encode_latency.json")
    args = ap.parse_args()
    from producer_latency import build_chain
    from lcv import producer as PR
    from lcv import wire
    from lcv._native import Lib
    from lcv.device import EncodedMessages, Verifier
    hostsim = os.environ.get("LCV_BENCH_HOSTSIM") == "1"
    lib = Lib(os.path.join(ROOT, "light-client-consensus-specs_amd", "build", "liblcv_hostsim.so")) if hostsim else None
    v = Verifier(0, lib=lib)
    cfg = v.config
    n = args.n
    states, blocks, cases = build_chain(n, args.fin_lag, 7, cfg)
    views = PR.pack_views(states, blocks)
    rb, reasons = v.create_updates_resident(views, cases)
    if reasons.any():
        raise SystemExit(f"rows failed to derive: {np.flatnonzero(reasons)[:8].tolist()}")
    pitch = v.encode_pitch("update")
    out = {"tool": "tools/encode_latency.py", "library": os.path.basename(v.lib.path), "build": v.lib.build_id(),
           "updates": n, "kind": "update", "fork": "auto", "pitch": pitch, "output_bytes": n * pitch,
           "warmup": args.warmup, "runs": args.runs}

    def med(xs):
        return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
                "runs": [round(x, 3) for x in xs]}

    # ---- device: the kernel's stage time and the whole call on the host clock, into the same arrays every run
    enc = EncodedMessages.empty(n, pitch)
    kernel, call = [], []
    for k in range(args.warmup + args.runs):
        t = time.perf_counter()
        v.encode_resident(rb, "update", "auto", out=enc)
        dt = time.perf_counter() - t
        if k >= args.warmup:
            call.append(dt * 1e3)
            kernel.append(v.last_timings()["wire_encode"])
    if enc.status.any():
        raise SystemExit(f"rows refused: {np.flatnonzero(enc.status)[:8].tolist()}")
    out["wire_encode_kernel_ms"] = med(kernel)
    out["batch_encode_call_ms"] = med(call)
    msg_bytes = int(enc.length.astype(np.int64).sum())
    out["message_bytes"] = msg_bytes
    k_ms, c_ms = out["wire_encode_kernel_ms"]["median"], out["batch_encode_call_ms"]["median"]
    out["kernel_GBps_read_plus_written"] = round((msg_bytes + n * pitch) / (k_ms * 1e-3) / 1e9, 1) if k_ms > 0 else None
    out["copy_GBps_outside_kernel"] = round(n * pitch / ((c_ms - k_ms) * 1e-3) / 1e9, 2) if c_ms > k_ms else None
    out["kernel_share_of_call"] = round(k_ms / c_ms, 4) if c_ms > 0 else None

    # ---- the present path: the rows to the host, then the Python encoder
    parts = {"download": [], "encode_updates": [], "total": []}
    msgs = None
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        down = v.download(rb)
        t1 = time.perf_counter()
        msgs = wire.encode_updates(down, "update", "deneb")
        t2 = time.perf_counter()
        for name, dt in (("download", t1 - t0), ("encode_updates", t2 - t1), ("total", t2 - t0)):
            parts[name].append(dt * 1e3)
    out["python_path_ms"] = {k: med(x) for k, x in parts.items()}
    if enc.messages() != msgs or set(enc.fork.tolist()) != {0}:
        raise SystemExit("device and Python messages differ")
    out["messages_equal_python_path"] = True
    out["python_over_device_call"] = round(out["python_path_ms"]["total"]["median"] / c_ms, 1)

    # ---- the by-range responder: 128 periods
    gvr = hashlib.sha256(b"encode_latency").digest()
    v.set_config(cfg.with_(EPOCHS_PER_SYNC_COMMITTEE_PERIOD=args.range_epochs))
    try:
        first = int(blocks[0].slot) // v.config.SLOTS_PER_PERIOD + 1
        ms, chunks = [], []
        for k in range(args.warmup + args.runs):
            t = time.perf_counter()
            chunks = PR.updates_by_range(rb, first, 128, gvr, v)
            dt = time.perf_counter() - t
            if k >= args.warmup:
                ms.append(dt * 1e3)
        out["updates_by_range_ms"] = med(ms)
        out["updates_by_range_chunks"] = len(chunks)
        out["updates_by_range_slots_per_period"] = v.config.SLOTS_PER_PERIOD
    finally:
        v.set_config(cfg)
    rb.free()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
