"""Bound-crop benchmark: random crops of the C2 stream (-cs8 -cpf4096 -cbd8,
44.1 kHz stereo synthetic, as tools/bench_decode_crops.py) decoded two ways in
one process.

  python tools/bench_decode_crops_bound.py [--seconds 1024] [--steps 10] [--warmup 3] [--gsc CACHE] [--out FILE]
                                           [--commit TEXT]

  bound      `Decoder.bind([st], ...)` once, then `binding.decode_crops(crops)`
             with the crops already in a device tensor: the kernel plans them
  host       `Decoder.decode_crops([st], crops, ...)` with the same crops as a
             host list: planned on the host, one allocation and one copy per call

for 64 x 1 s, 256 x 1 s and 1024 x 0.05 s at the stream's own rate and 64 x 1 s
brought to 48 kHz stereo.  The two alternate call by call.  Per call three
clocks, each the median (min, max) of --steps repetitions after --warmup:

  enqueue_ms  host time of the call alone, the device idle before it
  device_ms   between two events around the call on its stream
  wall_ms     between two device synchronisations around the call

Outputs and written lengths are compared after the clock; a difference exits
with status 3.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# (crops per call, crop length in seconds, output rate or None, output channels or None)
WORKLOADS = [(64, 1.0, None, None), (256, 1.0, None, None), (1024, 0.05, None, None), (64, 1.0, 48000, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1024.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gsc", default=None, help="cache file of the encoded stream (written when missing)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git HEAD)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import soundchunks_amd as sc
    from soundchunks_amd.synth import synth_wav

    cache = Path(args.gsc) if args.gsc else None
    if cache and cache.exists():
        gsc = cache.read_bytes()
    else:
        gsc = sc.Encoder(["-cs8", "-cpf4096", "-cbd8"]).encode(synth_wav(args.seconds, 44100, 2))
        if cache:
            cache.parent.mkdir(parents=True, exist_ok=True)
            cache.write_bytes(gsc)

    st = sc.Decoder.open(gsc)
    n, fi = st.samples_per_channel, st.sample_rate
    dev = torch.device("cuda", st.device)
    rng = np.random.default_rng(2026)

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def clocked(fn):
        """(result, enqueue ms, device ms, wall ms) of one call"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        ta = time.perf_counter()
        r = fn()
        tb = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        return r, (tb - ta) * 1e3, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    results, ok = [], True
    for batch, secs, rate, channels in WORKLOADS:
        fo = fi if rate is None else rate
        T = int(round(secs * fo))
        src = int(round(secs * fi)) + 64  # source samples a crop reads, the filter's reach included
        if src > n:
            continue
        begins = rng.integers(0, n - src + 1, batch)
        crops = [(0, int(b), T) for b in begins]
        if rate is not None:
            sc.Decoder.prepare_resample(fi, rate)
        binding = sc.Decoder.bind([st], rate=rate, channels=channels)
        ch = binding.channels
        crops_dev = torch.tensor(crops, dtype=torch.int64, device=dev)
        out_b = torch.empty((batch, T, ch), dtype=torch.int16, device=dev)
        out_h = torch.empty((batch, T, ch), dtype=torch.int16, device=dev)
        written = torch.empty((batch,), dtype=torch.int64, device=dev)

        def bound():
            return binding.decode_crops(crops_dev, T, out=out_b, written=written)

        def host():
            return sc.Decoder.decode_crops([st], crops, length=T, out=out_h, rate=rate, channels=channels)

        t = {"bound": ([], [], []), "host": ([], [], [])}
        for i in range(args.warmup + args.steps):
            for name, fn in (("host", host), ("bound", bound)):
                _, enq, devms, wall = clocked(fn)
                if i >= args.warmup:
                    for k, v in enumerate((enq, devms, wall)):
                        t[name][k].append(v)
        call = binding.last_call()
        _, nh = host()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out_b, out_h) and written.tolist() == nh)
        ok = ok and equal
        row = {"crops": batch, "crop_seconds": secs, "crop_samples": T, "rate": fo, "channels": ch,
               "kernel": "fused" if rate is None and channels is None else "resample"}
        for name in ("bound", "host"):
            for k, clock in enumerate(("enqueue_ms", "device_ms", "wall_ms")):
                row[f"{name}_{clock}"] = stats(t[name][k])
        row["bound_last_call"] = call
        row["enqueue_ratio"] = round(row["host_enqueue_ms"][0] / row["bound_enqueue_ms"][0], 1)
        row["device_ratio"] = round(row["bound_device_ms"][0] / row["host_device_ms"][0], 3)
        # the expectation: the in-kernel plan costs no more device time than the host-planned runs spread
        row["bound_device_within_host_max"] = bool(row["bound_device_ms"][0] <= row["host_device_ms"][2])
        row["outputs_equal"] = equal
        results.append(row)
        binding.close()

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = {"bench": "decode_crops_bound", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
           "commit": commit, "gsc_bytes": len(gsc), "frames": st.frame_count, "steps": args.steps,
           "warmup": args.warmup, "times": "[median, min, max] ms", "workloads": results}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    if not ok:
        print("bench_decode_crops_bound: the bound and the host-planned outputs differ", file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
