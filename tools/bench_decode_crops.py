"""Crop-decode benchmark: random crops of the C2 stream (-cs8 -cpf4096 -cbd8,
44.1 kHz stereo synthetic) into an int16 [B, T, C] tensor on the device, two ways.

  python tools/bench_decode_crops.py [--seconds 1024] [--steps 10] [--warmup 3] [--gsc CACHE] [--out FILE]
                                     [--commit TEXT]

  resident   `Decoder.open` once (outside the timed region, its time reported),
             then one `Decoder.decode_crops` call per batch
  parent     what the package offered before resident streams: a kept `Index`,
             `ix.decode(frame range)` per crop, a host slice into a [B, T, C]
             array, one `torch` upload; and, beside it, one `ix.decode()` of
             the whole stream sliced on the host (the cheaper of the two is
             the figure to beat)

Every workload's outputs are checked equal (torch.equal).  Times are the
median (min, max) of --steps repetitions after --warmup, wall clock between
two device synchronisations; `device_ms` is the resident path between two
events on the stream.  Prints one JSON line.
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

# (crops per call, crop length in seconds); the first is the headline workload
WORKLOADS = [(64, 1.0), (1, 1.0), (16, 0.25), (256, 1.0), (64, 4.0), (1024, 0.05)]


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

    def timed(fn, sync=True):
        runs = []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            if sync:
                torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                runs.append(dt)
        return r, [round(statistics.median(runs), 4), round(min(runs), 4), round(max(runs), 4)]

    t0 = time.perf_counter()
    st = sc.Decoder.open(gsc)
    open_ms = (time.perf_counter() - t0) * 1e3
    open_t = sc.Decoder.last_timing()
    ix = sc.Decoder.index(gsc)
    first = ix.first_sample
    n, ch, rate = st.samples_per_channel, st.channels, st.sample_rate
    dev = torch.device("cuda", st.device)
    rng = np.random.default_rng(2024)

    results = []
    for batch, secs in WORKLOADS:
        T = int(round(secs * rate))
        if T > n:
            continue
        begins = rng.integers(0, n - T + 1, batch)
        crops = [(0, int(b), T) for b in begins]

        def resident():
            return sc.Decoder.decode_crops([st], crops, length=T, dtype=torch.int16, layout="TC")[0]

        def resident_float_ct():
            return sc.Decoder.decode_crops([st], crops, length=T, dtype=torch.float32, layout="CT")[0]

        def device_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            resident()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def parent_per_crop():
            host = np.empty((batch, T, ch), np.int16)
            for i, b in enumerate(begins):
                fa = int(np.searchsorted(first, b, side="right")) - 1
                fb = int(np.searchsorted(first, b + T - 1, side="right")) - 1
                pcm = ix.decode(fa, fb + 1)
                host[i] = pcm[b - first[fa]:b - first[fa] + T]
            return torch.from_numpy(host).to(dev)

        def parent_whole():
            pcm = ix.decode()
            host = np.stack([pcm[b:b + T] for b in begins])
            return torch.from_numpy(host).to(dev)

        row = {"crops": batch, "crop_seconds": secs, "crop_samples": T}
        x, row["resident_ms"] = timed(resident)
        devs = sorted(device_ms() for _ in range(args.steps))
        row["device_ms"] = [round(statistics.median(devs), 4), round(devs[0], 4), round(devs[-1], 4)]
        row["h2d_bytes"] = sc.Decoder.last_timing()["h2d_bytes"]
        xf, row["resident_float32_ct_ms"] = timed(resident_float_ct)
        _, row["resident_enqueue_only_ms"] = timed(resident, sync=False)
        yp, row["parent_per_crop_ms"] = timed(parent_per_crop)
        yw, row["parent_whole_stream_ms"] = timed(parent_whole)
        equal = bool(torch.equal(x, yp) and torch.equal(x, yw) and
                     torch.equal(xf, (x.to(torch.float32) / 32768).transpose(1, 2).contiguous()))
        assert equal, f"outputs differ at {batch} crops of {secs} s"
        row["outputs_equal"] = equal
        row["speedup_over_best_parent"] = round(min(row["parent_per_crop_ms"][0], row["parent_whole_stream_ms"][0]) /
                                                row["resident_ms"][0], 1)
        results.append(row)
        del x, xf, yp, yw

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = {
        "bench": "decode_crops", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
        "commit": commit, "gsc_bytes": len(gsc), "frames": st.frame_count,
        "checkpoint_symbols": sc.Decoder.checkpoint_symbols(), "steps": args.steps, "warmup": args.warmup,
        "times": "[median, min, max] ms",
        "open_ms": round(open_ms, 2), "open_host_walk_ms": round(open_t["host_index_ms"], 2),
        "open_h2d_bytes": open_t["h2d_bytes"], "workloads": results,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
