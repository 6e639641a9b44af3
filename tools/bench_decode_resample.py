"""Resampled-crop benchmark: random 1 s crops of the C2 stream (-cs8 -cpf4096
-cbd8, 44.1 kHz stereo synthetic) brought to another rate and channel count on
the device, against the native-rate `decode_crops` of the same crops.

  python tools/bench_decode_resample.py [--seconds 1024] [--steps 10] [--warmup 3] [--gsc CACHE] [--out FILE]
                                        [--commit TEXT]

  native     `Decoder.decode_crops(crops, length=44100)`: the fused kernel, the
             floor the new path cannot beat (it decodes the same source second)
  resampled  `Decoder.decode_crops(crops, length=rate, rate=rate, channels=c)`
             for 48000 Hz stereo (32 taps, 0.92 source samples per output) and
             16000 Hz mono (90 taps, 2.76 source samples per output, two source
             channels filtered per output)

The two alternate call by call in one session.  Times are the median (min, max)
of --steps repetitions after --warmup: wall clock between two device
synchronisations, and device time between two events on the stream.  The
tables are uploaded before the clock (`prepare_resample`).  After the clock
every output is checked against the integer definition applied in numpy to the
native-rate decode of the whole second and its surroundings (itself checked
against the oracle by the tests); a difference exits non-zero.  Prints one
JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from math import gcd
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BATCHES = [64, 256]
TARGETS = [(48000, 2), (16000, 1)]  # (rate, channels)


def model(pcm, begins, table, fi, fo, co):
    """int16 [B, fo, co]: one second of output from each begin, by the definition."""
    import numpy as np

    g = gcd(fi, fo)
    L, M = fo // g, fi // g
    T = table.shape[1] // 2
    n_s, cs = pcm.shape
    xp = np.pad(pcm.astype(np.int64), ((T, T + 1), (0, 0)))
    tab = table.astype(np.int64)
    out = np.zeros((len(begins), fo, co), np.int16)
    n = np.arange(fo, dtype=np.int64)
    for i, b in enumerate(begins):
        pos = int(b) * L + n * M
        i0, ph = pos // L, pos % L
        assert i0[-1] < n_s
        acc = np.zeros((fo, cs), np.int64)
        for j in range(2 * T):
            acc += tab[ph, j][:, None] * xp[i0 + j + 1]  # sample i0 + (j - T + 1) sits at xp[. + T]
        y = np.clip((acc + (1 << 23)) >> 24, -32768, 32767)
        if co == 1 and cs > 1:
            y = (2 * y.sum(axis=1, keepdims=True) + cs) // (2 * cs)
        out[i] = y
    return out


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
    n, ch, fi = st.samples_per_channel, st.channels, st.sample_rate
    pcm = st.index.decode()  # the whole stream at its own rate: the model's input
    rng = np.random.default_rng(2025)

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def clocked(fn):
        """(result, wall ms, device ms) of one call"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    results, ok = [], True
    for fo, co in TARGETS:
        sc.Decoder.prepare_resample(fi, fo)
        table = sc.Decoder.resample_table(fi, fo)
        for batch in BATCHES:
            begins = rng.integers(0, n - fi - table.shape[1], batch)
            native_crops = [(0, int(b), fi) for b in begins]
            crops = [(0, int(b), fo) for b in begins]

            def native():
                return sc.Decoder.decode_crops([st], native_crops, length=fi)[0]

            def resampled():
                return sc.Decoder.decode_crops([st], crops, length=fo, rate=fo, channels=co)[0]

            t = {"native": ([], []), "resampled": ([], [])}
            for i in range(args.warmup + args.steps):
                for name, fn in (("native", native), ("resampled", resampled)):
                    x, wall, dev = clocked(fn)
                    if i >= args.warmup:
                        t[name][0].append(wall)
                        t[name][1].append(dev)
                    if name == "resampled":
                        got = x
            want = model(pcm, begins, table, fi, fo, co)
            equal = bool(np.array_equal(got.cpu().numpy(), want))
            ok = ok and equal
            row = {"crops": batch, "rate": fo, "channels": co, "taps": int(table.shape[1]),
                   "phases": int(table.shape[0]), "source_samples_per_output": round(fi / fo, 4),
                   "native_wall_ms": stats(t["native"][0]), "native_device_ms": stats(t["native"][1]),
                   "resampled_wall_ms": stats(t["resampled"][0]), "resampled_device_ms": stats(t["resampled"][1]),
                   "outputs_equal_model": equal}
            row["wall_ratio"] = round(row["resampled_wall_ms"][0] / row["native_wall_ms"][0], 2)
            row["device_ratio"] = round(row["resampled_device_ms"][0] / row["native_device_ms"][0], 2)
            # multiply-adds of the call: outputs x source channels filtered x taps
            mads = batch * fo * ch * table.shape[1]
            row["multiply_adds"] = int(mads)
            row["device_ns_per_1000_multiply_adds"] = round(
                (row["resampled_device_ms"][0] - row["native_device_ms"][0]) * 1e6 / (mads / 1000), 3)
            results.append(row)

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = {"bench": "decode_resample", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
           "commit": commit, "gsc_bytes": len(gsc), "frames": st.frame_count, "tile": sc.Decoder.resample_tile(),
           "steps": args.steps, "warmup": args.warmup, "times": "[median, min, max] ms", "workloads": results}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    if not ok:
        print("bench_decode_resample: an output differs from the model", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
