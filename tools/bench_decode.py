"""Decode benchmark: times `Decoder.decode` on the C2 stream (-cs8 -cpf4096
-cbd8, 44.1 kHz stereo synthetic) and checks the PCM against the oracle.

  python tools/bench_decode.py [--seconds 1024] [--steps 7] [--warmup 2] [--lib PATH] [--out FILE]

The .gsc is produced once by the encoder outside the timed region.  Each step
is one `gsc_decode` call (host walk, upload, unpack, synthesis, download); the
figures are the medians over the steps of `gsc_last_decode_timing`'s stages,
beside the oracle's single-threaded decode of the same bytes on this host.
Prints one JSON line.  --lib times another build of the library (the A/B of
the checkpoint spacing S builds it with -DGSC_DECODE_S=...).
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
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1024.0)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lib", default=None, help="path of another libsoundchunks_amd.so to time")
    ap.add_argument("--gsc", default=None, help="cache file of the encoded stream (written when missing)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import numpy as np

    import oracle_ffi
    import soundchunks_amd as sc
    from soundchunks_amd import _lib
    from soundchunks_amd.synth import synth_wav

    if args.lib:
        _lib._lib = _lib.load(args.lib)
    argv = ["-cs8", "-cpf4096", "-cbd8"]
    cache = Path(args.gsc) if args.gsc else None
    if cache and cache.exists():
        gsc = cache.read_bytes()
    else:
        gsc = sc.Encoder(argv).encode(synth_wav(args.seconds, 44100, 2))
        if cache:
            cache.parent.mkdir(parents=True, exist_ok=True)
            cache.write_bytes(gsc)

    t0 = time.perf_counter()
    want, ch, rate = oracle_ffi.decode(gsc)
    oracle_ms = (time.perf_counter() - t0) * 1e3

    dec = sc.Decoder()
    runs = []
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        pcm, got_rate = dec.decode(gsc)
        wall = (time.perf_counter() - t0) * 1e3
        if i == 0:
            assert got_rate == rate and pcm.shape[1] == ch
            assert np.array_equal(pcm.reshape(-1), want), "decoded PCM differs from the oracle's"
        t = dec.last_timing()
        t["python_wall_ms"] = wall
        if i >= args.warmup:
            runs.append(t)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0] if k.endswith("_ms")}
    spread = {k: [min(r[k] for r in runs), max(r[k] for r in runs)] for k in med}
    dev_ms = med["gpu_unpack_ms"] + med["gpu_synth_ms"]
    moved = len(gsc) + 2 * runs[0]["symbols"] * 2 + 2 * runs[0]["samples"]  # bytes in, symbol words out + in, PCM out
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {
        "bench": "decode", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
        "commit": commit, "lib": args.lib or "in-tree", "checkpoint_symbols": dec.checkpoint_symbols(),
        "gsc_bytes": len(gsc), "frames": runs[0]["frames"], "symbols": runs[0]["symbols"],
        "pcm_bytes": 2 * runs[0]["samples"], "steps": args.steps, "warmup": args.warmup,
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(a, 3), round(b, 3)] for k, (a, b) in spread.items()},
        "oracle_decode_ms": round(oracle_ms, 1),
        "host_walk_share": round(med["host_index_ms"] / med["total_ms"], 3),
        "device_stages_ms": round(dev_ms, 3),
        "device_bytes_moved": moved,
        "device_GBps": round(moved / dev_ms / 1e6, 1),
        "pcm_matches_oracle": True,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
