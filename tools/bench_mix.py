"""Mix benchmark: gain-weighted sums of crops of the C2 stream (-cs8 -cpf4096
-cbd8, 44.1 kHz stereo synthetic, as tools/bench_fidelity.py), two ways in one
process.

  python tools/bench_mix.py [--seconds 1024] [--steps 10] [--warmup 3] [--gsc CACHE] [--out FILE] [--commit TEXT]

  mix      `binding.mix(sources, length)` into tensors that exist: one launch,
           the R x K crops summed in LDS, R rows written
  decode   what a user did before for the same rows: the bound `decode_crops` of
           the R x K crops into a device tensor, then the definition in torch:
           widened to int64, times the gains, summed over K, + 16384, >> 15,
           clamped, narrowed to int16

Four workloads: R = 64 rows of K = 3 crops of 1 s and R = 1024 rows of K = 2
crops of 0.05 s, each with a native binding and with one at 48 kHz stereo.
Crops start at random samples, gains are random within +-2 x unity.  The two
outputs (rows and written) are compared before the clock; a difference exits
with status 3.  The paths alternate call by call.  Per path the median (min,
max) of --steps repetitions after --warmup of

  enqueue_ms  host time until the path's calls have returned (nothing waited for)
  device_ms   between two events around the path on its stream
  wall_ms     between two device synchronisations around it

the peak device memory each allocates above what is resident
(`torch.cuda.max_memory_allocated`; the mix path writes into tensors made
before the clock, the decode path into tensors it makes, as a user would), and
the bytes of PCM each writes.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1024.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gsc", default=None, help="cache file of the encoded stream (written when missing)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git HEAD)")
    args = ap.parse_args()

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

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def clocked(fn):
        """(enqueue ms, device ms, wall ms, peak bytes allocated above the start) of one run of fn"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        enq = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return enq, e0.elapsed_time(e1), wall, torch.cuda.max_memory_allocated() - base

    st = sc.Decoder.open(gsc)
    dev = torch.device("cuda", st.device)
    n = st.samples_per_channel

    def measure(name, R, K, seconds, rate, channels):
        binding = sc.Decoder.bind([st], rate=rate, channels=channels)
        ch = binding.channels
        length = int(round(seconds * (rate or st.sample_rate)))
        rng = np.random.default_rng(R + K)
        src = np.zeros((R, K, 4), np.int64)
        src[..., 1] = rng.integers(0, n - int(seconds * st.sample_rate) - 64, (R, K))
        src[..., 2] = length
        src[..., 3] = rng.integers(-65536, 65537, (R, K))
        sources = torch.from_numpy(src).to(dev)
        crops = sources[..., :3].reshape(R * K, 3).contiguous()
        gains = sources[..., 3].reshape(R, K, 1, 1).contiguous()
        out = torch.empty((R, length, ch), dtype=torch.int16, device=dev)
        written = torch.empty((R,), dtype=torch.int64, device=dev)
        got = {}

        def mix():
            binding.mix(sources, length, out=out, written=written)

        def decode():
            x, w = binding.decode_crops(crops, length)  # [R * K, length, ch]
            s = (x.view(R, K, length, ch).to(torch.int64) * gains).sum(dim=1)
            got["x"] = ((s + 16384) >> 15).clamp_(-32768, 32767).to(torch.int16)
            got["w"] = w.view(R, K).amax(dim=1)

        mix()
        decode()
        torch.cuda.synchronize()
        equal = bool(torch.equal(got["x"], out) and torch.equal(got["w"], written))
        paths = (("decode", decode), ("mix", mix))
        t = {p: ([], [], [], []) for p, _ in paths}
        for i in range(args.warmup + args.steps):
            for p, fn in paths:
                res = clocked(fn)
                if i >= args.warmup:
                    for k, v in enumerate(res):
                        t[p][k].append(v)
        row = {"workload": name, "rows": R, "sources_per_row": K, "length": length, "channels": ch,
               "rate": rate or st.sample_rate, "converted": rate is not None or channels is not None,
               "outputs_equal": equal, "mix_pcm_bytes_written": R * length * ch * 2,
               "decode_pcm_bytes_written": R * K * length * ch * 2 + R * length * ch * 2}
        for p, _ in paths:
            for k, what in enumerate(("enqueue_ms", "device_ms", "wall_ms")):
                row[f"{p}_{what}"] = stats(t[p][k])
            row[f"{p}_peak_bytes"] = int(max(t[p][3]))
        row["device_ratio_to_decode"] = round(row["mix_device_ms"][0] / row["decode_device_ms"][0], 3)
        binding.close()
        return row

    rows = [measure("R64_K3_1s_native", 64, 3, 1.0, None, None),
            measure("R1024_K2_50ms_native", 1024, 2, 0.05, None, None),
            measure("R64_K3_1s_48k_stereo", 64, 3, 1.0, 48000, 2),
            measure("R1024_K2_50ms_48k_stereo", 1024, 2, 0.05, 48000, 2)]
    st.close()

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = {"bench": "mix", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
           "commit": commit, "gsc_bytes": len(gsc), "steps": args.steps, "warmup": args.warmup,
           "times": "[median, min, max] ms", "workloads": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    if not all(r["outputs_equal"] for r in rows):
        print("bench_mix: the mix call and the decoded sum differ", file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
