"""Envelope benchmark: block energy and peak of the C2 stream (-cs8 -cpf4096
-cbd8, 44.1 kHz stereo synthetic, as tools/bench_decode_crops_bound.py) at a hop
of 1024 samples, two ways in one process.

  python tools/bench_envelope.py [--seconds 1024] [--hop 1024] [--steps 10] [--warmup 3] [--gsc CACHE] [--out FILE]
                                 [--commit TEXT] [--set-streams 1024]

  envelope   `binding.envelope(hop)` into tensors that exist: one launch, straight
             from the compressed slabs
  decode     what the library offered before for the same numbers: the bound
             `decode_crops` of the whole stream into a device tensor, in rows of
             1 s, then the reductions in torch (square and |.| in int32, block
             sums in int64)

The two alternate call by call.  Per path the median (min, max) of --steps
repetitions after --warmup of

  device_ms  between two events around the path on its stream
  wall_ms    between two device synchronisations around it

and the peak device memory each allocates above what is resident
(`torch.cuda.max_memory_allocated`).  The envelope call waits for its stream
itself, so its wall time holds that wait.  Then the same for a set of
--set-streams copies of the 2-s stereo golden (tests/golden), whose last tile is
ragged.  Outputs are compared after the clock; a difference exits with status 3.
Prints one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1024.0)
    ap.add_argument("--hop", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--set-streams", type=int, default=1024)
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
    hop = args.hop

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def clocked(fn):
        """(device ms, wall ms, peak bytes allocated above the start) of one run of fn"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return e0.elapsed_time(e1), wall, torch.cuda.max_memory_allocated() - base

    def measure(streams, row_len):
        """Both paths over `streams` (equal lengths and channels); the decode path in rows of row_len samples."""
        binding = sc.Decoder.bind(streams)
        dev, ch = binding.device, binding.channels
        n = streams[0].samples_per_channel
        rows = -(-n // row_len)
        crops = torch.tensor([(s, r * row_len, min(row_len, n - r * row_len)) for s in range(len(streams))
                              for r in range(rows)], dtype=torch.int64, device=dev)
        nb = -(-n // hop)
        total = nb * len(streams)
        energy = torch.empty(total, dtype=torch.int64, device=dev)
        peak = torch.empty(total, dtype=torch.int32, device=dev)
        got = {}

        def envelope():
            binding.envelope(hop, energy=energy, peak=peak)

        def decode():
            x, _ = binding.decode_crops(crops, row_len)  # [streams * rows, row_len, ch], zero past a stream's end
            x = x.view(len(streams), rows * row_len, ch)[:, :n].to(torch.int32)
            x = torch.nn.functional.pad(x, (0, 0, 0, nb * hop - n)).view(total, hop * ch)
            got["peak"] = x.abs().amax(dim=1)
            got["energy"] = x.square_().sum(dim=1, dtype=torch.int64)

        t = {"envelope": ([], [], []), "decode": ([], [], [])}
        for i in range(args.warmup + args.steps):
            for name, fn in (("decode", decode), ("envelope", envelope)):
                r = clocked(fn)
                if i >= args.warmup:
                    for k, v in enumerate(r):
                        t[name][k].append(v)
        equal = bool(torch.equal(got["energy"], energy) and torch.equal(got["peak"].to(torch.int32), peak))
        row = {"streams": len(streams), "samples": n, "channels": ch, "hop": hop, "blocks": total,
               "decode_rows": rows * len(streams), "decode_row_samples": row_len, "outputs_equal": equal,
               "silent_blocks": int((energy == 0).sum())}
        for name in ("envelope", "decode"):
            row[f"{name}_device_ms"] = stats(t[name][0])
            row[f"{name}_wall_ms"] = stats(t[name][1])
            row[f"{name}_peak_bytes"] = int(max(t[name][2]))
        row["device_ratio"] = round(row["envelope_device_ms"][0] / row["decode_device_ms"][0], 3)
        binding.close()
        return row, equal

    st = sc.Decoder.open(gsc)
    head, ok = measure([st], st.sample_rate)
    st.close()
    small = (ROOT / "tests" / "golden" / "syn2s_c2_cs8_cpf4096.gsc").read_bytes()
    ss = sc.Decoder.open_many([small] * args.set_streams)
    ragged, ok2 = measure(ss.streams, ss[0].samples_per_channel)
    ss.close()

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = {"bench": "envelope", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
           "commit": commit, "gsc_bytes": len(gsc), "steps": args.steps, "warmup": args.warmup,
           "times": "[median, min, max] ms", "headline": head, "set": ragged}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    if not (ok and ok2):
        print("bench_envelope: the envelope and the decoded reduction differ", file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
