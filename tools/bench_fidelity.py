"""Fidelity benchmark: block error energy of the C2 stream (-cs8 -cpf4096 -cbd8,
44.1 kHz stereo synthetic, as tools/bench_envelope.py) against its source PCM at
a hop of 1024 samples, three ways in one process.

  python tools/bench_fidelity.py [--seconds 1024] [--hop 1024] [--steps 10] [--warmup 3] [--gsc CACHE] [--out FILE]
                                 [--commit TEXT] [--set-streams 1024]

  fidelity   `binding.fidelity(refs, hop)` into tensors that exist: one launch,
             straight from the compressed slabs, the references read in place
  decode     what the library offered before for the same numbers: the bound
             `decode_crops` of the whole stream into a device tensor, in rows of
             1 s, then the difference, the squares (the error's in int64: it
             does not fit int32) and the block sums in torch
  envelope   `binding.envelope(hop)` on the same streams: the same walk without
             the second operand

The three alternate call by call.  Per path the median (min, max) of --steps
repetitions after --warmup of

  device_ms  between two events around the path on its stream
  wall_ms    between two device synchronisations around it

and the peak device memory each allocates above what is resident
(`torch.cuda.max_memory_allocated`).  The fidelity and envelope calls wait for
their stream themselves, so their wall time holds that wait.  The headline
stream's reference is the PCM it was encoded from (no longer than the stream:
the encoder pads).  Then the same for a set of --set-streams copies of
the 2-s stereo golden (tests/golden), whose last tile is ragged, against random
full-range references of the streams' own length, which the decode path reads
as one tensor.  The fidelity and decode outputs are compared after the clock; a
difference exits with status 3.  Prints one JSON line.
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

    wav = synth_wav(args.seconds, 44100, 2)
    pcm = np.frombuffer(wav, "<i2", offset=44).reshape(-1, 2).astype(np.int16)
    cache = Path(args.gsc) if args.gsc else None
    if cache and cache.exists():
        gsc = cache.read_bytes()
    else:
        gsc = sc.Encoder(["-cs8", "-cpf4096", "-cbd8"]).encode(wav)
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

    def measure(streams, row_len, refs):
        """The three paths over `streams` (equal lengths and channels); the decode path in rows of row_len samples.
        refs: one int16 tensor [len(streams), R, ch] on the device, R at most the streams' length."""
        binding = sc.Decoder.bind(streams)
        dev, ch = binding.device, binding.channels
        n = streams[0].samples_per_channel
        rows = -(-n // row_len)
        crops = torch.tensor([(s, r * row_len, min(row_len, n - r * row_len)) for s in range(len(streams))
                              for r in range(rows)], dtype=torch.int64, device=dev)
        nb = -(-n // hop)
        total = nb * len(streams)
        ref_list = list(refs.unbind(0))
        R = refs.shape[1]
        out = {k: torch.empty(total, dtype=dt, device=dev)
               for k, dt in (("err_energy", torch.int64), ("ref_energy", torch.int64), ("err_peak", torch.int32),
                             ("energy", torch.int64), ("peak", torch.int32))}
        got = {}

        def fidelity():
            binding.fidelity(ref_list, hop, err_energy=out["err_energy"], ref_energy=out["ref_energy"],
                             err_peak=out["err_peak"])

        def envelope():
            binding.envelope(hop, energy=out["energy"], peak=out["peak"])

        def decode():
            x, _ = binding.decode_crops(crops, row_len)  # [streams * rows, row_len, ch], zero past a stream's end
            x = x.view(len(streams), rows * row_len, ch)[:, :n].to(torch.int32)
            r = torch.nn.functional.pad(refs.to(torch.int32), (0, 0, 0, nb * hop - R)).view(total, hop * ch)
            d = torch.nn.functional.pad(x, (0, 0, 0, nb * hop - n)).view(total, hop * ch).sub_(r)
            got["err_peak"] = d.abs().amax(dim=1)
            got["err_energy"] = d.to(torch.int64).square_().sum(dim=1)
            got["ref_energy"] = r.square_().sum(dim=1, dtype=torch.int64)

        paths = (("decode", decode), ("fidelity", fidelity), ("envelope", envelope))
        t = {name: ([], [], []) for name, _ in paths}
        for i in range(args.warmup + args.steps):
            for name, fn in paths:
                res = clocked(fn)
                if i >= args.warmup:
                    for k, v in enumerate(res):
                        t[name][k].append(v)
        equal = bool(torch.equal(got["err_energy"], out["err_energy"]) and
                     torch.equal(got["ref_energy"], out["ref_energy"]) and
                     torch.equal(got["err_peak"].to(torch.int32), out["err_peak"]))
        err, ref = int(out["err_energy"].sum()), int(out["ref_energy"].sum())
        row = {"streams": len(streams), "samples": n, "reference_samples": R, "channels": ch, "hop": hop,
               "blocks": total, "decode_rows": rows * len(streams), "decode_row_samples": row_len,
               "outputs_equal": equal, "snr_db": round(10 * np.log10(ref / err), 3) if err and ref else None}
        for name, _ in paths:
            row[f"{name}_device_ms"] = stats(t[name][0])
            row[f"{name}_wall_ms"] = stats(t[name][1])
            row[f"{name}_peak_bytes"] = int(max(t[name][2]))
        row["device_ratio_to_decode"] = round(row["fidelity_device_ms"][0] / row["decode_device_ms"][0], 3)
        row["device_ratio_to_envelope"] = round(row["fidelity_device_ms"][0] / row["envelope_device_ms"][0], 3)
        binding.close()
        return row, equal

    st = sc.Decoder.open(gsc)
    dev = torch.device("cuda", st.device)
    assert len(pcm) <= st.samples_per_channel
    head, ok = measure([st], st.sample_rate, torch.from_numpy(pcm).to(dev).unsqueeze(0))
    st.close()
    small = (ROOT / "tests" / "golden" / "syn2s_c2_cs8_cpf4096.gsc").read_bytes()
    ss = sc.Decoder.open_many([small] * args.set_streams)
    gen = torch.Generator(device=dev).manual_seed(5)
    refs = torch.randint(-32768, 32768, (args.set_streams, ss[0].samples_per_channel, ss[0].channels), device=dev,
                         generator=gen, dtype=torch.int32).to(torch.int16)
    ragged, ok2 = measure(ss.streams, ss[0].samples_per_channel, refs)
    ss.close()

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = {"bench": "fidelity", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
           "commit": commit, "gsc_bytes": len(gsc), "steps": args.steps, "warmup": args.warmup,
           "times": "[median, min, max] ms", "headline": head, "set": ragged}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    if not (ok and ok2):
        print("bench_fidelity: the fidelity call and the decoded reduction differ", file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
