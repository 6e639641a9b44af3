"""Corpus open benchmark: N streams opened as one set (`Decoder.open_many`)
against the loop of `Decoder.open(gsc, table=t)`, on two workloads:

  corpus     the 22 lame_test files, encoded once as a batch at -cs8 -cpf4096
  synthetic  1024 streams of about 2 s each, cut from the synthetic signal, at
             -cs8 -cpf256

  python tools/bench_decode_open_many.py [--workload corpus|synthetic|both] [--streams 1024]
         [--stream-seconds 2] [--steps 10] [--warmup 3] [--cache DIR] [--commit NAME] [--out FILE]

The streams and their tables come from the batch encoder
(`encode_files(with_tables=True)`) outside the timed region.  In one session
the two ways alternate, set then loop, step by step; the figures are medians
with min and max over the steps of the Python wall time of the open alone
(closing is outside the clock), and of `gsc_last_set_open_timing`'s stages and
call counts.  The set counts as faster when the two [min, max] ranges do not
overlap.  After the clock stops, members and the loop's streams are compared
with the whole-frame decode of the same bytes: "outputs_equal", and every
differing probe with its side in "outputs_differing"; a difference exits with
status 3.  Prints one JSON line per workload.
"""
from __future__ import annotations

import argparse
import json
import pickle
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _spread(vals):
    return {"median": round(statistics.median(vals), 3), "min_max": [round(min(vals), 3), round(max(vals), 3)]}


def _encode_batch(sc, argv, wavs):
    p = sc.Encoder(argv).prepare_many(wavs)
    try:
        blob, sizes, tables = p.encode_files(with_tables=True)
    finally:
        p.close()
    files, o = [], 0
    for n in sizes:
        files.append(blob[o:o + n])
        o += n
    return files, tables


def _workload(sc, name, args):
    cache = Path(args.cache) / f"open_many_{name}_{args.streams}x{args.stream_seconds}.pkl" if args.cache else None
    if cache and cache.exists():
        return pickle.loads(cache.read_bytes())
    if name == "corpus":
        argv = ["-cs8", "-cpf4096"]
        wavs = [p.read_bytes() for p in sorted((ROOT / "tests" / "golden" / "lame_test").glob("*.wav"))]
        what = f"{len(wavs)} lame_test files, {' '.join(argv)}"
    else:
        from soundchunks_amd.decoder import wav_header
        from soundchunks_amd.synth import synth_pcm

        argv = ["-cs8", "-cpf256"]
        per = int(args.stream_seconds * 44100)
        pcm = synth_pcm(args.streams * args.stream_seconds, 44100, 2)
        wavs = []
        for i in range(args.streams):
            data = pcm[i * per:(i + 1) * per].astype("<i2", copy=False).tobytes()
            wavs.append(wav_header(2, 44100, len(data)) + data)
        what = f"{args.streams} streams of {args.stream_seconds} s cut from the synthetic signal, {' '.join(argv)}"
    files, tables = _encode_batch(sc, argv, wavs)
    res = (what, files, tables)
    if cache:
        cache.parent.mkdir(parents=True, exist_ok=True)
        cache.write_bytes(pickle.dumps(res))
    return res


def _run(sc, name, args):
    import numpy as np

    what, files, tables = _workload(sc, name, args)
    dec = sc.Decoder
    walls = {"set": [], "loop": []}
    stages = []
    probe = range(len(files))  # every member, both kinds, at its first and last samples
    differing = []  # [side, member, begin, end] of every probe that is not the whole-frame decode's
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        ss = dec.open_many(files, tables)
        w_set = (time.perf_counter() - t0) * 1e3
        tim = dec.last_set_open_timing()
        t0 = time.perf_counter()
        rs = [dec.open(g, table=t) for g, t in zip(files, tables)]
        w_loop = (time.perf_counter() - t0) * 1e3
        if i == 0:  # after the clock: the same samples either way, and the whole-frame decode's
            for k in probe:
                m = rs[k].samples_per_channel
                n = min(4096, m)
                ref = sc.Decoder().decode(files[k])[0]
                for a, b in ((0, n), (m - n, m)):
                    for side, st in (("set", ss[k]), ("loop", rs[k])):
                        if not np.array_equal(st.decode_samples(a, b), ref[a:b]):
                            differing.append([side, k, a, b])
        ss.close()
        for r in rs:
            r.close()
        if i >= args.warmup:
            walls["set"].append(w_set)
            walls["loop"].append(w_loop)
            stages.append(tim)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = {"bench": "decode_open_many", "workload": name, "config": what, "commit": commit, "steps": args.steps,
           "warmup": args.warmup, "streams": len(files), "gsc_bytes": sum(len(g) for g in files),
           "table_bytes": sum(len(t) for t in tables), "set_wall_ms": _spread(walls["set"]),
           "loop_wall_ms": _spread(walls["loop"])}
    res["set_stages_ms"] = {k: _spread([s[k] for s in stages]) for k in stages[0] if k.endswith("_ms")}
    res["set_counts"] = {k: stages[-1][k] for k in stages[-1] if not k.endswith("_ms")}
    res["loop_per_stream_ms"] = round(res["loop_wall_ms"]["median"] / len(files), 4)
    res["set_per_stream_ms"] = round(res["set_wall_ms"]["median"] / len(files), 4)
    res["ratio_of_medians"] = round(res["loop_wall_ms"]["median"] / res["set_wall_ms"]["median"], 2)
    res["set_faster"] = res["set_wall_ms"]["min_max"][1] < res["loop_wall_ms"]["min_max"][0]
    res["loop_faster"] = res["loop_wall_ms"]["min_max"][1] < res["set_wall_ms"]["min_max"][0]
    res["outputs_equal"] = not differing
    res["outputs_differing"] = differing
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=("corpus", "synthetic", "both"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--stream-seconds", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cache", default=None, help="directory that keeps the encoded workloads between runs")
    ap.add_argument("--commit", default="", help="names the measured build where the tree has no git metadata")
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()

    import soundchunks_amd as sc

    lines, bad = [], False
    for name in (("corpus", "synthetic") if args.workload == "both" else (args.workload,)):
        res = _run(sc, name, args)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        bad = bad or not res["outputs_equal"]
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    if bad:
        sys.exit(3)


if __name__ == "__main__":
    main()
