"""Open benchmark: `Decoder.open(gsc)` (the host walk) against
`Decoder.open(gsc, table)` (a seek table checked on the device), and
`decode(gsc)` against `decode(gsc, table=t)`, on the C2 stream of
tools/bench_decode.py (-cs8 -cpf4096 -cbd8, 44.1 kHz stereo synthetic).

  python tools/bench_decode_open.py [--seconds 1024] [--steps 10] [--warmup 3] [--gsc FILE] [--out FILE]

The .gsc and its table are produced once outside the timed region (the
table by the encoder's packer; it is compared with `Index(gsc).table()`).  In
one session the two ways alternate, walk then table, step by step; the figures
are medians with min and max over the steps of the Python wall time and of
`gsc_last_open_timing`'s stages.  Outputs are compared after the clock
stops.  Prints one JSON line.
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


def _stats(rows):
    keys = [k for k in rows[0] if k.endswith("_ms")]
    return ({k: round(statistics.median(r[k] for r in rows), 3) for k in keys},
            {k: [round(min(r[k] for r in rows), 3), round(max(r[k] for r in rows), 3)] for k in keys})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1024.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gsc", default=None, help="cache file of the encoded stream; its table goes to FILE.gsct")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()

    import numpy as np

    import soundchunks_amd as sc
    from soundchunks_amd.synth import synth_wav

    argv = ["-cs8", "-cpf4096", "-cbd8"]
    cache = Path(args.gsc) if args.gsc else None
    tcache = Path(str(cache) + "t") if cache else None
    if cache and cache.exists() and tcache.exists():
        gsc, table = cache.read_bytes(), tcache.read_bytes()
    else:
        gsc, table = sc.Encoder(argv).encode(synth_wav(args.seconds, 44100, 2), with_table=True)
        if cache:
            cache.parent.mkdir(parents=True, exist_ok=True)
            cache.write_bytes(gsc)
            tcache.write_bytes(table)
    dec = sc.Decoder()

    rows = {"open_walk": [], "open_table": [], "decode_walk": [], "decode_table": []}
    probes = []
    ranges = None
    for i in range(args.warmup + args.steps):
        for how, tb in (("open_walk", None), ("open_table", table)):
            t0 = time.perf_counter()
            st = dec.open(gsc, table=tb)
            wall = (time.perf_counter() - t0) * 1e3
            t = dec.last_open_timing()
            t["python_wall_ms"] = wall
            if ranges is None:
                n = st.samples_per_channel
                edge = int(st.index.first_sample[1]) if st.frame_count > 1 else n // 2
                ranges = [(0, 4096), (edge - 2048, edge + 2048), (n - 4096, n)]
            if i == 0:
                probes.append([st.decode_samples(a, b) for a, b in ranges])
                probes.append(st.index)
            st.close()
            if i >= args.warmup:
                rows[how].append(t)
    pcms = {}
    for i in range(args.warmup + args.steps):
        for how, tb in (("decode_walk", None), ("decode_table", table)):
            t0 = time.perf_counter()
            pcm, _ = dec.decode(gsc, table=tb)
            wall = (time.perf_counter() - t0) * 1e3
            pcms[how] = pcm
            if i >= args.warmup:
                rows[how].append({"python_wall_ms": wall})
    # after the clock: the same table, the same index, the same samples
    walked = dec.index(gsc)
    assert table == walked.table(), "the encoder's table differs from the walk's"
    for a, b in zip(probes[0], probes[2]):
        assert np.array_equal(a, b), "resident streams differ"
    for f in ("byte_offset", "first_sample", "frame_length", "chunk_size", "chunk_count"):
        assert np.array_equal(getattr(probes[1], f), getattr(probes[3], f)), f
    assert np.array_equal(pcms["decode_walk"], pcms["decode_table"]), "decoded PCM differs"

    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"bench": "decode_open", "config": "c2 -cs8 -cpf4096 -cbd8 44.1 kHz stereo", "seconds": args.seconds,
           "commit": commit, "checkpoint_symbols": dec.checkpoint_symbols(), "gsc_bytes": len(gsc),
           "table_bytes": len(table), "frames": walked.frame_count, "steps": args.steps, "warmup": args.warmup,
           "uploaded_bytes": rows["open_table"][0]["uploaded_bytes"], "checkpoints": rows["open_table"][0]["checkpoints"]}
    for how, r in rows.items():
        med, spread = _stats(r)
        res[how] = {"median_ms": med, "min_max_ms": spread}
    res["open_speedup"] = round(res["open_walk"]["median_ms"]["python_wall_ms"] /
                                res["open_table"]["median_ms"]["python_wall_ms"], 2)
    res["decode_speedup"] = round(res["decode_walk"]["median_ms"]["python_wall_ms"] /
                                  res["decode_table"]["median_ms"]["python_wall_ms"], 2)
    res["outputs_equal"] = True
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
