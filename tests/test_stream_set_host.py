"""Stream sets, what needs no device: ``Decoder.open_many`` refuses malformed
arguments before any device call, and the set's host code (the layout of the
slabs, the tables expanded on demand, the per-file cut of a batch's table)
runs clean as a stand-alone program under the host sanitizers."""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

from golden.cases import HERE

ROOT = Path(__file__).resolve().parents[1]
GOLDENS = sorted(p.stem for p in HERE.glob("*.gsc"))


def test_open_many_argument_errors():
    import soundchunks_amd as sc

    gsc = (HERE / "tiny_passthrough_cs8.gsc").read_bytes()
    t = sc.Decoder.index(gsc).table()
    # none of these messages is the one a missing device gives: the arguments are refused first
    with pytest.raises(sc.GscError, match="open_many: 2 streams, 1 tables"):
        sc.Decoder.open_many([gsc, gsc], [t])
    with pytest.raises(sc.GscError, match="open_many: 1 streams, 0 tables"):
        sc.Decoder.open_many([gsc], [])
    with pytest.raises(sc.GscError, match="open_many: stream 1 is str, not bytes"):
        sc.Decoder.open_many([gsc, "a.gsc"])
    with pytest.raises(sc.GscError, match="open_many: stream 0 is NoneType, not bytes"):
        sc.Decoder.open_many([None, gsc], [t, t])
    with pytest.raises(sc.GscError, match="open_many: table 1 is int, not bytes"):
        sc.Decoder.open_many([gsc, gsc], [None, 7])
    with pytest.raises(sc.GscError, match="no streams"):
        sc.Decoder.open_many([])
    # what the host sees of a bad member is refused with its index, before a device is asked for
    with pytest.raises(sc.GscError, match="stream 1: gsc seek table"):
        sc.Decoder.open_many([gsc, gsc], [t, t[:-1]])
    with pytest.raises(sc.GscError, match="stream 0: gsc decode: frame"):
        sc.Decoder.open_many([gsc[:-2], gsc[:-2]], [None, t])


def test_set_needs_the_device_and_never_falls_back():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import soundchunks_amd as sc

    gsc = (HERE / "tiny_passthrough_cs8.gsc").read_bytes()
    with pytest.raises(sc.GscError, match="no HIP device|gfx950"):
        sc.Decoder.open_many([gsc])
    with pytest.raises(sc.GscError, match="no HIP device|gfx950"):
        sc.Decoder.open_many([gsc], [sc.Decoder.index(gsc).table()])


def test_set_check_under_sanitizers():
    """make set_check: set_layout, the rebased frame descriptors, the tables on
    demand and index_table_split on exact-size heap copies of every golden, in
    sets of 1, 2 and all, built with -fsanitize=address,undefined as a
    stand-alone program.  Nothing is loaded into Python."""
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "soundchunks_amd" / "csrc"), "set_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
    ok = [ln for ln in r.stdout.splitlines() if ln.endswith(": ok")]
    assert len(ok) == 2 * len(GOLDENS) + 2, r.stdout[-2000:]  # sets of 1, of 2 (one fewer), of all; split; refusals
