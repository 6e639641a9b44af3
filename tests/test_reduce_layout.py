"""The Reduce batch's slab layout (csrc/gsc_reduce_layout.h), checked on the host."""
from __future__ import annotations

import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_reduce_layout_check_under_sanitizers():
    """make reduce_layout_check: gsc::reduce_layout for 1 to 3 frames, equal and
    mixed K, built with -fsanitize=address,undefined as a stand-alone program:
    every region inside the slab totals, none overlapping, and the offsets the
    four call sites used to write out by hand."""
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "soundchunks_amd" / "csrc"), "reduce_layout_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("frames ")]
    assert len(lines) == 3 and "FAIL" not in r.stdout, r.stdout[-2000:]
