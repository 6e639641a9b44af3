"""Code objects of the batched scan's two instantiations per shape (CPU, no GPU).

Every ScanCfg that launch_scan dispatches must exist as a PLAIN and as a
general kernel, and the PLAIN one exists to free registers: at the benchmark
shape (D = 16, K = 4096) it must spill no more VGPRs and use no more scratch
than the general one.  Reads the resource metadata of the gfx950 code object
(llvm-readelf --notes) only; the kernels' argument list comes from the same
metadata (the product kernels take no experiment `opts`).
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
OBJ = ROOT / "soundchunks_amd" / "lib" / "gsc_scan.o"
LLVM = Path("/opt/rocm/lib/llvm/bin")

# (D, LOGK, SL, DR) of gsc_launch_scan_batch's dispatch table.  The split layout
# (32, 12, 8, 16) dispatches the general kernel alone: its PLAIN object spilled
# more than the general one and ran slower (profiles/scan_plain/kernel_resources.txt)
SHAPES = [(d, lk, sl, d) for d in (8, 16) for lk, sl in ((8, 1), (9, 1), (10, 2), (11, 4), (12, 8))] + \
         [(32, lk, sl, 32) for lk, sl in ((8, 1), (9, 1), (10, 2), (11, 4))]
SPLIT = (32, 12, 8, 16)


def _scan_kernels(tmp_path):
    fatbin, dev = tmp_path / "scan.fatbin", tmp_path / "scan_dev.o"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fatbin}", str(OBJ)], check=True,
                   cwd=tmp_path)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fatbin}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"], check=True, cwd=tmp_path)
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(dev)], check=True, capture_output=True,
                           text=True).stdout
    kernels, cur = [], {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "agpr_count" and cur:
            kernels.append(cur)
            cur = {}
        cur[k] = v
        if k == "value_kind" and not v.startswith("hidden_"):
            cur["explicit_args"] = cur.get("explicit_args", 0) + 1
    if cur:
        kernels.append(cur)
    out = {}
    for k in kernels:
        # scan_batch_kernel<ScanCfg<D, LOGK, SL, DR>, PLAIN>
        m = re.search(r"scan_batch_kernelINS_7ScanCfgILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEELb([01])E", k.get("name", ""))
        if m:
            d, lk, sl, dr, plain = map(int, m.groups())
            out[(d, lk, sl, dr), bool(plain)] = k
    return out


@pytest.mark.skipif(not OBJ.exists() or not (LLVM / "llvm-readelf").exists(),
                    reason="scan kernel object not built here")
def test_both_kinds_of_every_shape_and_plain_frees_registers(tmp_path):
    ks = _scan_kernels(tmp_path)
    for shape in SHAPES:
        for plain in (False, True):
            assert (shape, plain) in ks, ("missing instantiation", shape, "PLAIN" if plain else "general")
    assert (SPLIT, False) in ks and (SPLIT, True) not in ks
    assert len(ks) == 2 * len(SHAPES) + 1, sorted(ks)
    gen, pl = ks[(16, 12, 8, 16), False], ks[(16, 12, 8, 16), True]
    assert int(pl["vgpr_spill_count"]) <= int(gen["vgpr_spill_count"]), (pl, gen)
    assert int(pl["private_segment_fixed_size"]) <= int(gen["private_segment_fixed_size"]), (pl, gen)
    # no experiment switches in the product kernels: frames, nframes, X, C, scratch, rates, tol,
    # max_passes, tails -- and no `opts`
    for key, k in ks.items():
        assert k["explicit_args"] == 9, (key, k["explicit_args"])
