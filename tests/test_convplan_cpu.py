"""The 16-bit conv planner against the launch checks and the list of built kernels, on the host: tests/host/convplan_main.cpp is compiled
with the host compiler together with csrc/convplan.hip (as C++), csrc/convgeom.h and csrc/convvariants.h, and run as a stand-alone program;
nothing is loaded into this process.

This side writes the layer list -- every dense conv of YOLO11 n and s at 416 x 416, 128 x 128 and the shapes of
forward_obs.SHAPE_TABLE, with what the plan builder may fuse around it -- and compares the program's records (tiling, stages, LDS
layout, tiles per workgroup, grid, buffer ranges, kernel variant, SHA-256 of the packed weights) with tests/golden/convplan.json, recorded
when the host half was split out of conv.hip and before any formula was shared.  The file keeps, per model scale and tile shape and per
form, the number of records and the SHA-256 of their text (`digest`); a mismatch names the shape and the form, and the program's full
records of both trees can then be compared by hand.  `python tests/test_convplan_cpu.py --record` rewrites the file."""
import hashlib
import functools
import json
import os
import re
import shutil
import subprocess
import sys
from unittest import mock

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "convplan_main.cpp")
CSRC = os.path.join(ROOT, "oriented-object-detection_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "convplan.json")


def _rocm_include():
    for r in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h")):
            return os.path.join(r, "include")
    raise RuntimeError("hip/hip_runtime.h not found (ROCM_PATH)")


def layer_lines():
    """One line per distinct dense conv (the id names its first occurrence): see convplan_main.cpp for the columns."""
    import train_shapes
    from forward_obs import SHAPE_TABLE

    sizes = [(416, 416), (128, 128)] + [(h, w) for h, w, _ in SHAPE_TABLE]
    seen, lines = set(), []
    # (conv_layers builds the oracle model on every call, most of a second each: one model per scale serves all twelve sizes)
    with mock.patch.object(train_shapes, "Yolo11OBB", functools.lru_cache(None)(train_shapes.Yolo11OBB)):
        per_size = [(scale, h, w, train_shapes.conv_layers(scale, h, w)) for scale in ("n", "s") for h, w in sizes]
    for scale, h, w, layers in per_size:
        c2_of = {name: c2 for name, _, _, _, _, c2, _, _ in layers}
        for name, k, s, g, c1, c2, H, W in layers:
            if g != 1:
                continue
            Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if s == 2 else (H, W)
            # the skip member of the two [Upsample | skip] concats (model.6 / model.4 outputs)
            skip = {"model.13.cv1": c2_of["model.6.cv2"], "model.16.cv1": c2_of["model.4.cv2"]}.get(name, 0)
            tail = None  # the plain 1x1 into the head rows behind the last Conv of a head branch
            if re.fullmatch(r"model\.23\.cv[24]\.\d\.1", name):
                tail = name[:-1] + "2"
            if re.fullmatch(r"model\.23\.cv3\.\d\.1\.1", name):
                tail = name[:-3] + "2"
            t16 = {"model.1": "model.2.cv1", "model.3": "model.4.cv1", "model.5": "model.6.cv1", "model.7": "model.8.cv1"}.get(name)  # cv1 of the C3k2 block behind a stride-2 conv
            head = int(bool(re.fullmatch(r"model\.23\.cv[234]\.\d\.2", name)))
            m = re.fullmatch(r"model\.23\.cv2\.(\d)\.0", name)  # first convs of the box and angle branches read the same map
            merge = c2_of[f"model.23.cv4.{m.group(1)}.0"] if m else 0
            cols = (k, s, c1, c2, H, W, Ho, Wo, int(name == "model.0"), skip, c2_of[tail] if tail else 0, c2_of[t16] if t16 else 0, head, merge)
            if cols not in seen:
                seen.add(cols)
                lines.append(" ".join([f"{scale}:{h}x{w}:{name}"] + [str(c) for c in cols]))
    return lines


def digest(records):
    """{"<scale>:<h>x<w>": {"<form>": [records, sha256 of their lines `id [fields]`, sorted by id]}}; ids are `<scale>:<h>x<w>:<layer>|<form>`."""
    groups = {}
    for rid in sorted(records):
        shape, form = rid.rsplit(":", 1)[0], rid.rsplit("|", 1)[1]
        groups.setdefault(shape, {}).setdefault(form, []).append(rid + " " + json.dumps(records[rid], separators=(",", ":")))
    return {shape: {form: [len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()] for form, v in forms.items()} for shape, forms in groups.items()}


def run_program(tmp):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe, lst, rec = (os.path.join(tmp, n) for n in ("convplan_main", "layers.txt", "records.json"))
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + CSRC, SRC, "-x", "c++", os.path.join(CSRC, "convplan.hip"), "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    with open(lst, "w") as f:
        f.write("\n".join(layer_lines()) + "\n")
    p = subprocess.run([exe, lst, rec], capture_output=True, text=True, timeout=300)
    records = json.load(open(rec)) if os.path.exists(rec) else None
    return p, records


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    return run_program(str(tmp_path_factory.mktemp("convplan")))


def test_planned_launches_pass_the_launch_checks(result):
    """(a) + (c): every planned launch is accepted with a kernel variant of the list, within that row's LDS cap, the staging cap of its form
    and the fragment capacity of its tile; the refused stay refused."""
    p, _ = result
    assert p.returncode == 0, p.stdout + p.stderr
    assert "convplan ok" in p.stdout


def test_records_match_the_split(result):
    """(b): tiling, LDS layout, grid, buffer ranges, kernel variant and packed-weight hash of every launch, as recorded before the geometry was shared."""
    _, records = result
    golden = json.load(open(GOLDEN))
    assert records is not None
    got = digest(records)
    assert sorted(got) == sorted(golden)
    bad = [(shape, form) for shape in golden for form in sorted(set(golden[shape]) | set(got[shape])) if got[shape].get(form) != golden[shape].get(form)]
    assert not bad, f"records of {len(bad)} (shape, form) groups differ from the recorded ones: {bad[:8]}"


if __name__ == "__main__":
    import tempfile

    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    with tempfile.TemporaryDirectory() as tmp:
        p, records = run_program(tmp)
        sys.stdout.write(p.stdout + p.stderr)
        if "--record" in sys.argv and records is not None:
            with open(GOLDEN, "w") as f:
                f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in digest(records).items()) + "\n}\n")
            print("wrote", GOLDEN, len(records), "records")
        sys.exit(p.returncode)
