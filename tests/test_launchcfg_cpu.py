"""csrc/launchcfg.h on the host: tests/host/launchcfg_main.cpp defines the HIP calls the header makes as recorders and asserts how
often each is reached (per device, per kernel, per size; failures not cached; 8 threads x 2 devices).  Compiled and run as a
stand-alone program, once plain and once under ThreadSanitizer; nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "launchcfg_main.cpp")
CSRC = os.path.join(ROOT, "oriented-object-detection_amd", "csrc")


def _rocm_include():
    for r in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h")):
            return os.path.join(r, "include")
    raise RuntimeError("hip/hip_runtime.h not found (ROCM_PATH)")


def _compile(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + CSRC, "-pthread", *extra, SRC, "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "launchcfg ok" in p.stdout


def test_launchcfg_plain(tmp_path):
    exe, c = _compile(tmp_path, "launchcfg_plain", [])
    assert c.returncode == 0, c.stderr
    _run(exe)


def test_launchcfg_tsan(tmp_path):
    exe, c = _compile(tmp_path, "launchcfg_tsan", ["-fsanitize=thread"])
    if c.returncode != 0 and ("tsan" in c.stderr.lower() or "sanitize" in c.stderr.lower()):
        pytest.skip("ThreadSanitizer runtime not available to the host compiler: " + c.stderr.strip().splitlines()[-1])
    assert c.returncode == 0, c.stderr
    _run(exe)
