"""CPU: csrc/workspace.h, the cursor every multi-piece device workspace is measured and carved with, through the stand-alone
driver of tests/host/workspace_driver.cpp -- built with g++ once plain and once with -fsanitize=address,undefined; nothing
from ROCm, no Python in the process.  The driver measures a dozen piece lists (counts of 0 and 1, elements of 1 to 16 bytes,
base alignment 16 and 256), carves each out of a heap block of exactly bytes() bytes at five misalignments and writes every
piece over its whole length."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "single-view-3d-reconstruction_amd", "csrc")
DRIVER = os.path.join(REPO, "tests", "host", "workspace_driver.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_cursor_measures_what_it_carves(tmp_path, variant):
    if variant == "sanitized":
        import torch
        if torch.cuda.is_available():
            pytest.skip("sanitizer builds run on the CPU machine only")
    exe = tmp_path / ("workspace_driver_" + variant)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if variant == "sanitized" else [])
    r = subprocess.run(cmd + ["-I", CSRC, DRIVER, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    assert r.stdout.split() == ["ok", "12", "60"]      # 12 piece lists, each carved at 5 misalignments
