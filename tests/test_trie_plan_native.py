"""phant_amd/csrc/trie_plan.h -- what the trie hasher's launcher chooses, as plain host C++: the knobs resolved once, the pass, the
min-tree's level sizes, leaves ahead or not, the scratch bound and every depth bin's launch -- driven alone by
tests/native/trie_plan_main.cpp, whose expected values are numbers written out there: the bins of 1, 512, 513, 1 024, 1 025, 2 048,
2 049, 4 096, 4 097, 65 535, 65 536 and 65 537 nodes (the crowded ones at 3c, 3c + 1, 6c and 6c + 1 children) under every knob that moves
a launch, the pass around 2 048 and 4 096 keys and a mean value of a rate block, the helper stream around 400 000 keys, the idle LDS's
clamp, leaves ahead around 8 Mi keys and with free memory one byte short of the tables, and the one scratch bound against the three sums
the driver used to carry.  Built with AddressSanitizer + UBSan as a stand-alone program.  No GPU and no Python-loaded library is
involved."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trie_plan_alone_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "trie_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unused-function",
           "-Wno-unused-parameter", "-I", os.path.join(ROOT, "tests", "native", "shim"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "trie_plan_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    checks = int(re.fullmatch(r"(\d+) checks\n", r.stdout).group(1))
    assert checks > 600  # (14 settings x 19 bins x 2, and the rest)
