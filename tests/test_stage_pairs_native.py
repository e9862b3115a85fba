"""phant_amd/csrc/staging.h's stage_pairs -- the one way in for a forest's sorted pairs in host memory, shared by the host forms of the
trie hasher and of its prover -- driven alone by tests/native/stage_pairs_main.cpp over the emulated runtime, with no kernel at all:
inputs that end exactly at the pinned stage's size, one byte beyond it and well beyond it (nine values of 1 MiB), no pairs with and
without offset tables, one trie without a segment table, several tries with empty ones among them, caller offset tables that do not
begin at 0, a caller's arrays appended behind the five.  Every staged byte and every rebased offset is read back, the copies are counted
(one when staged, one per non-empty array otherwise), operator new is counted around the call (the staged path makes none), and every
invalid input is given alone and in pairs.  Built twice: under AddressSanitizer + UBSan the arena poisons its padding (nothing may be
staged, and a copy that touched padding would stop the program), under UBSan alone the stage is used.  No GPU and no Python-loaded
library is involved."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize, poisons", [("address,undefined", 1), ("undefined", 0)])
def test_stage_pairs_alone_under_sanitizers(tmp_path, sanitize, poisons):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "stage_pairs"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
           "-I", os.path.join(ROOT, "tests", "native", "shim"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "stage_pairs_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    calls, staged, got_poisons = map(int, re.fullmatch(r"(\d+) calls, (\d+) staged, poisons (\d)\n", r.stdout).groups())
    assert got_poisons == poisons and calls > 30
    assert staged == 0 if poisons else staged >= 15
