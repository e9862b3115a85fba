"""The host-side checks of phant_block_fee_history -- phant_amd/csrc/feehist_check.h over the firsts rule of segment_checks.h -- and
wide_uint.h's mul_small, compiled as a stand-alone program under AddressSanitizer + UBSan (tests/native/feehist_check_main.cpp): a good
call with one thing wrong at a time, every array in an allocation of exactly its entries; the multiply and the division-free threshold
test against the compiler's 128-bit integers.  No GPU is involved, and nothing loaded into Python runs under a sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_checks_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "feehist_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "feehist_check_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    cases, refused, accepted = (int(x) for x in re.search(r"(\d+) cases: (\d+) refused, (\d+) accepted", r.stdout).groups())
    assert cases == refused + accepted and refused > 40 and accepted > 20, r.stdout
