"""phant_amd/csrc/staging.h -- the layout, the input stager and the output list that block_receipts, header_chain, block_transactions
and block_txs_prestate share -- driven alone by tests/native/call_staging_main.cpp over the emulated runtime: synthetic calls in all
three forms with zero-byte, NULL and unwanted arrays at the first, a middle and the last position, no output wanted at all, spans that
end exactly at the pinned stage's size and one byte beyond, an arena that grows between two calls and an output delivered after the
control words were read; every delivered byte is compared with what was put in and every copy and synchronisation is counted.  Built
twice: under AddressSanitizer + UBSan the arena poisons its padding (the helper must never stage, and a copy that touched padding would
stop the program), under UBSan alone the stage is used.  No GPU and no Python-loaded library is involved."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize, poisons", [("address,undefined", 1), ("undefined", 0)])
def test_the_helper_alone_under_sanitizers(tmp_path, sanitize, poisons):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "call_staging"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
           "-I", os.path.join(ROOT, "tests", "native", "shim"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "call_staging_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    calls, staged_in, staged_out, got_poisons = map(int, re.fullmatch(r"(\d+) calls, (\d+) staged in, (\d+) staged out, poisons (\d)\n", r.stdout).groups())
    assert got_poisons == poisons and calls > 50
    assert (staged_in, staged_out) == (0, 0) if poisons else (staged_in > 25 and staged_out > 25)
