"""The lane functions of phant_block_access_lists -- al::walk_tuple, walk_count, key_ok, load_key / same_key, slot_home and tuple_home of
phant_amd/csrc/access_lists.hip.h and the address functions of txstate.hip.h they build on, the routines the kernels run in every lane --
compiled for the host as a stand-alone program under AddressSanitizer + UBSan (tests/native/access_main.cpp) and held against the rows of
tests/access_ref.py: seeded blocks with repeats and joins, every header boundary, and every malformed span of
tests/test_gpu_access_lists.py, each span in an allocation of exactly its size.  No GPU and no Python-loaded library is involved."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import access_ref as R
from tests.test_gpu_access_lists import MALFORMED_SPANS, addr, entries, key, pool, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_of(spans, addresses=(), slot_first=None, slots=()):
    """a case of the corpus (tests/native/access_main.cpp states the layout): the inputs and the definition's answer"""
    o, t = R.define(spans, addresses, slot_first, slots)
    words = lambda xs: struct.pack("<%dI" % len(xs), *xs)  # noqa: E731
    return b"".join([
        words([len(spans), len(addresses), len(slots)]), b"".join(addresses), words(list(slot_first) if len(addresses) else [0]), b"".join(slots),
        b"".join(words([len(s)]) + bytes(s) for s in spans),
        words([t["n_tuples"], t["n_keys"], t["n_missing_accounts"], t["n_missing_slots"], t["first_malformed"]]),
        words(o["tuple_first"]), words(o["al_flags"]), words(o["warm_addresses"]), words(o["warm_keys"]),
        b"".join(o["address"]), words(o["key_first"]), words(o["account_row"]), words(o["tuple_same"]),
        b"".join(o["key"]), words(o["slot_row"]), words(o["key_same"])])


def test_walk_mix_and_compare_against_the_definition_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "access"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "access_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    w = pool()
    good = [R.encode([(addr(1), [key(1), key(2)]), (addr(2), [])]), R.encode([(addr(2), [key(2)])])]
    cases = [case_of([good[0], span, good[1]], **w) for span in MALFORMED_SPANS.values()]
    cases.append(case_of([s for span in MALFORMED_SPANS.values() for s in (good[1], span)] + [b""], **w))
    # spans cut at every length: whatever is left is walked to its last byte and not beyond
    whole = R.encode([(addr(3), [key(1)]), (addr(4), []), (addr(3), [key(5), key(1)])])
    cases.append(case_of([whole[:k] for k in range(len(whole) + 1)], **w))
    for nk in (0, 1, 2, 7, 8, 1985, 1986):
        cases.append(case_of([R.encode([(addr(2), [key(j % 50) for j in range(nk)]), (addr(5), [key(1)])]), b""], **w))
    rng = np.random.default_rng(17)
    for trial in range(60):
        spans = [R.encode(entries(int(rng.integers(0, 6)), int(rng.integers(0, 5)), seed=1000 * trial + i, accounts=12, keys=9)) if i % 4 else b""
                 for i in range(int(rng.integers(1, 9)))]
        tables = [{}, pool(12, 9, 3, seed=trial), witness([(addr(2), [key(1)])] * 3 + [(addr(4), [])])][trial % 3]
        cases.append(case_of(spans, **tables))
    p = tmp_path / "corpus.bin"
    p.write_bytes(b"".join(cases))
    r = subprocess.run([str(exe), str(p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
    got = [int(x) for x in re.findall(r"(\d+) (?:cases|tuples|keys|malformed|joined)", r.stdout)]
    assert got[0] == len(cases) and got[1] > 500 and got[2] > 4000 and got[3] >= 2 * len(MALFORMED_SPANS) and got[4] > 100, r.stdout
