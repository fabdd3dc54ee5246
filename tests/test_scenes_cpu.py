"""The shared random-scene generator (tests/scenes.py random_case) without a GPU: every seed still gives the scene it gave when the
generator lived in test_fuzz_gpu.py -- the digests in tests/golden/random_case_digests.json were recorded from that version."""
import hashlib
import json
import os

import numpy as np

import scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_case_digests.json")


def _digest(case):
    h = hashlib.sha256()
    for k in sorted(case):
        v = case[k]
        h.update(k.encode())
        if isinstance(v, np.ndarray):
            h.update(f"{v.dtype.str}{v.shape}".encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


def test_random_case_is_unchanged_for_seeds_0_to_63():
    from volpath import host
    want = json.load(open(GOLDEN))
    assert sorted(int(s) for s in want) == list(range(64))
    got = {str(s): _digest(scenes.random_case(s, host)) for s in range(64)}
    assert [s for s in want if got[s] != want[s]] == []
