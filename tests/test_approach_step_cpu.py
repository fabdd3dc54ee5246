"""The approach walks' free-flight step, without a GPU (profiles/experiments/approach_step.txt):

  - the integer identity behind logf_'s folded exponent (vp_math.h logf_chain_): with the bias taken off the constant,
    (int32)(ix + 0xc0cafb0c) >> 23 is ((ix + 0x004afb0c) >> 23) - 127 and the low 23 bits of the two sums are the same, for every
    pattern below 0xbf3504f4 -- every non-negative float, +inf and the positive NaNs, a superset of logf_'s domain.  Pinned at both
    ends: 0xbf3504f3 is the last pattern where it holds, 0xbf3504f4 the first where it does not;
  - scripts/approach_step_isa.py compiles the exact unit and reports, for the walk loops of approach_k, approach_local_k<..., true>
    and approach_local_tab_k on Philox2x32-7, fewer vector instructions per step than the parent's 46 / 49 / 49 (the figures of
    the parent's assembly under the script's own count, recorded in profiles/experiments/approach_step.txt)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD, NEW = 0x004AFB0C, 0xC0CAFB0C
LAST_GOOD, FIRST_BAD = 0xBF3504F3, 0xBF3504F4


def _old(ix):
    iy = (ix.astype(np.uint64) + OLD) & 0xFFFFFFFF
    return (iy >> 23).astype(np.int64) - 127, iy & 0x007FFFFF


def _new(ix):
    iy = ((ix.astype(np.uint64) + NEW) & 0xFFFFFFFF).astype(np.uint32)
    return (iy.view(np.int32) >> 23).astype(np.int64), iy.astype(np.uint64) & 0x007FFFFF   # (numpy's >> on int32 is arithmetic)


def _same(ix):
    (e0, m0), (e1, m1) = _old(ix), _new(ix)
    return (e0 == e1) & (m0 == m1)


def test_the_constants_differ_by_the_bias():
    assert (OLD - 0x3F800000) % 2 ** 32 == NEW
    assert (OLD - NEW) % 2 ** 23 == 0


def test_identity_on_every_exponent_and_the_mantissas_around_the_fold():
    mant = np.array([0, 1, 0x3504F3, 0x3504F4, 0x3504F5, 0x7FFFFE, 0x7FFFFF], np.uint32)
    ix = ((np.arange(256, dtype=np.uint32)[:, None] << 23) | mant[None, :]).ravel()
    assert ix.size == 256 * 7
    assert _same(ix).all(), [hex(int(v)) for v in ix[~_same(ix)]]
    # what the chain reads off: the unbiased exponent, one more where the mantissa field exceeds that of fl(sqrt 2)
    e, _ = _new(ix)
    want = (ix >> 23).astype(np.int64) - 127 + ((ix & 0x7FFFFF) >= 0x3504F4)
    assert np.array_equal(e, want)


def test_identity_on_random_patterns_of_the_stated_domain():
    rng = np.random.default_rng(20240523)
    ix = rng.integers(0, 0x7F800001, 2 ** 24, dtype=np.uint32)
    assert ix.max() < 0x7F800001
    ok = _same(ix)
    assert ok.all(), [hex(int(v)) for v in ix[~ok][:8]]


def test_the_identity_ends_where_the_comment_says():
    assert _same(np.array([LAST_GOOD], np.uint32)).all()
    assert not _same(np.array([FIRST_BAD], np.uint32)).any()
    # ... and holds on the whole stretch up to there that the other tests do not sample: the positive NaNs and a band below the end
    for lo, hi in ((0x7F800000, 0x80000000), (LAST_GOOD - 2 ** 20, LAST_GOOD + 1)):
        assert _same(np.arange(lo, hi, dtype=np.uint64).astype(np.uint32)).all()


def test_walk_loops_have_fewer_vector_instructions_than_the_parents():
    """the script's own run: the exact unit's development build (the bench workloads' kernels), parent figures from the record"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "approach_step_isa.py"), "--dev", "--exact-only", "--json"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    parent, new = out["parent"]["walks"], out["new"]["walks"]
    print("vector instructions per step, parent -> this build:", {k: (parent.get(k), new.get(k)) for k in new}, out["parent_source"])
    assert parent == {"approach_k": 46.0, "approach_local_k": 49.0, "approach_local_tab_k": 49.0}, parent
    # (the hand count that started this work had 46 / 48 for the parent: the script's count of a loop takes in every block of the
    # graph's component, one more instruction there; the bar is the lower of the two)
    by_hand = {"approach_k": 46, "approach_local_k": 48, "approach_local_tab_k": 48}
    for k in ("approach_k", "approach_local_k", "approach_local_tab_k"):
        assert new[k] is not None and new[k] < min(parent[k], by_hand[k]), (k, new[k], parent[k])
    # no kernel of the unit spills because of it, and the walks keep eight waves
    kernels = out["new"]["kernels"]["vp_kernels"]
    for name, (vinsts, vgpr, occupancy, scratch) in kernels.items():
        if name.startswith("approach_"):
            assert occupancy == 8 and scratch == 0, (name, vgpr, occupancy, scratch)
