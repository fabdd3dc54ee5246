"""Which render_k instance and which approach kernel a launch runs (csrc/vp_dispatch.h), pinned for every request the API admits.

The output tests cannot see a wrong choice: an ACH, CANCEL or LDSB instance picked wrongly computes the same bits and only costs
speed or occupancy, and an instance missing from one build is an abort() in somebody's A/B run.  So the choice is tabulated by
render_variants_probe.cpp THROUGH the real launcher -- host stand-ins for the kernels, no HIP runtime, no device -- in the four
builds (exact or fast arithmetic, full or development) and compared with tests/golden/render_variants.txt (its head
explains the cells).

The fixture was recorded from the hand-written launchers that vp_dispatch.h replaced (the same probe around their text, abort()
turned into the probe's throw), not from vp_dispatch.h: a row that changes is a change of behaviour.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

BUILDS = {
    "exact full": [],
    "exact dev": ["-DVP_DEV_BUILD"],
    "fast full": ["-DVP_ARITH_FAST"],
    "fast dev": ["-DVP_ARITH_FAST", "-DVP_DEV_BUILD"],
}


def _golden():
    tables, name = {}, None
    for line in open(os.path.join(HERE, "golden", "render_variants.txt")).read().splitlines():
        if line.startswith("##"):
            continue
        if line.startswith("# "):
            name = line[2:]
            tables[name] = []
        else:
            tables[name].append(line)
    return tables


GOLDEN = _golden()


def _cells(rows, kinds):
    # (a line with lds=* stands for three)
    return [c for r in rows if r.split()[0] in kinds for c in r.split(": ")[1].split() * (3 if "lds=*" in r else 1)]


def _selected(rows, kinds):
    return {c.split(":")[0].split("@")[0] for c in _cells(rows, kinds) if c not in ("-", ".")}


@pytest.mark.parametrize("build", list(BUILDS))
def test_every_admitted_request_runs_the_instance_it_ran_before(build, tmp_path):
    exe = str(tmp_path / "probe")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-std=c++17", "-I" + os.path.join(ROOT, "cuda-volpath_amd", "csrc")] + BUILDS[build]
                          + [os.path.join(HERE, "render_variants_probe.cpp"), "-o", exe])
    got = subprocess.check_output([exe], text=True).splitlines()
    want = GOLDEN[build]
    changed = [(w, g) for w, g in zip(want, got) if w != g]
    assert not changed, f"{len(changed)} lines changed, the first: {changed[0]}"
    assert len(got) == len(want)


def test_the_fixture_covers_the_domain_and_the_kernel_set():
    # exact mode: 1512 render requests, 36 light-class requests, 72 approach requests; fast mode: 144 and 32 (no light class of its own)
    for build, requests, not_built in (("exact full", 1512 + 36 + 72, 0), ("exact dev", 1512 + 18 + 72, 1426), ("fast full", 144 + 32, 0), ("fast dev", 144 + 32, 104)):
        assert GOLDEN[build][-1] == f"requests {requests}, not built {not_built}"
    admitted = lambda build, kind: sum(c != "." for c in _cells(GOLDEN[build][:-1], {kind}))
    assert [admitted("exact full", k) for k in ("render", "light", "approach")] == [1512, 36, 72]
    assert [admitted("fast full", k) for k in ("render", "light", "approach")] == [144, 0, 32]
    # the distinct instances the admitted requests select are the render_k kernels of each object: 292 + 30 of the exact full build's
    # 322, all 60 and 28 of the fast builds'.  (The development build compiles 52: these 48, and the four float-table light instances
    # of the decomposition estimator, which only a float volume -- outside what that build admits -- selects.)
    assert len(_selected(GOLDEN["exact full"][:-1], {"render"})) == 292
    assert len(_selected(GOLDEN["exact full"][:-1], {"render", "light"})) == 322
    assert len(_selected(GOLDEN["exact dev"][:-1], {"render", "light"})) == 48
    assert len(_selected(GOLDEN["fast full"][:-1], {"render"})) == 60
    assert len(_selected(GOLDEN["fast dev"][:-1], {"render"})) == 28
    # ... and the approach kernels: 12 + approach_segments_k = the exact builds' 13; 8 and 6
    assert [len(_selected(GOLDEN[b][:-1], {"approach"})) for b in BUILDS] == [12, 12, 8, 6]
