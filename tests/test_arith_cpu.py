"""The arithmetic-mode switch (include/volpath.h vp_set_arithmetic) without a GPU: constants, argument checks, the CLI flag."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cuda-volpath_amd", "volpath_render")


def _header():
    return open(os.path.join(ROOT, "include", "volpath.h")).read()


def test_constants_match_header():
    import volpath
    text = _header()
    m = re.search(r"enum\s*\{\s*VP_ARITH_EXACT\s*=\s*(\d+)\s*,\s*VP_ARITH_FAST\s*=\s*(\d+)\s*\}", text)
    assert m, "VP_ARITH_* enum missing from include/volpath.h"
    assert (volpath.ARITH_EXACT, volpath.ARITH_FAST) == (int(m.group(1)), int(m.group(2)))
    tol = re.search(r"#define\s+VP_ARITH_FAST_REL_L2\s+([0-9.eE+-]+)", text)
    assert tol and float(tol.group(1)) == volpath.ARITH_FAST_REL_L2
    assert 0.0 < volpath.ARITH_FAST_REL_L2 < 0.1
    assert {"vp_set_arithmetic", "vp_last_arithmetic"} <= set(volpath.PART2_SYMBOLS)


@pytest.mark.parametrize("mode", [2, -1, 7])
def test_bad_mode_is_refused_before_the_device(mode):
    import volpath
    with pytest.raises(volpath.VolpathError, match="arithmetic"):
        volpath.set_arithmetic(mode)
    assert volpath.lib().vp_set_arithmetic(mode) == -3   # VP_E_ARG


def test_cli_arith_flag():
    r = subprocess.run([EXE, "--arith", "bogus"], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--arith" in r.stdout
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--arith exact|fast" in r.stdout
    # the fast mode needs a counter-based stream: refused before any device is touched
    r = subprocess.run([EXE, "--arith", "fast", "--rng", "samplerh"], capture_output=True, text=True)
    assert r.returncode == 2 and "--arith fast" in r.stderr


@pytest.mark.parametrize("which,n", [(-1, 4), (12, 4), (99, 4), (0, -1), (7, -5)])
def test_test_math_refuses_bad_arguments_before_the_device(which, n):
    """vp_test_math: `which` outside 0..11 (include/volpath.h) and n < 0 are VP_E_ARG before any device is touched -- an unknown code
    no longer runs some helper silently"""
    import volpath
    assert volpath.lib().vp_test_math(which, None, None, n) == -3   # VP_E_ARG
    assert "vp_test_math" in volpath.lib().vp_last_error().decode()
    if n >= 0:
        import numpy as np
        with pytest.raises(volpath.VolpathError, match="vp_test_math"):
            volpath.test_math(which, np.ones(n, np.float32))
