"""The instance table of tests/test_filter_instances_gpu.py is held to the source: every hipLaunchKernelGGL site of csrc/vp_denoise.hip,
with its kernel and its explicit template arguments, expanded over the values its launchers hand down, is exactly one row.  An
instance added to a launcher without a row in the table -- and so without a GPU run against the restatement -- fails here."""
import os
import re

import test_filter_instances_gpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "cuda-volpath_amd", "csrc", "vp_denoise.hip")
# the launch sites as they are written: (kernel, explicit template arguments).  F is launch_guided_tiled's own parameter and V... the
# pack that is empty for vp_denoise / vp_denoise_guided and the one plane for vp_denoise_var
SITES = sorted(
    [("denoise_guided_tiled_k", "F, %d, V..." % nf) for nf in (1, 2, 3, 4)]
    + [("denoise_tiled_k", "%d, V..." % f) for f in (0, 1, 2, 3)]
    + [("denoise_plain_k", "V..."), ("denoise_guided_plain_k", "V...")]
    + [("variance_tiled_k", "%d" % f) for f in (0, 1, 2, 3)]
    + [("variance_plain_k", ""), ("select_tiled_k", ""), ("select_plain_k", "")])


def launch_sites(text):
    found = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)\s*(?:<([^>]*)>)?", text)
    assert len(found) == text.count("hipLaunchKernelGGL")
    return sorted((k, " ".join(a.split())) for k, a in found)


def test_the_launch_sites_are_the_tables_rows():
    text = open(SOURCE).read()
    assert launch_sites(text) == SITES
    # what the launchers hand down: launch_guided_tiled<F> for these F, and the two packs of each _v launcher (a call ends in `svar)` or not)
    guided_patches = sorted(int(f) for f in re.findall(r"\blaunch_guided_tiled<(\d+)>\(", text))
    assert guided_patches == [0, 1, 2, 3]
    for launcher in ("launch_denoise_v", "launch_denoise_guided_v"):
        calls = re.findall(r"\b%s\(([^;{]*)\);" % launcher, text)
        assert sorted(c.rstrip().endswith("svar") for c in calls) == [False, True], (launcher, calls)
    rows = set()
    for kernel, args in SITES:
        packs = (False, True) if "V..." in args else (False,)
        ints = [a.strip() for a in args.split(",") if a.strip() and a.strip() != "V..."]
        for f in (guided_patches if "F" in ints else [None]):
            targs = tuple(f if a == "F" else int(a) for a in ints)
            rows.update((kernel, targs, plane) for plane in packs)
    table = [(kernel, targs, plane) for _, kernel, targs, plane in T.INSTANCES] + list(T.PLAIN_INSTANCES)
    assert len(table) == len(set(table)) == 8 + 32 + 4 + 1 + 6
    assert set(table) == rows
    # every tiled row is a test case, and the call of a row is the one that reaches its kernel
    assert sorted(T.COLOUR_ROWS + T.VARIANCE_ROWS) == sorted(r for r in T.INSTANCES if r[1] != "select_tiled_k")
    for call, kernel, targs, plane in T.INSTANCES:
        assert plane == (call == "vp_denoise_var") and (len(targs) == 2) == (kernel == "denoise_guided_tiled_k")
    # the census of the summary: what the older tests reached is inside the table
    for (kernel, plane), reached in T.BEFORE.items():
        assert reached <= {targs for _, k, targs, p in T.INSTANCES if k == kernel and p == plane}


def test_a_site_without_a_row_is_noticed():
    """the parser sees an instance that a launcher gains"""
    text = open(SOURCE).read()
    more = text.replace("    default: hipLaunchKernelGGL(variance_tiled_k<3>,",
                        "    case 3: hipLaunchKernelGGL(variance_tiled_k<3>, grid, block, lds, st, dst, u, q, W, H, R, k2); break;\n"
                        "    default: hipLaunchKernelGGL(variance_tiled_k<4>,")
    assert more != text and launch_sites(more) != SITES and ("variance_tiled_k", "4") in launch_sites(more)
