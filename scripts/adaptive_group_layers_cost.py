"""What the adaptive rounds on three planes (vp_render_adaptive_group_layers) cost against the uniform
vp_render_frames_group_layers_stats calls, what they return, and whether the feature cost the beauty render anything (development tool;
the bench is bench.py):

    python scripts/adaptive_group_layers_cost.py c2,c4f [--frames 256] [--round 32] [--repeat 3] [--parent-tree DIR] [--out FILE]
                                                        [--step-seconds 300]

A workload is a bench workload of volpath/scene.py at the bench's size.  Every GPU step runs in a child process of its own under a time
limit of its own (--step-seconds); the first step that fails, or runs into its limit, ends the script with a non-zero status, and the
steps that were not reached are listed as "not measured".  The steps, per workload:

  rounds   the cost of the rounds.  The adaptive call with tolerances 0 and min_frames above --frames (nothing can freeze: every round
           renders every pixel) alternates `repeat` times with the same frames sent through vp_render_frames_group_layers_stats in
           calls of --round frames.  Both queue the same render launches and the same reduces; the adaptive call adds, per round, one
           compaction of the pixel lists (three small kernels) and one read-back of three counts with a synchronisation, and it
           renders the compacted list, which lacks the per-view ray and segment tables of the cached lists.  Times are whole calls, a
           host clock from before the first call to after vp_synchronize; min / median / max over the repeats, and the spread of the
           alternation is the noise floor of the comparison.  Accumulators and records of the two are compared by hash.
  return   what the rounds return: rel_tol (0.05, 0.05, 0.05), the CLI's floors (1e-3 for sun and sky, 1e-2 for trans), min_frames 16,
           --round frames per round, --frames frames at most -- samples used of samples possible, rounds, and the whole call's time
           against ONE uniform _stats call of --frames frames.  A record, not a pass criterion.
  beauty   with --parent-tree (a built cuda-volpath_amd directory of the parent commit: its library and its Python package): that
           build's vp_render_frames and this build's in child processes before and after the two steps above (parent, this build, ...,
           this build, parent), compared child against child; the image hashes must be equal."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("workloads")
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--round", type=int, default=32)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--beauty-frames", type=int, default=1024)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--step-seconds", type=int, default=300)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)      # rounds | return | beauty: one GPU step of one workload
args = ap.parse_args()
KEY = (0x9E3779B9, 0x85EBCA6B)
CLI_FLOORS = (1e-3, 1e-3, 1e-2)


def mmm(v):
    v = list(v)
    return "%.2f / %.2f / %.2f" % (min(v), statistics.median(v), max(v))


def spread(v):
    v = list(v)
    return 100.0 * (max(v) - min(v)) / statistics.median(v)


def sha(*arrays):
    import numpy as np
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:12]


# ---------------------------------------------------------------------------------------------------------- one GPU step (a child)
def child(step, spec):
    sys.path.insert(0, os.environ.get("VOLPATH_TREE") or os.path.join(ROOT, "cuda-volpath_amd"))
    import volpath as vp
    from volpath import scene
    lines = []
    say = lines.append

    def timed(fn):
        vp.synchronize(); vp.render_time_ms()
        t = time.perf_counter()
        out = fn()
        vp.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        ms, launches = vp.render_time_ms()
        return wall, ms, launches, out

    vp.set_device(0)
    N = args.beauty_frames if step == "beauty" else args.frames
    P, info = scene.setup(spec, rng_mode=int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7)), key=KEY, last_frame=N, sunsky=scene.default_sunsky())
    W, H, B = P.width, P.height, args.round
    buf = vp.DeviceBuffer(W, H)
    vp.prepare(P); vp.reserve_frames(P, N)
    vp.render_frames(buf.ptr, 0, 2, P); vp.synchronize()
    if step == "beauty":
        t = []
        for _ in range(args.repeat):
            buf.reset()
            t.append(timed(lambda: vp.render_frames(buf.ptr, 0, N, P))[:3])
        print(json.dumps({"times": t, "hash": sha(buf.download())}))
        return
    sky, trans, rec = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), tuple(vp.StatsBuffer(W, H) for _ in range(3))
    ptrs = (buf.ptr, sky.ptr, trans.ptr) + tuple(r.ptr for r in rec)
    adaptive_fn, stats_fn = vp.render_adaptive_group_layers, vp.render_frames_group_layers_stats
    vp.reserve_frames_groups(P, min(N, B) if step == "rounds" else N)

    def reset():
        for b in (buf, sky, trans) + rec:
            b.reset()

    def state():
        return sha(buf.download(), sky.download(), trans.download()), sha(*(r.download() for r in rec))

    if step == "rounds":
        rounds = -(-N // B)

        def adaptive():
            reset()
            return timed(lambda: adaptive_fn(*ptrs, 0, N, P, (0.0, 0.0, 0.0), CLI_FLOORS, N + 1, B))

        def uniform():
            reset()
            return timed(lambda: [stats_fn(*ptrs, f, min(B, N - f), P) for f in range(0, N, B)])

        adaptive_fn(*ptrs, 0, 4, P, (0.0, 0.0, 0.0), CLI_FLOORS, 5, 2)      # warm both: kernels loaded, lists built
        stats_fn(*ptrs, 0, 2, P); vp.synchronize()
        a, u = [], []
        for _ in range(args.repeat):
            a.append(adaptive()); ha = state()
            u.append(uniform()); hu = state()
        res = a[-1][3]
        assert res["samples"] == W * H * N and res["rounds"] == rounds and res["active_left"] == W * H, res
        say(f"== {spec}: {W}x{H}, group layers, {N} frames in {rounds} rounds / calls of {B}, {args.repeat} alternations (min / median / max)")
        say(f"rounds  adaptive call, nothing freezes  wall ms {mmm(x[0] for x in a)}   render kernel ms {mmm(x[1] for x in a)}   launches {a[0][2]}   planes {ha[0]} records {ha[1]}")
        say(f"rounds  _stats calls of {B} frames      wall ms {mmm(x[0] for x in u)}   render kernel ms {mmm(x[1] for x in u)}   launches {u[0][2]}   planes {hu[0]} records {hu[1]}"
            + ("" if ha == hu else "   STATES DIFFER"))
        wa, wu = statistics.median(x[0] for x in a), statistics.median(x[0] for x in u)
        ka, ku = statistics.median(x[1] for x in a), statistics.median(x[1] for x in u)
        sa, su = spread(x[0] for x in a), spread(x[0] for x in u)
        inside = abs(wa - wu) <= max(sa, su) / 100.0 * wu
        say(f"rounds  adaptive against _stats, medians: wall {wa - wu:+.2f} ms ({100.0 * (wa / wu - 1):+.2f} %), {(wa - wu) / rounds:+.3f} ms per round;"
            f" render kernel {ka - ku:+.2f} ms ({100.0 * (ka / ku - 1):+.2f} %); wall minus render kernel: adaptive {wa - ka:.2f} ms, _stats {wu - ku:.2f} ms;"
            f" spread of the alternation (max - min over median): adaptive {sa:.2f} %, _stats {su:.2f} %"
            + (" -- the difference is INSIDE the spread" if inside else " -- the difference is outside the spread"))
        if ha != hu:
            raise SystemExit("\n".join(lines) + "\nthe adaptive call and the _stats calls left different bits")
    else:
        adaptive_fn(*ptrs, 0, 4, P, (0.0, 0.0, 0.0), CLI_FLOORS, 5, 2)
        stats_fn(*ptrs, 0, 2, P); vp.synchronize()
        a, u = [], []
        for _ in range(args.repeat):
            reset()
            a.append(timed(lambda: adaptive_fn(*ptrs, 0, N, P, (0.05, 0.05, 0.05), CLI_FLOORS, 16, B)))
            reset()
            u.append(timed(lambda: stats_fn(*ptrs, 0, N, P)))
        res = a[-1][3]
        assert all(x[3] == res for x in a), "the adaptive call is not reproducible"
        wa, wu = statistics.median(x[0] for x in a), statistics.median(x[0] for x in u)
        say(f"return  {spec}: rel_tol (0.05, 0.05, 0.05), floors {CLI_FLOORS}, min_frames 16, rounds of {B}, at most {N} frames:"
            f" {res['samples']} of {W * H * N} samples ({100.0 * res['samples'] / (W * H * N):.1f} %), {res['rounds']} rounds, {res['active_left']} of {W * H} pixels still active;"
            f" wall ms adaptive {mmm(x[0] for x in a)} against ONE uniform _stats call {mmm(x[0] for x in u)} ({100.0 * (wa / wu - 1):+.1f} %, {wu / wa:.2f} x);"
            f" launches {a[0][2]} against {u[0][2]}")
    print(json.dumps({"lines": lines}))


# ------------------------------------------------------------------------------------------------------------------- the driver
def main():
    out_file = open(args.out, "a") if args.out else None

    def say(*a):
        line = " ".join(str(v) for v in a)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n"); out_file.flush()

    own_tree = os.path.join(ROOT, "cuda-volpath_amd")
    specs = args.workloads.split(",")
    plan = []
    for spec in specs:
        before = [("beauty", spec, args.parent_tree, "parent"), ("beauty", spec, own_tree, "own")] if args.parent_tree else []
        plan += before + [("rounds", spec, own_tree, "own"), ("return", spec, own_tree, "own")] + before[::-1]
    beauty = {}
    for i, (step, spec, tree, who) in enumerate(plan):
        env = dict(os.environ, VOLPATH_TREE=os.path.abspath(tree))
        env.pop("VOLPATH_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), spec, "--child", step, "--frames", str(args.frames), "--round", str(args.round),
               "--repeat", str(args.repeat), "--beauty-frames", str(args.beauty_frames)]
        why = None
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.step_seconds)
            if r.returncode:
                why = "exit status %d: %s" % (r.returncode, (r.stderr or r.stdout)[-1500:])
        except subprocess.TimeoutExpired:
            why = "no result within %d s" % args.step_seconds
        if why:
            say(f"FAILED  {step} {spec} ({who}): {why}")
            for s2, sp2, _, w2 in plan[i:]:
                say(f"not measured: {s2} {sp2} ({w2})")
            raise SystemExit(1)
        result = json.loads(r.stdout.strip().splitlines()[-1])
        if step == "beauty":
            beauty.setdefault((spec, who), []).append(result)
        else:
            for line in result["lines"]:
                say(line)
        if step == "beauty" and len(beauty.get((spec, "parent"), [])) == 2 and len(beauty.get((spec, "own"), [])) == 2:
            t = [x for b in beauty[(spec, "parent")] for x in b["times"]]
            o = [x for b in beauty[(spec, "own")] for x in b["times"]]
            hashes = {b["hash"] for k in ("parent", "own") for b in beauty[(spec, k)]}
            kp, ko = statistics.median(x[1] for x in t), statistics.median(x[1] for x in o)
            wp, wo = statistics.median(x[0] for x in t), statistics.median(x[0] for x in o)
            say(f"beauty  {spec}, vp_render_frames of {args.beauty_frames} frames, child processes before and after: parent wall ms {mmm(x[0] for x in t)} kernel ms {mmm(x[1] for x in t)};"
                f" this build wall ms {mmm(x[0] for x in o)} kernel ms {mmm(x[1] for x in o)}; image {sorted(hashes)[0]}" + ("" if len(hashes) == 1 else "   IMAGES DIFFER"))
            say(f"beauty  {spec}, this build against the parent's, child against child, medians: kernel {100.0 * (ko / kp - 1):+.2f} %, wall {100.0 * (wo / wp - 1):+.2f} %"
                f" (kernel spreads: parent {spread(x[1] for x in t):.2f} %, this build {spread(x[1] for x in o):.2f} %)")
            if len(hashes) != 1:
                raise SystemExit(1)


if args.child:
    child(args.child, args.workloads)
else:
    main()
