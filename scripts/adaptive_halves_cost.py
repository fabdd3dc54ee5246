"""What the adaptive rounds on half-buffers (vp_render_adaptive_halves / vp_render_adaptive_planes_halves) cost
and return (development tool; the bench is bench.py):

    python scripts/adaptive_halves_cost.py c2,c4f [--frames 256] [--round 32] [--repeat 3] [--parent-tree DIR] [--out FILE]
                                                  [--step-seconds 300] [--steps adaptive,uniform,quality]

A workload is a bench workload of volpath/scene.py at the bench's size.  Every GPU step runs in a child process of its own under a time
limit of its own (--step-seconds); the first step that fails, or runs into its limit, ends the script with a non-zero status, and the
steps that were not reached are listed as "not measured".  The steps, per workload, each for the beauty image ("beauty") and for group
layers ("planes3"):

  adaptive  rounds on halves against the existing adaptive call at the same tolerance (0.05, the CLI's floors, min_frames 16):
            vp_render_adaptive_halves alternates `repeat` times with vp_render_adaptive (vp_render_adaptive_planes_halves with
            vp_render_adaptive_group_layers).  Whole-call wall time and render-kernel time, min / median / max, and the spread of the
            alternation.  The difference is the freeze kernel and the halves reduce -- and the other frozen set: the two rules are not
            the same rule, so the samples of both are stated.  With --parent-tree the existing call is ALSO timed in a child process of
            the parent's build (its library and Python package), before and after.
  uniform   the rounds themselves: the call on halves with tolerance 0 and min_frames above --frames (nothing freezes, every round
            renders every pixel) alternates with the same frames through vp_render_frames_halves_stats (_planes_halves_stats) in calls of
            --round frames; states compared by hash.
  quality   (beauty only) relative L2 of the RGB channels against the mean of 1024 other frames, at 16, 32 and 64 frames at most:
            rounds on halves at tolerance 0.05 (min_frames 8, rounds of 8) through the cross-filter, against the uniform halves call
            through the same filter at the frame count nearest to the samples the adaptive run used per pixel.  A record, whatever it is.
  render    with --parent-tree: that build's vp_render_frames and this build's in child processes before and after the other steps,
            compared child against child; the image hashes must be equal."""
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
ap.add_argument("--render-frames", type=int, default=1024)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--step-seconds", type=int, default=300)
ap.add_argument("--steps", default="adaptive,uniform,quality")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)      # one GPU step of one workload
args = ap.parse_args()
KEY = (0x9E3779B9, 0x85EBCA6B)
FLOORS3 = (1e-3, 1e-3, 1e-2)
TOL = 0.05


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


def compare(say, tag, what_a, a, what_b, b, rounds):
    wa, wb = statistics.median(x[0] for x in a), statistics.median(x[0] for x in b)
    ka, kb = statistics.median(x[1] for x in a), statistics.median(x[1] for x in b)
    sa, sb = spread(x[0] for x in a), spread(x[0] for x in b)
    say(f"{tag}  {what_a:34s} wall ms {mmm(x[0] for x in a)}   render kernel ms {mmm(x[1] for x in a)}   launches {a[0][2]}")
    say(f"{tag}  {what_b:34s} wall ms {mmm(x[0] for x in b)}   render kernel ms {mmm(x[1] for x in b)}   launches {b[0][2]}")
    inside = abs(wa - wb) <= max(sa, sb) / 100.0 * wb
    say(f"{tag}  first against second, medians: wall {wa - wb:+.2f} ms ({100.0 * (wa / wb - 1):+.2f} %), {(wa - wb) / rounds:+.3f} ms per round; render kernel {ka - kb:+.2f} ms"
        f" ({100.0 * (ka / kb - 1):+.2f} %); spread of the alternation (max - min over median): {sa:.2f} % and {sb:.2f} %"
        + (" -- the wall difference is INSIDE the spread" if inside else " -- the wall difference is outside the spread"))


# ---------------------------------------------------------------------------------------------------------- one GPU step (a child)
def child(step, spec):
    sys.path.insert(0, os.environ.get("VOLPATH_TREE") or os.path.join(ROOT, "cuda-volpath_amd"))
    import numpy as np
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
    N, B = args.frames, args.round
    last = {"render": args.render_frames, "quality": 1000 + 1024}.get(step, N)
    P, info = scene.setup(spec, rng_mode=int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7)), key=KEY, last_frame=last, sunsky=scene.default_sunsky())
    W, H = P.width, P.height
    buf = vp.DeviceBuffer(W, H)
    vp.prepare(P); vp.reserve_frames(P, args.render_frames if step == "render" else N)
    vp.render_frames(buf.ptr, 0, 2, P); vp.synchronize()
    if step == "render":
        t = []
        for _ in range(args.repeat):
            buf.reset()
            t.append(timed(lambda: vp.render_frames(buf.ptr, 0, args.render_frames, P))[:3])
        print(json.dumps({"times": t, "hash": sha(buf.download())}))
        return
    if step == "parent_adaptive":      # the existing adaptive calls, as the build in VOLPATH_TREE runs them
        out = {}
        rec = [vp.StatsBuffer(W, H) for _ in range(3)]
        acc = [buf, vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)]
        vp.reserve_frames_groups(P, N)
        for kind in ("beauty", "planes3"):
            t = []
            for _ in range(args.repeat + 1):
                for b in acc + rec:
                    b.reset()
                if kind == "beauty":
                    t.append(timed(lambda: vp.render_adaptive(acc[0].ptr, rec[0].ptr, 0, N, P, TOL, 1e-3, 16, B)))
                else:
                    t.append(timed(lambda: vp.render_adaptive_group_layers(*[b.ptr for b in acc + rec], 0, N, P, (TOL,) * 3, FLOORS3, 16, B)))
            out[kind] = {"times": [x[:3] for x in t[1:]], "samples": t[-1][3]["samples"]}
        print(json.dumps(out))
        return

    for kind in ("beauty", "planes3"):
        if step == "quality" and kind != "beauty":
            continue
        n = 1 if kind == "beauty" else 3
        half = [[(vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)) for _ in range(n)] for _ in (0, 1)]
        one = [(vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)) for _ in range(n)]
        ptrs = [[(a.ptr, r.ptr) for a, r in h] for h in half]
        everything = [b for h in half for pair in h for b in pair] + [b for pair in one for b in pair]
        vp.reserve_frames_groups(P, N)
        tol, fl = ((TOL,), (1e-3,)) if kind == "beauty" else ((TOL,) * 3, FLOORS3)

        def reset():
            for b in everything:
                b.reset()

        def state():
            return sha(*[b.download() for h in half for pair in h for b in pair])

        def on_halves(first, frames, tol, min_frames, round_frames):
            if kind == "beauty":
                return vp.render_adaptive_halves(ptrs[0][0][0], ptrs[1][0][0], ptrs[0][0][1], ptrs[1][0][1], first, frames, P, tol[0], fl[0], min_frames, round_frames)
            return vp.render_adaptive_planes_halves(vp.PLANES_GROUP_LAYERS, ptrs[0], ptrs[1], first, frames, P, tol, fl, min_frames, round_frames)

        def existing(first, frames):
            if kind == "beauty":
                return vp.render_adaptive(one[0][0].ptr, one[0][1].ptr, first, frames, P, TOL, 1e-3, 16, B)
            return vp.render_adaptive_group_layers(*[a.ptr for a, _ in one], *[r.ptr for _, r in one], first, frames, P, tol, fl, 16, B)

        def uniform_halves(first, frames):
            if kind == "beauty":
                return vp.render_frames_halves_stats(ptrs[0][0][0], ptrs[1][0][0], ptrs[0][0][1], ptrs[1][0][1], first, frames, P)
            return vp.render_frames_planes_halves_stats(vp.PLANES_GROUP_LAYERS, ptrs[0], ptrs[1], first, frames, P)

        on_halves(0, 4, (0.0,) * n, 5, 2); existing(0, 4); uniform_halves(0, 2); vp.synchronize()      # warm: kernels loaded, lists built
        rounds = -(-N // B)
        if step == "adaptive":
            a, e = [], []
            for _ in range(args.repeat):
                reset(); a.append(timed(lambda: on_halves(0, N, tol, 16, B)))
                reset(); e.append(timed(lambda: existing(0, N)))
            ra, re_ = a[-1][3], e[-1][3]
            assert all(x[3] == ra for x in a) and all(x[3] == re_ for x in e), "an adaptive call is not reproducible"
            say(f"== {spec} {kind}: {W}x{H}, rel_tol {TOL}, min_frames 16, rounds of {B}, at most {N} frames, {args.repeat} alternations (min / median / max)")
            compare(say, "adaptive", "rounds on halves", a, "the existing adaptive call", e, max(ra["rounds"], 1))
            say(f"adaptive  rounds on halves: {ra['samples']} of {W * H * N} samples ({100.0 * ra['samples'] / (W * H * N):.1f} %), {ra['rounds']} rounds, {ra['active_left']} pixels still active;"
                f" the existing call: {re_['samples']} samples ({100.0 * re_['samples'] / (W * H * N):.1f} %), {re_['rounds']} rounds, {re_['active_left']} still active")
        elif step == "uniform":
            a, u = [], []
            for _ in range(args.repeat):
                reset(); a.append(timed(lambda: on_halves(0, N, (0.0,) * n, N + 1, B))); ha = state()
                reset(); u.append(timed(lambda: [uniform_halves(f, min(B, N - f)) for f in range(0, N, B)])); hu = state()
            res = a[-1][3]
            assert res["samples"] == W * H * N and res["rounds"] == rounds and res["active_left"] == W * H, res
            say(f"== {spec} {kind}: {W}x{H}, {N} frames in {rounds} rounds / calls of {B}, nothing freezes, {args.repeat} alternations (min / median / max)")
            compare(say, "uniform ", "rounds on halves, nothing freezes", a, f"uniform halves calls of {B} frames", u, rounds)
            say(f"uniform   states: {ha} and {hu}" + ("" if ha == hu else "   STATES DIFFER"))
            if ha != hu:
                raise SystemExit("\n".join(lines) + "\nthe rounds and the uniform halves calls left different bits")
        elif step == "quality" and kind == "beauty":
            ref = vp.DeviceBuffer(W, H)
            vp.render_frames(ref.ptr, 1000, 1024, P)
            want = ref.download().astype(np.float64)[..., :3] / 1024.0
            dst, ta, tb = vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H)

            def rel_l2():
                vp.denoise_cross(dst.ptr, None, ptrs[0][0][0], ptrs[0][0][1], ptrs[1][0][0], ptrs[1][0][1], ta.ptr, tb.ptr, W, H, 5, 1, 0.45)
                got = dst.download().astype(np.float64)[..., :3]
                return float(np.sqrt(((got - want) ** 2).sum() / (want ** 2).sum()))

            for cap in (16, 32, 64):
                reset()
                res = on_halves(0, cap, (TOL,), 8, 8)
                qa = rel_l2()
                per_pixel = res["samples"] / float(W * H)
                nu = max(2, 2 * int(round(per_pixel / 2.0)))      # an even count: as many frames for one half as for the other
                reset()
                uniform_halves(0, nu)
                qu = rel_l2()
                reset()
                uniform_halves(0, cap)
                qc = rel_l2()
                say(f"quality   {spec}: at most {cap} frames, --cross-noise {TOL} (min 8, rounds of 8) -> {per_pixel:.2f} samples per pixel, {res['active_left']} pixels still active,"
                    f" relative L2 after the cross-filter {qa:.6f}; uniform halves of {nu} frames through the same filter {qu:.6f}; uniform halves of all {cap} frames {qc:.6f}")
        for b in everything:
            b.free()
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
    steps = [s for s in args.steps.split(",") if s]
    plan = []
    for spec in args.workloads.split(","):
        before = [("render", spec, args.parent_tree, "parent"), ("render", spec, own_tree, "own"), ("parent_adaptive", spec, args.parent_tree, "parent")] if args.parent_tree else []
        plan += before + [(s, spec, own_tree, "own") for s in steps] + before[::-1]
    render, parent_adaptive = {}, {}
    for i, (step, spec, tree, who) in enumerate(plan):
        env = dict(os.environ, VOLPATH_TREE=os.path.abspath(tree))
        env.pop("VOLPATH_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), spec, "--child", step, "--frames", str(args.frames), "--round", str(args.round),
               "--repeat", str(args.repeat), "--render-frames", str(args.render_frames)]
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
        if step == "render":
            render.setdefault((spec, who), []).append(result)
        elif step == "parent_adaptive":
            parent_adaptive.setdefault(spec, []).append(result)
            if len(parent_adaptive[spec]) == 2:
                for kind in ("beauty", "planes3"):
                    t = [x for b in parent_adaptive[spec] for x in b[kind]["times"]]
                    say(f"adaptive  {spec} {kind}: the PARENT build's existing adaptive call, child processes before and after: wall ms {mmm(x[0] for x in t)}"
                        f"   render kernel ms {mmm(x[1] for x in t)}   launches {t[0][2]}   samples {parent_adaptive[spec][0][kind]['samples']}")
        else:
            for line in result["lines"]:
                say(line)
        if step == "render" and len(render.get((spec, "parent"), [])) == 2 and len(render.get((spec, "own"), [])) == 2:
            t = [x for b in render[(spec, "parent")] for x in b["times"]]
            o = [x for b in render[(spec, "own")] for x in b["times"]]
            hashes = {b["hash"] for k in ("parent", "own") for b in render[(spec, k)]}
            kp, ko = statistics.median(x[1] for x in t), statistics.median(x[1] for x in o)
            wp, wo = statistics.median(x[0] for x in t), statistics.median(x[0] for x in o)
            say(f"render    {spec}, vp_render_frames of {args.render_frames} frames, child processes before and after: parent wall ms {mmm(x[0] for x in t)} kernel ms {mmm(x[1] for x in t)};"
                f" this build wall ms {mmm(x[0] for x in o)} kernel ms {mmm(x[1] for x in o)}; image {sorted(hashes)[0]}" + ("" if len(hashes) == 1 else "   IMAGES DIFFER"))
            say(f"render    {spec}, this build against the parent's, child against child, medians: kernel {100.0 * (ko / kp - 1):+.2f} %, wall {100.0 * (wo / wp - 1):+.2f} %"
                f" (kernel spreads: parent {spread(x[1] for x in t):.2f} %, this build {spread(x[1] for x in o):.2f} %)")
            if len(hashes) != 1:
                raise SystemExit(1)


if args.child:
    child(args.child, args.workloads)
else:
    main()
