"""What per-pixel filter selection costs and what it returns (development tool; the bench is bench.py):

    python scripts/denoise_select_cost.py c2,c4f [--frames 16] [--ref-frames 1024] [--candidates 5:1:0.45,10:3:0.45] [--var-params 1:3:0.45]
                                          [--select-radii 1:1] [--repeat 21] [--plain-repeat 5] [--parent-tree DIR [--beauty-frames 256]] [--out FILE]

A workload is a bench workload of volpath/scene.py at its own image size (c2: 800 x 600, c4f: 1280 x 720).  Per workload, on the two
halves of --frames frames (vp_render_frames_halves_stats):

  cost     vp_cross_error; vp_select at radii (1, 1) and (3, 3) with n = 2 and n = 4 candidates, the tiled form (0) against the plain one
           (1), alternated; the whole output stage of --denoise-select (volpath.denoise_select with --candidates) against the one of
           --denoise-var at the LAST candidate's window (volpath.denoise_cross with the variance stage), alternated.  HIP events on the
           context's stream round each warm call; min / median / max in ms, and the spread (max - min over the median).
  returns  relative L2 of the RGB mean image against the mean of --ref-frames frames under OTHER keys -- the reference and the keys of
           denoise_cross_cost.py's table --: vp_denoise self-guided on all the frames at the first candidate's window, the cross-filter
           with the variance stage at each candidate's window, the selection between them, the per-pixel best of the candidates (which
           uses the reference), and the share of pixels each candidate wins; smoothing and blend radius from --select-radii.

With --parent-tree (a built cuda-volpath_amd directory of the parent commit: its library and its Python package) vp_render_frames of
that build and of this one run --beauty-frames frames in child processes of denoise_cross_cost.py, alternated (parent, this build,
parent, this build): the two builds are compared child against child, and the parent's own two readings are the margin."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-volpath_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("workloads")
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--ref-frames", type=int, default=1024)
ap.add_argument("--candidates", default="5:1:0.45,10:3:0.45")
ap.add_argument("--var-params", default="1:3:0.45")
ap.add_argument("--select-radii", default="1:1")
ap.add_argument("--repeat", type=int, default=21)
ap.add_argument("--plain-repeat", type=int, default=5)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--beauty-frames", type=int, default=256)
ap.add_argument("--out", default=None)
args = ap.parse_args()
out_file = open(args.out, "a") if args.out else None
KEY, REF_KEY = (0x9E3779B9, 0x85EBCA6B), (0x1234567, 0x7654321)
parse = lambda s: [(int(r), int(f), float(k)) for r, f, k in (p.split(":") for p in s.split(","))]
CANDS, VAR = parse(args.candidates), parse(args.var_params)[0]
SMOOTH, BLEND = (int(v) for v in args.select_radii.split(":"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import volpath as vp  # noqa: E402
from volpath import scene  # noqa: E402

RNG = int(os.environ.get("VP_PERF_RNG", vp.RNG_PHILOX7))


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n"); out_file.flush()


def mmm(v):
    v = list(v)
    return "%.3f / %.3f / %.3f (spread %.1f %%)" % (min(v), statistics.median(v), max(v), 100.0 * (max(v) - min(v)) / statistics.median(v))


def rel_l2(img, ref):
    a, b = img[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


if not torch.cuda.is_available():
    raise SystemExit("denoise_select_cost.py needs a GPU: there is nothing to time without one")


def beauty_child(spec, tree):
    """vp_render_frames of a build of the library in a child process of denoise_cross_cost.py: {"times": [(wall, kernel, launches)], "hash"}"""
    env = dict(os.environ, VOLPATH_TREE=os.path.abspath(tree))
    env.pop("VOLPATH_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "denoise_cross_cost.py"), spec, "--frames", str(args.beauty_frames), "--repeat", "5", "--plain-child"],
                       env=env, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("child with %s failed: %s" % (tree, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


if args.parent_tree:
    # before this process opens the device: one process with the GPU at a time
    own_tree = os.path.join(ROOT, "cuda-volpath_amd")
    for spec in args.workloads.split(","):
        runs = [(who, beauty_child(spec, tree)) for who, tree in (("parent", args.parent_tree), ("own", own_tree), ("parent", args.parent_tree), ("own", own_tree))]
        kern = {who: [statistics.median(x[1] for x in r["times"]) for w, r in runs if w == who] for who in ("parent", "own")}
        hashes = {who: {r["hash"] for w, r in runs if w == who} for who in ("parent", "own")}
        kp, ko = statistics.mean(kern["parent"]), statistics.mean(kern["own"])
        say(f"beauty  {spec}  vp_render_frames, {args.beauty_frames} frames, child processes in the order parent, own, parent, own; kernel ms, median of 5 per child:"
            f" parent {kern['parent'][0]:.3f}, {kern['parent'][1]:.3f}   own {kern['own'][0]:.3f}, {kern['own'][1]:.3f}"
            f"   own against parent {100.0 * (ko / kp - 1):+.2f} %   the parent's two readings differ by {100.0 * abs(kern['parent'][0] - kern['parent'][1]) / kp:.2f} %"
            f"   same image: {hashes['parent'] == hashes['own'] and len(hashes['own']) == 1}")

torch.cuda.set_device(0)
vp.set_device(0)
stream = torch.cuda.Stream()
vp.set_stream(stream.cuda_stream)
sky = scene.default_sunsky()


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternated(calls, repeat):
    """each call once to warm it, then `repeat` rounds of all of them in turn: {name: [ms]}"""
    for _, c in calls:
        c()
    vp.synchronize()
    ms = {n: [] for n, _ in calls}
    for _ in range(repeat):
        for n, c in calls:
            ms[n].append(timed(c))
    return ms


class Bytes:
    def __init__(self, n):
        self.n = n
        self.ptr = vp.lib().vp_malloc(n)
        assert self.ptr

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes == self.n
        vp.lib().vp_download(out.ctypes.data, self.ptr, self.n)
        return out

    def free(self):
        vp.lib().vp_free(self.ptr)


for wl in args.workloads.split(","):
    N = args.frames
    P, info = scene.setup(wl, rng_mode=RNG, key=REF_KEY, last_frame=max(N, args.ref_frames), sunsky=sky)
    W, H = P.width, P.height
    npix = W * H
    ref = vp.DeviceBuffer(W, H)
    vp.render_frames(ref.ptr, 0, args.ref_frames, P)
    vp.scale(ref.ptr, ref.ptr, npix, 1.0 / args.ref_frames)
    ref_img = ref.download()
    vp.set_rng(RNG, KEY)
    whole, wrec = vp.DeviceBuffer(W, H), vp.StatsBuffer(W, H)
    h = (vp.DeviceBuffer(W, H), vp.DeviceBuffer(W, H))
    rec = (vp.StatsBuffer(W, H), vp.StatsBuffer(W, H))
    dst, dst1, ta, tb = (vp.DeviceBuffer(W, H) for _ in range(4))
    img = [vp.DeviceBuffer(W, H) for _ in CANDS]
    err = [Bytes(npix * 4) for _ in CANDS]
    u, q, uf = Bytes(npix * 4), Bytes(npix * 4), Bytes(npix * 4)
    idx, idx1 = Bytes(npix), Bytes(npix)
    vp.render_frames_stats(whole.ptr, wrec.ptr, 0, N, P)
    vp.render_frames_halves_stats(h[0].ptr, h[1].ptr, rec[0].ptr, rec[1].ptr, 0, N, P)
    say(f"== {wl}: {W}x{H}, {N} frames ({(N + 1) // 2} + {N // 2} in the halves), reference {args.ref_frames} frames under other keys;"
        f" {args.repeat} warm calls each, the plain form {args.plain_repeat} (min / median / max in ms, HIP events)")
    sel_args = dict(candidates=CANDS, smooth=SMOOTH, blend=BLEND, variance=VAR, var_ptrs=(u.ptr, q.ptr, uf.ptr),
                    tmp=(ta.ptr, tb.ptr, [i.ptr for i in img], [e.ptr for e in err]))
    halves = (h[0].ptr, rec[0].ptr, h[1].ptr, rec[1].ptr)
    vp.set_denoise_form(0)
    vp.denoise_select(dst.ptr, idx.ptr, *halves, W, H, **sel_args)          # fills the candidates' images and error planes

    # ---- cost
    ms = alternated([("err", lambda: vp.cross_error(err[-1].ptr, ta.ptr, tb.ptr, *halves, npix))], args.repeat)
    say(f"cost  {wl}  vp_cross_error  {mmm(ms['err'])}")
    # n = 4: the candidates' planes twice over -- the work of four planes, whatever they hold
    planes = {2: ([i.ptr for i in img[:2]], [e.ptr for e in err[:2]]), 4: ([i.ptr for i in (img * 2)[:4]], [e.ptr for e in (err * 2)[:4]])}
    for n in (2, 4):
        if len(CANDS) < 2:
            break
        for Rs, Rb in ((1, 1), (3, 3)):
            def run(form, d, ix, n=n, Rs=Rs, Rb=Rb):
                vp.set_denoise_form(form)
                vp.select(d.ptr, ix.ptr, planes[n][0], planes[n][1], W, H, Rs, Rb)
            ms = alternated([("tiled", lambda: run(0, dst, idx)), ("plain", lambda: run(1, dst1, idx1))], args.plain_repeat)
            same = dst.download().tobytes() == dst1.download().tobytes() and idx.download(np.uint8, (H, W)).tobytes() == idx1.download(np.uint8, (H, W)).tobytes()
            vp.set_denoise_form(0)
            t0 = alternated([("tiled", lambda: run(0, dst, idx))], args.repeat)["tiled"]
            say(f"cost  {wl}  vp_select n = {n}, radii ({Rs}, {Rb})  tiled {mmm(t0)}   alternated with plain: tiled {mmm(ms['tiled'])}   plain {mmm(ms['plain'])}"
                f"   plain / tiled {statistics.median(ms['plain']) / statistics.median(ms['tiled']):.1f} x   same bytes: {same}")
    vp.set_denoise_form(0)
    R, F, k = CANDS[-1]
    ms = alternated([("var", lambda: vp.denoise_cross(dst1.ptr, None, *halves, ta.ptr, tb.ptr, W, H, R, F, k, variance=VAR, var_ptrs=(u.ptr, q.ptr, uf.ptr))),
                     ("select", lambda: vp.denoise_select(dst.ptr, idx.ptr, *halves, W, H, **sel_args))], args.repeat)
    mv, msel = statistics.median(ms["var"]), statistics.median(ms["select"])
    say(f"cost  {wl}  the output stage: --denoise-var at ({R}, {F}, {k}) {mmm(ms['var'])}   --denoise-select of {CANDS} {mmm(ms['select'])}"
        f"   select against var, medians {100.0 * (msel / mv - 1):+.1f} %")

    # ---- returns
    R0, F0, k0 = CANDS[0]
    vp.denoise(dst1.ptr, whole.ptr, wrec.ptr, W, H, R0, F0, k0)
    self_guided = rel_l2(dst1.download(), ref_img)
    vp.denoise_select(dst.ptr, idx.ptr, *halves, W, H, **sel_args)
    selected = rel_l2(dst.download(), ref_img)
    index = idx.download(np.uint8, (H, W))
    cimg = [i.download() for i in img]
    cand = [rel_l2(c, ref_img) for c in cimg]
    se = np.stack([((c[..., :3].astype(np.float64) - ref_img[..., :3]) ** 2).sum(-1) for c in cimg])
    best = np.take_along_axis(np.stack(cimg), se.argmin(0)[None, ..., None], 0)[0]
    e0 = err[0].download(np.float32, (H, W))
    say(f"returns  {wl}, smooth {SMOOTH}, blend {BLEND}: rel L2 self-guided ({R0}, {F0}, {k0}) {self_guided:.4f} | " + " | ".join(f"--denoise-var {c} {v:.4f}" for c, v in zip(CANDS, cand))
        + f" | --denoise-select {selected:.4f} | per-pixel best (uses the reference) {rel_l2(best, ref_img):.4f} | share of the pixels won: "
        + ", ".join(f"candidate {c} {float((index == c).mean()):.3f}" for c in range(len(CANDS)))
        + f" | estimates of candidate 0: {float((e0 < 0).mean()):.3f} negative, {float((e0 == 0).mean()):.3f} zero"
        + f" | the selection is {'BETTER than both' if selected < min(cand) else 'between them' if selected <= max(cand) else 'WORSE than both'}"
        + f" and {'BETTER' if selected < self_guided else 'NOT better'} than self-guided")
    for x in [ref, whole, wrec, h[0], h[1], rec[0], rec[1], dst, dst1, ta, tb, u, q, uf, idx, idx1] + img + err:
        x.free()
