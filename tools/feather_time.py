"""The three synopses on one multi-facet job: bench.py's six-fisheye workload (WORKLOADS["config5"]: six 8192 x 8192
circular-fisheye facets, hfov 130, looking front / right / back / left / up / down, PTO lens a / b / c, onto a
16384 x 8192 spherical target, bilinear) composed as `panorama`, `hdr_merge` and `feather`, with 4-channel facets (the
workload's own: voronoi_syn_plus against the two weighted sums) and with 3-channel facets (voronoi_syn).
What is measured is KERNEL time: eu_hip_render_timed's HIP events on the library's stream around --iters launches into
device memory, after one untimed launch; the sources are loaded once and shared by the three. The three alternate,
--reps times, after a warm-up of every one of them that also brings the clocks up; min, median and max over the
repetitions are reported, and the spread of each. Nothing is promised about the numbers: they are what DESIGN.md 5 quotes.
The share of covered pixels of every synopsis' frame is reported, and the tool ends with an error where a frame is
mostly empty. Needs a HIP device: without one there is nothing to time.
Prints one JSON line per job; --out FILE keeps them (a JSON list).
    python tools/feather_time.py [--out profiles/feather_times.json] [--reps 9] [--iters 20] [--facet 8192] [--channels 4,3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import envutil_amd as ea  # noqa: E402
from bench import WORKLOADS, synth_on_device  # noqa: E402  (the workload is bench.py's; nothing of it is edited)

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--facet", type=int, default=0, help="facet size in pixels, square (default: the workload's)")
ap.add_argument("--channels", default="4,3")
ap.add_argument("--feather", type=float, default=0.0, help="ramp width in source pixels (default 0: half the facet)")
opt = ap.parse_args()
if opt.reps < 5:
    sys.exit("at least five repetitions")
if ea.device_count() < 1:
    sys.exit("feather_time.py needs a HIP device: there is nothing to time without one")
import torch  # noqa: E402

(sname, sw, sh, shfov), (tname, tw, th, thfov), _, degree, twine, ypr = WORKLOADS["config5"]
if opt.facet:
    tw, th = max(64, tw * opt.facet // sw), max(32, th * opt.facet // sh)
    sw = sh = opt.facet
sprj, tprj = ea.api.PROJECTION_NAMES.index(sname), ea.api.PROJECTION_NAMES.index(tname)
VIEWS = [(0, 0, 0), (90, 0, 0), (180, 0, 0), (270, 0, 0), (0, 90, 0), (0, -90, 0)]
SYNOPSES = ("panorama", "hdr_merge", "feather")
L = ea.lib()
dev = torch.device("cuda", 0)


def stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def run(nch):
    sources = []
    for v in VIEWS:
        img = synth_on_device(torch, dev, sw, sh, nch)
        if nch == 4:
            img[:, :, 3] = 1.0
        host = img.cpu().numpy()
        del img
        torch.cuda.empty_cache()
        sources.append(ea.Source.load(ea.facet_spec(sprj, sw, sh, shfov, nchannels=nch, yaw=v[0], pitch=v[1], roll=v[2],
                                                    lens=dict(a=0.01, b=-0.03, c=0.02)), host, degree))
        del host
        print(f"facet {len(sources)} of {len(VIEWS)} loaded ({nch} channels)", file=sys.stderr, flush=True)
    out = torch.empty((th, tw, nch), device=dev, dtype=torch.float32)
    jobs = {s: ea.arguments(tprj, tw, th, thfov, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree, twine=twine,
                            synopsis=s, feather=opt.feather if s == "feather" else 0.0) for s in SYNOPSES}

    def once(s, iters):
        return ea.render_timed(jobs[s], sources, out.data_ptr(), iters, nch)

    # warm-up: every shape of the timed window, and ~0.3 s of launches for the clocks
    share = {}
    for s in SYNOPSES:
        once(s, max(opt.iters, 20))
        ea.sync()
        frame = out[::16, ::16].cpu().numpy()
        share[s] = round(float((frame != 0).any(axis=2).mean()), 4)
        if share[s] < 0.5:
            sys.exit(f"{s}: the frame is mostly empty - no timing is kept")
    ms = {s: [] for s in SYNOPSES}
    for _ in range(opt.reps):
        for s in SYNOPSES:                       # the three alternate: a drift of the clocks hits all of them alike
            ms[s].append(once(s, opt.iters))
    st = {s: stats(ms[s]) for s in SYNOPSES}
    res = {"job": f"six {sname} facets {sw}x{sh}, {nch} channels, lens polynomial -> {tname} {tw}x{th}, degree {degree}",
           "what": "kernel time per launch, ms: HIP events around --iters launches, min / median / max over the repetitions",
           "repetitions": opt.reps, "iters": opt.iters, "feather_width": opt.feather, "covered_share": share,
           "kernel_ms": st, "spread_ms": {s: round(st[s]["max"] - st[s]["min"], 4) for s in SYNOPSES},
           "feather_over_hdr_merge": round(st["feather"]["median"] / st["hdr_merge"]["median"], 4),
           "feather_over_panorama": round(st["feather"]["median"] / st["panorama"]["median"], 4),
           "all_ms": {s: [round(v, 4) for v in ms[s]] for s in SYNOPSES}}
    for s in sources:
        s.release()
    del out
    torch.cuda.empty_cache()
    return res


results = []
for nch in (int(c) for c in opt.channels.split(",")):
    results.append(run(nch))
    print(json.dumps(results[-1]), flush=True)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
