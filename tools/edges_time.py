"""Feathering to alpha edges (--feather_edges, EU_LOAD_EDGES), two figures.
Load: a --side x --side RGBA fisheye facet with an elliptic lens crop, loaded with and without the distance plane -
wall time of Source.load from host floats to a synchronised device, the two alternating, --reps times after a warm-up
of each; min, median and max and the spread of each, and the ratio of the medians. The two passes of the transform
are kernels of their own (eu_edges_rows_kernel, eu_edges_cols_kernel): their times come from a kernel trace of this
tool with --loads-only, which does nothing else.
Blend: six such facets (front / right / back / left / up / down) onto a spherical target of twice the side, as
`feather` - kernel time of eu_hip_render_timed, HIP events around --iters launches - with planes and without, the two
alternating. Needs a HIP device. Prints one JSON line per figure; --out FILE keeps them (a JSON list).
    python tools/edges_time.py [--out profiles/edges_times.json] [--side 4096] [--reps 7] [--iters 10] [--loads-only]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import envutil_amd as ea  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--side", type=int, default=4096)
ap.add_argument("--blend-side", type=int, default=2048)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--loads-only", action="store_true")
opt = ap.parse_args()
if opt.reps < 5:
    sys.exit("at least five repetitions")
if ea.device_count() < 1:
    sys.exit("edges_time.py needs a HIP device: there is nothing to time without one")
VIEWS = [(0, 0, 0), (90, 0, 0), (180, 0, 0), (270, 0, 0), (0, 90, 0), (0, -90, 0)]


def stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4),
            "spread": round(max(v) - min(v), 4)}


def picture(side):
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    img = np.stack([0.5 + 0.3 * np.sin(x / (40.0 + 9 * c)) * np.cos(y / (55.0 + 7 * c)) for c in range(3)], 2)
    return np.ascontiguousarray(img, np.float32)


def load(img, edges, view=(0, 0, 0)):
    side = img.shape[0]
    fct = ea.facet_spec(ea.FISHEYE, side, side, 130.0, nchannels=4, yaw=view[0], pitch=view[1], roll=view[2])
    m = side // 50
    return ea.Source.load(fct, img, 1, crop=(m, side - m, m, side - m), crop_kind=2, edges=edges)


def load_times(side):
    img = picture(side)
    ms = {True: [], False: []}
    for flag in (True, False):
        load(img, flag).release()
    for _ in range(opt.reps):
        for flag in (True, False):
            ea.sync()
            t0 = time.perf_counter()
            s = load(img, flag)
            ea.sync()
            ms[flag].append(1e3 * (time.perf_counter() - t0))
            s.release()
    st = {"flagged": stats(ms[True]), "unflagged": stats(ms[False])}
    return {"figure": f"load of a {side} x {side} RGBA fisheye facet (3 channels from the host, alpha gained) with an elliptic crop, degree 1",
            "what": "wall time of Source.load to a synchronised device, ms", "repetitions": opt.reps, "load_ms": st,
            "flagged_over_unflagged": round(st["flagged"]["median"] / st["unflagged"]["median"], 4),
            "plane_bytes": 4 * side * side}


def blend_times(side):
    import torch
    img = picture(side)
    sets = {flag: [load(img, flag, v) for v in VIEWS] for flag in (True, False)}
    tw, th = 2 * side, side
    out = torch.empty((th, tw, 4), device="cuda:0", dtype=torch.float32)
    a = ea.arguments(ea.SPHERICAL, tw, th, 360.0, spline_degree=1, synopsis="feather")
    ms = {True: [], False: []}
    for flag in (True, False):
        ea.render_timed(a, sets[flag], out.data_ptr(), max(opt.iters, 20), 4)
    for _ in range(opt.reps):
        for flag in (True, False):
            ms[flag].append(ea.render_timed(a, sets[flag], out.data_ptr(), opt.iters, 4))
    st = {"with_planes": stats(ms[True]), "without": stats(ms[False])}
    return {"figure": f"feather, six {side} x {side} RGBA fisheye facets with elliptic crops -> spherical {tw} x {th}, degree 1",
            "what": "kernel time per launch, ms: HIP events around --iters launches", "repetitions": opt.reps, "iters": opt.iters,
            "kernel_ms": st, "with_over_without": round(st["with_planes"]["median"] / st["without"]["median"], 4)}


results = [load_times(opt.side)]
print(json.dumps(results[-1]), flush=True)
if not opt.loads_only:
    results.append(blend_times(opt.blend_side))
    print(json.dumps(results[-1]), flush=True)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
