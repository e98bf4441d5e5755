"""A camera path through eu_hip_render_views against the same path as a loop of eu_hip_render calls.
From a 4096 x 2048 lat/lon RGB source, in one process, into device memory:
    64 views of 256 x 256, rectilinear, hfov 60, yaw stepping 5 degrees per view, at degrees 1 and 3;
    16 views of 1920 x 1080, rectilinear, hfov 90, same path, degree 3.
Each job is rendered two ways: (a) one eu_hip_render per view, then eu_hip_sync(); (b) one eu_hip_render_views,
then eu_hip_sync(). What is measured is the HOST's wall clock around calls plus sync - the host side is what the
call exists for - with the targets and the view array built beforehand. The two ways alternate, after one warm-up
each; min, median and max over the repetitions are reported, and whether (b)'s median lies below (a)'s minimum by
more than (a)'s own spread (max - min). The frames of the two ways are compared bit for bit.
Prints one JSON line per job; --out FILE keeps them (a JSON list).
    python tools/views_time.py [--out profiles/views_times.json] [--reps 15]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import envutil_amd as ea  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--source", default="4096x2048")
opt = ap.parse_args()
if opt.reps < 7:
    sys.exit("at least seven repetitions")
if ea.device_count() < 1:
    sys.exit("views_time.py needs a HIP device: there is nothing to time without one")

SW, SH = (int(v) for v in opt.source.split("x"))
# name, views, width, height, hfov, degree
JOBS = [("64 x 256x256 d1", 64, 256, 256, 60.0, 1), ("64 x 256x256 d3", 64, 256, 256, 60.0, 3),
        ("16 x 1920x1080 d3", 16, 1920, 1080, 90.0, 3)]
L = ea.lib()


def malloc(nbytes):
    p = C.c_void_p()
    ea.api._check(L.eu_hip_malloc(C.byref(p), nbytes))
    return p


def download(dev, nbytes):
    out = np.zeros(nbytes // 4, np.uint32)
    ea.api._check(L.eu_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dev, nbytes))
    return out


def stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def run(name, n, w, h, hfov, degree, src):
    yprs = [(5.0 * k, 0.0, 0.0) for k in range(n)]
    row, frame = w * 3 * 4, w * h * 3 * 4
    out_a, out_b = malloc(n * frame), malloc(n * frame)
    try:
        arr = (C.c_void_p * 1)(src.handle)
        # (a): one target per view, built beforehand
        jobs_a = [ea.arguments(ea.RECTILINEAR, w, h, hfov, yaw=y, pitch=p, roll=r, spline_degree=degree) for y, p, r in yprs]
        targets = [a.target(3) for a in jobs_a]
        dst = [C.c_void_p(out_a.value + k * frame) for k in range(n)]
        # (b): the shared target and the view array
        shared = ea.arguments(ea.RECTILINEAR, w, h, hfov, spline_degree=degree)
        t = shared.target(3)
        views = ea.api._views_struct(shared, yprs)

        def loop_ms():
            t0 = time.perf_counter()
            for k in range(n):
                rc = L.eu_hip_render(C.byref(targets[k]), arr, 1, dst[k], row, 1, None)
                if rc:
                    ea.api._check(rc)
            ea.api._check(L.eu_hip_sync())
            return (time.perf_counter() - t0) * 1e3

        def views_ms():
            t0 = time.perf_counter()
            rc = L.eu_hip_render_views(C.byref(t), views, n, src.handle, out_b, row, frame, 1, None)
            ea.api._check(rc)
            ea.api._check(L.eu_hip_sync())
            return (time.perf_counter() - t0) * 1e3

        loop_ms(), views_ms()                      # one warm-up each
        a_ms, b_ms = [], []
        for _ in range(opt.reps):
            a_ms.append(loop_ms())
            b_ms.append(views_ms())
        same = bool((download(out_a, n * frame) == download(out_b, n * frame)).all())
        if not same:
            sys.exit(f"{name}: the frames of the two ways differ - no timing is kept")
        sa, sb = stats(a_ms), stats(b_ms)
        spread = sa["max"] - sa["min"]
        return {"job": name, "source": f"{SW}x{SH} lat/lon RGB", "degree": degree, "views": n, "view": f"{w}x{h}",
                "repetitions": opt.reps, "frames_equal": same,
                "loop_of_render_ms": sa, "render_views_ms": sb,
                "loop_spread_ms": round(spread, 4),
                "views_median_below_loop_min_by_more_than_spread": bool(sa["min"] - sb["median"] > spread),
                "per_view_us": {"loop_median": round(1e3 * sa["median"] / n, 2), "views_median": round(1e3 * sb["median"] / n, 2)},
                "all_ms_loop": [round(v, 4) for v in a_ms], "all_ms_views": [round(v, 4) for v in b_ms]}
    finally:
        L.eu_hip_free(out_a)
        L.eu_hip_free(out_b)


px = np.random.default_rng(12345).random((SH, SW, 3), dtype=np.float32)
sources = {}
results = []
for name, n, w, h, hfov, degree in JOBS:
    if degree not in sources:
        sources[degree] = ea.Source.load(ea.facet_spec(ea.SPHERICAL, SW, SH, 360.0, nchannels=3), px, degree)
    results.append(run(name, n, w, h, hfov, degree, sources[degree]))
    print(json.dumps(results[-1]), flush=True)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
