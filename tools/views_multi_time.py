"""A camera path over a multi-facet job through eu_hip_render_views_multi against the same path as a loop of
eu_hip_render calls. Six circular-fisheye facets (140 degrees, PTO lens polynomial, looking front / right / back /
left / up / down with a little roll, brighten 1 .. 1.25: the set of tests/test_gpu_parity.py's facet_set) of
--facet pixels (default 1024x1024), spline degree 1, in one process, into device memory:
    64 views of 256 x 256, rectilinear, hfov 60, yaw stepping 5 degrees per view,
    once with RGB facets (voronoi_syn) and once with RGBA facets with feathered alpha (voronoi_syn_plus).
Each job is rendered two ways: (a) one eu_hip_render per view, then eu_hip_sync(); (b) one
eu_hip_render_views_multi, then eu_hip_sync(). What is measured is the HOST's wall clock around calls plus sync, with
the targets and the view array built beforehand. The two ways alternate, after one warm-up each; min, median and max
over the repetitions are reported, and whether (b)'s median lies below (a)'s minimum by more than (a)'s own spread
(max - min). (b) per view bounds the kernel time of a view from above: what is left of (a) per view is host work.
The frames of the two ways are compared bit for bit; the tool ends with an error if they differ.
Prints one JSON line per job; --out FILE keeps them (a JSON list).
    python tools/views_multi_time.py [--out profiles/views_multi_times.json] [--reps 15]"""
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
ap.add_argument("--facet", default="1024x1024")
opt = ap.parse_args()
if opt.reps < 7:
    sys.exit("at least seven repetitions")
if ea.device_count() < 1:
    sys.exit("views_multi_time.py needs a HIP device: there is nothing to time without one")

FW, FH = (int(v) for v in opt.facet.split("x"))
N, W, H, HFOV, DEGREE = 64, 256, 256, 60.0, 1
FACETS = [(0, 0, 0), (90, 0, 3), (180, 0, -2), (270, 0, 1), (0, 90, 0), (0, -90, 5)]
LENS = dict(a=0.01, b=-0.03, c=0.02)
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


def facets(nch):
    rng = np.random.default_rng(12345 + nch)
    out = []
    for i, (yaw, pitch, roll) in enumerate(FACETS):
        px = rng.random((FH, FW, nch), dtype=np.float32)
        if nch == 4:
            yy, xx = np.mgrid[0:FH, 0:FW]
            r = np.hypot((xx - FW / 2) / (FW / 2), (yy - FH / 2) / (FH / 2))
            px[:, :, 3] = np.clip(1.6 - 1.4 * r, 0.0, 1.0)
            px[:, :, :3] *= px[:, :, 3:]
        out.append(ea.Source.load(ea.facet_spec(ea.FISHEYE, FW, FH, 140.0, nchannels=nch, yaw=yaw, pitch=pitch, roll=roll,
                                                brighten=1.0 + 0.05 * i, lens=LENS), px, DEGREE))
    return out


def run(name, nch, srcs):
    yprs = [(5.0 * k, 0.0, 0.0) for k in range(N)]
    row, frame = W * nch * 4, W * H * nch * 4
    out_a, out_b = malloc(N * frame), malloc(N * frame)
    try:
        arr = (C.c_void_p * len(srcs))(*[s.handle for s in srcs])
        # (a): one target per view, built beforehand
        jobs_a = [ea.arguments(ea.RECTILINEAR, W, H, HFOV, yaw=y, pitch=p, roll=r, spline_degree=DEGREE) for y, p, r in yprs]
        targets = [a.target(nch) for a in jobs_a]
        dst = [C.c_void_p(out_a.value + k * frame) for k in range(N)]
        # (b): the shared target and the view array
        shared = ea.arguments(ea.RECTILINEAR, W, H, HFOV, spline_degree=DEGREE)
        t = shared.target(nch)
        views = ea.api._views_struct(shared, yprs)

        def loop_ms():
            t0 = time.perf_counter()
            for k in range(N):
                rc = L.eu_hip_render(C.byref(targets[k]), arr, len(srcs), dst[k], row, 1, None)
                if rc:
                    ea.api._check(rc)
            ea.api._check(L.eu_hip_sync())
            return (time.perf_counter() - t0) * 1e3

        def views_ms():
            t0 = time.perf_counter()
            rc = L.eu_hip_render_views_multi(C.byref(t), views, N, arr, len(srcs), out_b, row, frame, 1, None)
            ea.api._check(rc)
            ea.api._check(L.eu_hip_sync())
            return (time.perf_counter() - t0) * 1e3

        loop_ms(), views_ms()                      # one warm-up each
        a_ms, b_ms = [], []
        for _ in range(opt.reps):
            a_ms.append(loop_ms())
            b_ms.append(views_ms())
        fa, fb = download(out_a, N * frame), download(out_b, N * frame)
        if not bool((fa == fb).all()):
            sys.exit(f"{name}: the frames of the two ways differ - no timing is kept")
        sa, sb = stats(a_ms), stats(b_ms)
        spread = sa["max"] - sa["min"]
        return {"job": name, "facets": f"{len(srcs)} fisheye 140 deg, {FW}x{FH}, {nch} channels, lens polynomial",
                "degree": DEGREE, "views": N, "view": f"{W}x{H}", "repetitions": opt.reps, "frames_equal": True,
                "nonzero_share": round(float((fb.reshape(-1, nch) != 0).any(axis=1).mean()), 4),
                "loop_of_render_ms": sa, "render_views_multi_ms": sb,
                "loop_spread_ms": round(spread, 4),
                "views_median_below_loop_min_by_more_than_spread": bool(sa["min"] - sb["median"] > spread),
                "per_view_us": {"loop_median": round(1e3 * sa["median"] / N, 2), "views_median": round(1e3 * sb["median"] / N, 2)},
                "all_ms_loop": [round(v, 4) for v in a_ms], "all_ms_views": [round(v, 4) for v in b_ms]}
    finally:
        L.eu_hip_free(out_a)
        L.eu_hip_free(out_b)


results = []
for name, nch in (("64 x 256x256, six RGB facets", 3), ("64 x 256x256, six RGBA facets", 4)):
    results.append(run(name, nch, facets(nch)))
    print(json.dumps(results[-1]), flush=True)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
