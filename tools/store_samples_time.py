"""A rendered frame as 8-bit samples in host memory, by the two routes the library has:
(a) render to host floats, then the cheap host form of the quantiser, (clip(v, 0, 1) * 255 + 0.5).astype(uint8);
(b) render_samples: the frame is encoded on the device and leaves it as bytes.
A resident 8192 x 4096 x 3 source, degree 3, to the 6 x 2048 cubemap and to the headline's 6 x 4096. Both calls are
synchronous, so a host clock around them is valid. (a)'s host step is one multiply-add per sample, far cheaper than
the command line's one powf per colour sample - so (a) is timed in its favour. The routes alternate in one process,
one warm-up each, then five repetitions each. (a), the existing path, is the yardstick: the median of (b) has to lie
below the minimum of (a) by more than (a)'s spread, max - min. Prints one JSON line; --out FILE keeps it.
    python tools/store_samples_time.py [--out profiles/store_samples_times.json] [--reps 5] [--faces 2048 4096]
    python tools/store_samples_time.py --only b --faces 4096 [--bits 16]      (one route alone, for a kernel trace)"""
import argparse
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--degree", type=int, default=3)
ap.add_argument("--width", type=int, default=8192, help="of the lat/lon source")
ap.add_argument("--faces", type=int, nargs="+", default=[2048, 4096])
ap.add_argument("--bits", type=int, default=8, choices=[8, 16])
ap.add_argument("--only", choices=["a", "b"], help="one route alone, twice (for a kernel trace)")
opt = ap.parse_args()

W, H, NCH = opt.width, opt.width // 2, 3
x = np.arange(W, dtype=np.float32)[None, :, None]
y = np.arange(H, dtype=np.float32)[:, None, None]
c = np.arange(NCH, dtype=np.float32)[None, None, :]
# a smooth field that leaves [0, 1] on both sides, so that the clamp has work
img = (np.float32(0.5) + np.float32(0.65) * np.sin(x * (np.float32(0.003) + np.float32(0.001) * c)) * np.cos(y * np.float32(0.005))).astype(np.float32)
src = ea.Source.load(ea.facet_spec(ea.SPHERICAL, W, H, 360.0, nchannels=NCH), img, opt.degree)
del img, x, y, c
MAXVAL = (1 << opt.bits) - 1
DT = np.uint8 if opt.bits == 8 else np.uint16
steps = ea.sample_steps(opt.bits)


def route_a(args, frame, out):
    t0 = time.perf_counter()
    ea.render(args, src, out=frame)
    t1 = time.perf_counter()
    np.clip(frame, 0, 1, out=frame)
    frame *= np.float32(MAXVAL)
    frame += np.float32(0.5)
    out[...] = frame.astype(DT)
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3


def route_b(args, frame, out):
    t0 = time.perf_counter()
    ea.render_samples(args, src, colour_steps=steps, bits=opt.bits, out=out)
    t1 = time.perf_counter()
    return (t1 - t0) * 1e3, 0.0


def stats(x):
    return {"min": round(min(x), 3), "median": round(statistics.median(x), 3), "max": round(max(x), 3)}


res = {"source": f"{W}x{H}x{NCH}", "bits": opt.bits, "degree": opt.degree, "reps": opt.reps, "targets": {}}
for face in opt.faces:
    args = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=opt.degree)
    frame = np.zeros((6 * face, face, NCH), np.float32)
    out_a = np.zeros((6 * face, face, NCH), DT)
    out_b = np.zeros((6 * face, face, NCH), DT)
    if opt.only:
        route = {"a": route_a, "b": route_b}[opt.only]
        route(args, frame, out_a)
        res["targets"][f"6x{face}"] = {opt.only + "_ms": round(route(args, frame, out_a)[0], 3)}
        continue
    route_a(args, frame, out_a), route_b(args, frame, out_b)
    a, b = [], []
    for _ in range(opt.reps):
        a.append(route_a(args, frame, out_a))
        b.append(route_b(args, frame, out_b))
    ta, tb = [t for t, _ in a], [t for t, _ in b]
    res["targets"][f"6x{face}"] = {
        "a_render_floats_then_host_quantise_ms": stats(ta),
        "a_host_quantise_alone_ms": stats([g for _, g in a]),
        "b_render_samples_ms": stats(tb),
        "same_bytes": bool(np.array_equal(out_a, out_b)),
        "b_median_below_a_min_by_more_than_a_spread": statistics.median(tb) < min(ta) - (max(ta) - min(ta)),
    }
    del frame, out_a, out_b
line = json.dumps(res)
print(line)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(line + "\n")
