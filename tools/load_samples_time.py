"""Load of an 8-bit image, host samples -> a ready source, by the two routes the library has:
(a) widen and linearise on the host, then the float load: table[samples] with numpy.take, then Source.load;
(b) Source.load_samples: the samples go up as they are, the same table is looked up on the device.
8192 x 4096 x 3, 8 bit, sRGB -> Linear, degree 3. Both loads are synchronous, so a host clock around them is
valid. (a)'s host step is a table gather, far cheaper than the command line's one powf per colour sample - so (a)
is timed in its favour. The routes alternate in one process, one warm-up each, then five repetitions each.
Prints min and median of both in ms as one JSON line; --out FILE keeps it.
    python tools/load_samples_time.py [--out profiles/load_samples_times.json] [--reps 5] [--only b]"""
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
ap.add_argument("--width", type=int, default=8192)
ap.add_argument("--only", choices=["a", "b"], help="one route alone, once (for a kernel trace)")
opt = ap.parse_args()

W, H, NCH = opt.width, opt.width // 2, 3
rng = np.random.default_rng(2026)
samples = rng.integers(0, 256, (H, W, NCH), dtype=np.uint8)
v = np.arange(256, dtype=np.float32) / np.float32(255)
table = np.where(v <= np.float32(0.04045), v / np.float32(12.92),
                 np.power((v + np.float32(0.055)) / np.float32(1.055), np.float32(2.4))).astype(np.float32)
fct = ea.facet_spec(ea.SPHERICAL, W, H, 360.0, nchannels=NCH)


def route_a():
    t0 = time.perf_counter()
    px = np.take(table, samples)
    t1 = time.perf_counter()
    src = ea.Source.load(fct, px, opt.degree)
    t2 = time.perf_counter()
    src.release()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3


def route_b():
    t0 = time.perf_counter()
    src = ea.Source.load_samples(fct, samples, table, spline_degree=opt.degree)
    t1 = time.perf_counter()
    src.release()
    return (t1 - t0) * 1e3, 0.0


if opt.only:
    print(json.dumps({opt.only + "_ms": round({"a": route_a, "b": route_b}[opt.only]()[0], 3)}))
    sys.exit(0)
route_a(), route_b()
a, b = [], []
for _ in range(opt.reps):
    a.append(route_a())
    b.append(route_b())


def stats(x):
    return {"min": round(min(x), 3), "median": round(statistics.median(x), 3)}


res = {"source": f"{W}x{H}x{NCH}", "bits": 8, "colour": "sRGB -> Linear", "degree": opt.degree, "reps": opt.reps,
       "a_host_take_then_load_ms": stats([t for t, _ in a]),
       "a_host_take_alone_ms": stats([g for _, g in a]),
       "b_load_samples_ms": stats([t for t, _ in b]),
       "b_median_below_a_median": statistics.median([t for t, _ in b]) < statistics.median([t for t, _ in a])}
line = json.dumps(res)
print(line)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(line + "\n")
