"""Load of a masked and cropped facet, host pixels -> a ready source, by the two routes the library has:
(a) the host edit and the plain load: eu_hip_facet_alpha, then eu_hip_source_load;
(b) eu_hip_source_load_edited: upload at the image's own channel count, the edit on the device.
A 4096 x 3072 facet, 3 -> 4 channels, two polygons and an elliptic crop. Both loads are synchronous, so a host
clock around them is valid. The routes alternate in one process, one warm-up each, then five repetitions each.
(a) is given the pixels already widened to four channels (a fresh copy per repetition, made outside the clock:
the host function edits in place), which the host route has to do as well - so (a) is timed in its favour.
Prints min and median of both in ms as one JSON line; --out FILE keeps it.
    python tools/facet_edit_time.py [--out profiles/facet_edit_load_times.json] [--reps 5] [--only b]"""
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
ap.add_argument("--only", choices=["a", "b"], help="one route alone, once (for a kernel trace)")
opt = ap.parse_args()

W, H, PCH, NCH = 4096, 3072, 3, 4
rng = np.random.default_rng(2026)
px = rng.random((H, W, PCH), dtype=np.float32)
masks = [(np.array([300, 1900, 2300, 700], np.float32), np.array([200, 350, 1500, 1300], np.float32)),
         (np.array([2600.5, 3900, 3500, 2500], np.float32), np.array([1800, 1700.25, 2900, 3000], np.float32))]
crop, kind = (128, 3968, 96, 2976), 2
fct = ea.facet_spec(ea.FISHEYE, W, H, 150.0, nchannels=NCH)
wide = np.concatenate([px, np.ones((H, W, 1), np.float32)], 2)


def route_a():
    p = wide.copy()
    t0 = time.perf_counter()
    ea.facet_alpha(p, masks, crop, kind)
    src = ea.Source.load(fct, p, opt.degree)
    t1 = time.perf_counter()
    src.release()
    return (t1 - t0) * 1e3


def route_b():
    t0 = time.perf_counter()
    src = ea.Source.load(fct, px, opt.degree, masks=masks, crop=crop, crop_kind=kind)
    t1 = time.perf_counter()
    src.release()
    return (t1 - t0) * 1e3


if opt.only:
    print(json.dumps({opt.only + "_ms": round({"a": route_a, "b": route_b}[opt.only](), 3)}))
    sys.exit(0)
route_a(), route_b()
a, b = [], []
for _ in range(opt.reps):
    a.append(route_a())
    b.append(route_b())
res = {"facet": f"{W}x{H}", "channels": f"{PCH}->{NCH}", "polygons": len(masks), "crop": "elliptic",
       "degree": opt.degree, "reps": opt.reps,
       "a_host_edit_then_load_ms": {"min": round(min(a), 3), "median": round(statistics.median(a), 3)},
       "b_load_edited_ms": {"min": round(min(b), 3), "median": round(statistics.median(b), 3)},
       "b_median_below_a_min": statistics.median(b) < min(a)}
line = json.dumps(res)
print(line)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(line + "\n")
