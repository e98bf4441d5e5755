"""eu_hip_render_layers on L pictures of one geometry against the same pictures as a loop of L eu_hip_render calls,
in one process, into device memory:
    (a) the loop under EU_HIP_R4=0 EU_HIP_HYBRID=0: the same coordinate and evaluation code in single-picture form;
    (b) the loop with default switches: what a caller has today, staged kernels included.
Jobs:
    an 8192 x 4096 lat/lon RGB source -> 6 x 2048 cubemap, bilinear and cubic, L = 2, 4, 8;
    a 4096 x 2048 source -> 1920 x 1080 rectilinear, rotated, cubic, untwined and with --twine 4, L = 2, 4, 8;
    the headline shape - 16384 x 8192 -> 6 x 4096 cubemap, cubic, what bench.py times - at L = 2.
Every layer is a container of its own (the same pixels: what is timed does not look at them, and L distinct
containers are what fills the caches). What is measured is the host's wall clock around ten iterations plus
eu_hip_sync(), divided by ten; the ways alternate in seven pairs after one warm-up each; min, median and max of the
seven are reported. The first and last 256 rows of every layer are compared bit for bit between the ways.
The layered call runs with the switches the process was started with: every result records the EU_HIP_LAYERS_MAX
in force ("layers_max": null is the library's default) and the library's EU_LAYERS_GROUP. With --sweep the call is
also timed under EU_HIP_LAYERS_MAX = 1, 2, 4, 8 and 0 (all) at the job's largest L. --variants NAME=LIBRARY,... runs
the twined job again in a child process per library (EU_HIP_LIB; built by tools/mkvariant.sh NAME eu_render_layers
"-DEU_LAYERS_GROUP=n") and keeps its rows under "variants".
Prints one JSON line per (job, L); --out FILE keeps everything: {"commit", "tree_modified", "results", "variants"}.
    python tools/layers_time.py [--out profiles/layers_times.json] [--sweep] [--variants g2=PATH,g4=PATH]
                                [--only WORD] [--small] [--commit HASH --modified]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import envutil_amd as ea  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--only", default="")
ap.add_argument("--variants", default="", help="NAME=LIBRARY,...: the twined job again with EU_HIP_LIB=LIBRARY")
ap.add_argument("--commit", help="the commit the tree is based on, where the tool cannot ask git")
ap.add_argument("--modified", action="store_true", help="... and the tree differs from it")
ap.add_argument("--small", action="store_true", help="sources and targets at a quarter of the size in each direction (a dry run)")
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
opt = ap.parse_args()
if ea.device_count() < 1:
    sys.exit("layers_time.py needs a HIP device: there is nothing to time without one")

Q = 4 if opt.small else 1
# name, source width, target (projection, width, height, hfov), orientation, degree, twine, layer counts
CUBE, RECT, TURNED = (ea.CUBEMAP, 2048 // Q, 6 * 2048 // Q, 90.0), (ea.RECTILINEAR, 1920 // Q, 1080 // Q, 90.0), (30.0, 15.0, 7.5)
JOBS = [("8192x4096 -> cubemap 2048, bilinear", 8192 // Q, CUBE, (0.0, 0.0, 0.0), 1, 0, (2, 4, 8)),
        ("8192x4096 -> cubemap 2048, cubic", 8192 // Q, CUBE, (0.0, 0.0, 0.0), 3, 0, (2, 4, 8)),
        ("4096x2048 -> rectilinear 1920x1080 rotated, cubic", 4096 // Q, RECT, TURNED, 3, 0, (2, 4, 8)),
        ("4096x2048 -> rectilinear 1920x1080 rotated, cubic, twine 4", 4096 // Q, RECT, TURNED, 3, 4, (2, 4, 8)),
        ("16384x8192 -> cubemap 4096, cubic: the headline shape", 16384 // Q, (ea.CUBEMAP, 4096 // Q, 6 * 4096 // Q, 90.0),
         (0.0, 0.0, 0.0), 3, 0, (2,))]
L = ea.lib()
GROUP = int(L.eu_hip_layers_group())
LAYERS_MAX = os.environ.get("EU_HIP_LAYERS_MAX") or None     # what the layered call runs under outside the sweep
SWITCHES = ("EU_HIP_R4", "EU_HIP_HYBRID", "EU_HIP_LAYERS_MAX")


def switches(**kw):
    for k in SWITCHES:
        os.environ.pop(k, None)
    if LAYERS_MAX is not None and "EU_HIP_LAYERS_MAX" not in kw:
        os.environ["EU_HIP_LAYERS_MAX"] = LAYERS_MAX
    os.environ.update({k: str(v) for k, v in kw.items()})


def malloc(nbytes):
    p = C.c_void_p()
    ea.api._check(L.eu_hip_malloc(C.byref(p), nbytes))
    return p


def download(dev, offset, nbytes):
    out = np.zeros(nbytes // 4, np.uint32)
    ea.api._check(L.eu_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev.value + offset), nbytes))
    return out


def stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def run(name, layers, target, ypr, degree, twine, sweep):
    n = len(layers)
    prj, w, h, hfov = target
    a = ea.arguments(prj, w, h, hfov, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree, twine=twine)
    t = a.target(3)
    row, frame = w * 3 * 4, w * h * 3 * 4
    out_a, out_b = malloc(n * frame), malloc(n * frame)
    try:
        one = [(C.c_void_p * 1)(s.handle) for s in layers]
        dst = [C.c_void_p(out_a.value + k * frame) for k in range(n)]
        handles = (C.c_void_p * n)(*[s.handle for s in layers])

        def loop_ms(**sw):
            switches(**sw)
            t0 = time.perf_counter()
            for _ in range(opt.iters):
                for k in range(n):
                    rc = L.eu_hip_render(C.byref(t), one[k], 1, dst[k], row, 1, None)
                    if rc:
                        ea.api._check(rc)
            ea.api._check(L.eu_hip_sync())
            return (time.perf_counter() - t0) * 1e3 / opt.iters

        def layers_ms(**sw):
            switches(**sw)
            t0 = time.perf_counter()
            for _ in range(opt.iters):
                rc = L.eu_hip_render_layers(C.byref(t), handles, n, out_b, row, frame, 1, None)
                if rc:
                    ea.api._check(rc)
            ea.api._check(L.eu_hip_sync())
            return (time.perf_counter() - t0) * 1e3 / opt.iters

        def same_rows():
            rows = min(256, h) * row
            for k in range(n):
                for off in (k * frame, k * frame + frame - rows):
                    if not (download(out_a, off, rows) == download(out_b, off, rows)).all():
                        return False
            return True

        plain = dict(EU_HIP_R4=0, EU_HIP_HYBRID=0)
        loop_ms(**plain), loop_ms(), layers_ms()             # one warm-up each
        a_ms, b_ms, l_ms = [], [], []
        for _ in range(opt.pairs):
            a_ms.append(loop_ms(**plain))
            l_ms.append(layers_ms())
        same = same_rows()                                  # out_a holds (a)'s frames here
        for _ in range(opt.pairs):
            b_ms.append(loop_ms())
            l_ms.append(layers_ms())
        same = same and same_rows()                         # ... and (b)'s here
        if not same:
            sys.exit(f"{name}, {n} layers: the frames of the ways differ - no timing is kept")
        sa, sb, sl = stats(a_ms), stats(b_ms), stats(l_ms)
        res = {"job": name, "layers": n, "degree": degree, "twine": twine, "target": f"{w}x{h}", "pairs": opt.pairs,
               "iterations": opt.iters, "rows_equal": same, "library": os.path.basename(ea.lib_path()),
               "layers_group": GROUP, "layers_max": LAYERS_MAX,
               "loop_plain_ms": sa, "loop_default_ms": sb, "render_layers_ms": sl,
               "loop_plain_spread_ms": round(sa["max"] - sa["min"], 4),
               "layers_over_loop_plain": round(sl["median"] / sa["median"], 4),
               "layers_over_loop_default": round(sl["median"] / sb["median"], 4),
               "no_slower_than_loop_plain_by_more_than_its_spread": bool(sl["median"] - sa["median"] <= sa["max"] - sa["min"])}
        if sweep:
            res["layers_max_sweep_ms"] = {}
            for most in (1, 2, 4, 8, 0):
                layers_ms(EU_HIP_LAYERS_MAX=most)
                res["layers_max_sweep_ms"]["all" if not most else str(most)] = \
                    stats([layers_ms(EU_HIP_LAYERS_MAX=most) for _ in range(opt.pairs)])
        switches()
        return res
    finally:
        L.eu_hip_free(out_a)
        L.eu_hip_free(out_b)


def git(*argv):
    try:
        r = subprocess.run(["git", "-C", ROOT] + list(argv), capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 else None
    except OSError:
        return None


commit = opt.commit or git("rev-parse", "HEAD")
modified = True if opt.modified else (None if opt.commit or commit is None else bool(git("status", "--porcelain")))
results = []
pixels = {}
for name, sw, target, ypr, degree, twine, counts in JOBS:
    if opt.only and opt.only not in name:
        continue
    if sw not in pixels:
        pixels.clear()
        pixels[sw] = np.random.default_rng(12345).random((sw // 2, sw, 3), dtype=np.float32)
    fct = ea.facet_spec(ea.SPHERICAL, sw, sw // 2, 360.0, nchannels=3)
    layers = [ea.Source.load(fct, pixels[sw], degree) for _ in range(max(counts))]
    for n in counts:
        results.append(run(name, layers[:n], target, ypr, degree, twine, opt.sweep and n == max(counts) and n > 2))
        print(json.dumps(results[-1]), flush=True)
    for s in layers:
        s.release()
variants = {}
for item in filter(None, opt.variants.split(",")):
    vname, path = item.split("=", 1)
    argv = [sys.executable, os.path.abspath(__file__), "--only", "twine", "--pairs", str(opt.pairs), "--iters", str(opt.iters)]
    r = subprocess.run(argv + (["--small"] if opt.small else []), env=dict(os.environ, EU_HIP_LIB=os.path.abspath(path)),
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"variant {vname}: {r.stdout[-500:]} {r.stderr[-500:]}")
    variants[vname] = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    for row in variants[vname]:
        print(json.dumps(dict(row, variant=vname)), flush=True)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump({"commit": commit, "tree_modified": modified, "small": opt.small, "results": results, "variants": variants}, f, indent=1)
        f.write("\n")
