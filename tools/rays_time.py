"""The ray form against the packed render launch it shares its coordinate and evaluation code with.
For the headline job (16384 x 8192 lat/lon, cubic, to 6 x 4096) and the bilinear job of config 2 (8192 x 4096 to
6 x 2048): the job's stage-1 rays are written to device memory once; then eu_hip_render_rays_timed on them
(eu_rays2_kernel: reads 12 bytes of ray per pixel) alternates, in pairs in one process, with eu_hip_render_timed of
the same job under EU_HIP_R4=0 EU_HIP_HYBRID=0 (eu_render2_kernel in one launch: reads the stepper tables and forms
the rays itself). Both write the same frame; the first and last rows of the two frames are compared bit for bit.
Prints one JSON line per job; --out FILE keeps them (a JSON list).
    python tools/rays_time.py [--out profiles/rays_times.json] [--pairs 7] [--iters 10] [--only headline|config2]
    python tools/rays_time.py --only headline --form rays --pairs 1      (one form alone, for a kernel trace)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import envutil_amd as ea  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--only", choices=["headline", "config2"])
ap.add_argument("--form", choices=["rays", "packed"], help="time one form alone")
opt = ap.parse_args()

JOBS = {"headline": (16384, 8192, 4096, 3), "config2": (8192, 4096, 2048, 1)}     # source w, h; face; degree
L = ea.lib()


def malloc(nbytes):
    p = C.c_void_p()
    ea.api._check(L.eu_hip_malloc(C.byref(p), nbytes))
    return p


def rows_of(dev, row_bytes, first, count):
    out = np.zeros((count, row_bytes // 4), np.float32)
    ea.api._check(L.eu_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(dev.value + first * row_bytes),
                                      out.nbytes))
    return out.view(np.uint32)


def packed_ms(a, src, out):
    keep = {k: os.environ.get(k) for k in ("EU_HIP_R4", "EU_HIP_HYBRID")}
    os.environ["EU_HIP_R4"], os.environ["EU_HIP_HYBRID"] = "0", "0"
    try:
        return ea.render_timed(a, src, out.value, opt.iters)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run(name):
    sw, sh, face, degree = JOBS[name]
    tw, th = face, 6 * face
    px = np.random.default_rng(12345).random((sh, sw, 3), dtype=np.float32)
    src = ea.Source.load(ea.facet_spec(ea.SPHERICAL, sw, sh, 360.0, nchannels=3), px, degree)
    del px
    a = ea.arguments(ea.CUBEMAP, tw, th, 90.0, spline_degree=degree)
    row = tw * 3 * 4
    rays, out_r, out_p = malloc(th * row), malloc(th * row), malloc(th * row)
    try:
        t = a.target(3, stage=1)
        arr = (C.c_void_p * 1)(src.handle)
        ea.api._check(L.eu_hip_render(C.byref(t), arr, 1, rays, row, 1, None))
        ea.sync()
        r = ea.Rays()
        r.width, r.height, r.ninputs, r.nchannels = tw, th, 3, 3
        r.rays, r.ray_row_stride_bytes, r.rays_on_device = rays.value, row, 1

        def rays_ms():
            ms = C.c_float()
            ea.api._check(L.eu_hip_render_rays_timed(C.byref(r), src.handle, out_r, row, opt.iters, C.byref(ms)))
            return ms.value

        pairs = []
        for _ in range(opt.pairs):
            pairs.append([round(rays_ms(), 4) if opt.form != "packed" else None,
                          round(packed_ms(a, src, out_p), 4) if opt.form != "rays" else None])
        res = {"job": name, "source": f"{sw}x{sh} lat/lon RGB", "target": f"6x{face} cubemap", "degree": degree,
               "iters_per_measurement": opt.iters, "pairs_ms_rays_packed": pairs}
        if opt.form is None:
            same = all((rows_of(out_r, row, y0, 256) == rows_of(out_p, row, y0, 256)).all() for y0 in (0, th - 256))
            ra, pa = [p[0] for p in pairs], [p[1] for p in pairs]
            ratios = [x / y for x, y in pairs]
            res.update(frames_equal_first_last_256_rows=bool(same),
                       rays_ms={"min": min(ra), "median": statistics.median(ra), "max": max(ra)},
                       packed_ms={"min": min(pa), "median": statistics.median(pa), "max": max(pa)},
                       ratio_rays_over_packed={"min": round(min(ratios), 4), "median": round(statistics.median(ratios), 4),
                                               "max": round(max(ratios), 4)})
        return res
    finally:
        for p in (rays, out_r, out_p):
            L.eu_hip_free(p)
        src.release()


results = []
for name in ([opt.only] if opt.only else list(JOBS)):
    results.append(run(name))
    print(json.dumps(results[-1]), flush=True)
if opt.out:
    with open(opt.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
