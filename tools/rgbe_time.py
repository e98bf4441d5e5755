"""Radiance RGBE pixels to a ready source and a rendered frame to RGBE pixels in host memory, each by the two routes
the library has, and the encode kernel alone.
Load, random 8192 x 4096 quads, degree 3:
(a) decode on the host - mantissa * scale[E] in numpy, one multiply per channel, the decode timed separately - then
    Source.load of the floats;  (b) Source.load_rgbe: the quads go up as they are.
Store, a resident 8192 x 4096 x 3 source, degree 3, to the 6 x 2048 and the 6 x 4096 cubemap:
(a) render to host floats, then a vectorised numpy form of the encoder (float32 throughout, the encode timed
    separately);  (b) render_rgbe: the frame is encoded on the device and leaves it as quads.
All four calls are synchronous, so a host clock around them is valid. (a)'s host steps are vectorised numpy, far
cheaper than the command line's one pixel after the other on one thread - so (a) is timed in its favour. The routes
alternate in one process, one warm-up each, then five repetitions each. (a), the existing path, is the yardstick:
the median of (b) has to lie below the minimum of (a) by more than (a)'s spread, max - min.
Device alone: encode_rgbe of the 6 x 4096 frame in device memory into a device buffer, beside encode_samples at 8
bits on the same frame, between two events on a torch stream; the kernels move 16 and 15 bytes per pixel.
Prints one JSON line; --out FILE keeps it.
    python tools/rgbe_time.py [--out profiles/rgbe_times.json] [--commit ID] [--reps 5] [--faces 2048 4096]
    python tools/rgbe_time.py --only load_b | store_b | device     (one part alone, for a kernel trace)"""
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
ap.add_argument("--commit", default="?", help="recorded in the result")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--degree", type=int, default=3)
ap.add_argument("--width", type=int, default=8192, help="of the lat/lon source")
ap.add_argument("--faces", type=int, nargs="+", default=[2048, 4096])
ap.add_argument("--device-face", type=int, default=4096)
ap.add_argument("--device-iters", type=int, default=200)
ap.add_argument("--only", choices=["load_b", "store_b", "device"], help="one part alone (for a kernel trace)")
opt = ap.parse_args()

W, H = opt.width, opt.width // 2
fct = ea.facet_spec(ea.SPHERICAL, W, H, 360.0)
SCALE = np.concatenate([[0.0], np.ldexp(1.0, np.arange(1, 256) - 136)]).astype(np.float32)      # exact, denormals included
TOP, TINY = np.float32(255.0 * 2.0 ** 119), np.float32(1e-32)


def host_decode(q):
    return q[..., :3].astype(np.float32) * SCALE[q[..., 3]][..., None]


def host_encode(f, out):
    """eu_rgbe_encode in numpy, float32 throughout: the factor 2^(8 - e) from frexp's exponent"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = np.maximum(np.where(f[..., 0] > f[..., 1], f[..., 0], f[..., 1]), f[..., 2])   # (frames here hold no NaN)
        some = v >= TINY
        e = np.frexp(np.minimum(np.where(some, v, np.float32(1.0)), TOP))[1]
        m = np.ldexp(np.float32(1.0), 8 - e).astype(np.float32)
        c = np.minimum(f, TOP) * m[..., None]
        out[..., :3] = np.where(some[..., None] & (f > 0), c, np.float32(0.0)).astype(np.uint8)
        out[..., 3] = np.where(some, e + 128, 0).astype(np.uint8)


def stats(x):
    return {"min": round(min(x), 3), "median": round(statistics.median(x), 3), "max": round(max(x), 3)}


def verdict(ta, tb):
    return bool(statistics.median(tb) < min(ta) - (max(ta) - min(ta)))


res = {"commit": opt.commit, "source": f"{W}x{H}x3", "degree": opt.degree, "reps": opt.reps}

# ---- load ---------------------------------------------------------------------------------------------------------
if opt.only in (None, "load_b"):
    rng = np.random.default_rng(2026)
    quads = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    quads[..., 3] = 112 + quads[..., 3] % 32             # an HDR panorama's range; finite through the prefilter

    def load_a():
        t0 = time.perf_counter()
        px = host_decode(quads)
        t1 = time.perf_counter()
        src = ea.Source.load(fct, px, opt.degree)
        t2 = time.perf_counter()
        return src, (t2 - t0) * 1e3, (t1 - t0) * 1e3

    def load_b():
        t0 = time.perf_counter()
        src = ea.Source.load_rgbe(fct, quads, spline_degree=opt.degree)
        t1 = time.perf_counter()
        return src, (t1 - t0) * 1e3, 0.0

    if opt.only:
        load_b()[0].release()
        s, t, _ = load_b()
        s.release()
        res["load"] = {"b_ms": round(t, 3)}
    else:
        sa, sb = load_a()[0], load_b()[0]
        same = bool(np.array_equal(sa.download().view(np.uint32), sb.download().view(np.uint32)))
        sa.release(), sb.release()
        a, b = [], []
        for _ in range(opt.reps):
            for route, keep in ((load_a, a), (load_b, b)):
                s, t, g = route()
                s.release()
                keep.append((t, g))
        ta, tb = [t for t, _ in a], [t for t, _ in b]
        res["load"] = {"a_host_decode_then_load_ms": stats(ta), "a_host_decode_alone_ms": stats([g for _, g in a]),
                       "b_load_rgbe_ms": stats(tb), "same_container": same,
                       "b_median_below_a_min_by_more_than_a_spread": verdict(ta, tb)}
    del quads

# ---- store and the kernel alone -------------------------------------------------------------------------------------
if opt.only in (None, "store_b", "device"):
    x = np.arange(W, dtype=np.float32)[None, :, None]
    y = np.arange(H, dtype=np.float32)[:, None, None]
    c = np.arange(3, dtype=np.float32)[None, None, :]
    # a smooth field over five decades with a negative part, so that every branch of the encoder has work
    img = (np.exp2(np.float32(8.0) * np.sin(x * (np.float32(0.003) + np.float32(0.001) * c)) * np.cos(y * np.float32(0.005)))
           - np.float32(0.01)).astype(np.float32)
    src = ea.Source.load(fct, img, opt.degree)
    del img, x, y, c

if opt.only in (None, "store_b"):
    def store_a(args, frame, out):
        t0 = time.perf_counter()
        ea.render(args, src, out=frame)
        t1 = time.perf_counter()
        host_encode(frame, out)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3

    def store_b(args, frame, out):
        t0 = time.perf_counter()
        ea.render_rgbe(args, src, out=out)
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, 0.0

    res["store"] = {}
    for face in opt.faces:
        args = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=opt.degree)
        frame = np.zeros((6 * face, face, 3), np.float32)
        out_a = np.zeros((6 * face, face, 4), np.uint8)
        out_b = np.zeros((6 * face, face, 4), np.uint8)
        if opt.only:
            store_b(args, frame, out_b)
            res["store"][f"6x{face}"] = {"b_ms": round(store_b(args, frame, out_b)[0], 3)}
            continue
        store_a(args, frame, out_a), store_b(args, frame, out_b)
        a, b = [], []
        for _ in range(opt.reps):
            a.append(store_a(args, frame, out_a))
            b.append(store_b(args, frame, out_b))
        ta, tb = [t for t, _ in a], [t for t, _ in b]
        res["store"][f"6x{face}"] = {
            "a_render_floats_then_host_encode_ms": stats(ta), "a_host_encode_alone_ms": stats([g for _, g in a]),
            "b_render_rgbe_ms": stats(tb), "same_bytes": bool(np.array_equal(out_a, out_b)),
            "b_median_below_a_min_by_more_than_a_spread": verdict(ta, tb)}
        del frame, out_a, out_b

if opt.only in (None, "device"):
    import torch
    face = opt.device_face
    args = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=opt.degree)
    frame = torch.from_numpy(ea.render(args, src)).cuda()
    npix = 6 * face * face
    quads = torch.empty((6 * face, face, 4), dtype=torch.uint8, device="cuda")
    samples = torch.empty((6 * face, face, 3), dtype=torch.uint8, device="cuda")
    steps = ea.sample_steps(8)
    stream = torch.cuda.Stream()
    calls = {"encode_rgbe": (lambda: ea.encode_rgbe(frame, out=quads, stream=stream.cuda_stream), 16),
             "encode_samples_8_bit": (lambda: ea.encode_samples(frame, steps, out=samples, stream=stream.cuda_stream), 15)}
    res["device"] = {"frame": f"6x{face}", "iters": opt.device_iters}
    for name, (call, nbytes) in calls.items():
        call()
        stream.synchronize()
        runs = []
        for _ in range(opt.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(opt.device_iters):
                call()
            t1.record(stream)
            t1.synchronize()
            runs.append(t0.elapsed_time(t1) / opt.device_iters)
        ms = statistics.median(runs)
        res["device"][name] = {"ms": stats(runs), "bytes_per_pixel": nbytes, "TB_per_s": round(npix * nbytes / (ms * 1e-3) / 1e12, 3)}
    ea.sync()
    res["device"]["same_bytes_as_the_host_form"] = bool(np.array_equal(quads.cpu().numpy(), ea.encode_rgbe(frame.cpu().numpy())))

line = json.dumps(res)
print(line)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(line + "\n")
