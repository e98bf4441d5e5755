"""A rendered frame to the planes of a Y'CbCr frame: the encode kernel alone, and the render into host planes.
Device: the 6 x 4096 cubemap frame (3 channels) in device memory into device planes - encode_ycbcr to NV12, I420 and
I444 at 8 bit and to P010 - beside encode_samples to RGB8 of the same frame, the cheapest 8-bit way out there was,
in the same run: 200 launches between two events on a torch stream after a warm-up, repeated, the median reported. The
algorithmic bytes per pixel are 4 * 3 + (1 + 2 / (sub_x * sub_y)) * bits / 8.
Host: a resident 8192 x 4096 x 3 source, degree 3, to the 6 x 4096 cubemap as host NV12 planes (render_ycbcr) against
host RGB8 samples (render_samples): both calls are synchronous, a host clock around them is valid; the routes
alternate, one warm-up each.
Prints one JSON line; --out FILE keeps it.
    python tools/ycbcr_out_time.py [--out profiles/ycbcr_out_times.json] [--commit ID] [--reps 5]
    python tools/ycbcr_out_time.py --only device --device-iters 20       (for a kernel trace)"""
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
ap.add_argument("--face", type=int, default=4096)
ap.add_argument("--device-iters", type=int, default=200)
ap.add_argument("--only", choices=["device", "host"], help="one part alone")
opt = ap.parse_args()

W, H = opt.width, opt.width // 2
face = opt.face


def stats(x):
    return {"min": round(min(x), 3), "median": round(statistics.median(x), 3), "max": round(max(x), 3)}


x = np.arange(W, dtype=np.float32)[None, :, None]
y = np.arange(H, dtype=np.float32)[:, None, None]
c = np.arange(3, dtype=np.float32)[None, None, :]
# a smooth picture that leaves [0, 1] on both sides: every code of the tables has work
img = (np.float32(0.5) + np.float32(0.6) * np.sin(x * (np.float32(0.003) + np.float32(0.001) * c)) * np.cos(y * np.float32(0.005))).astype(np.float32)
src = ea.Source.load(ea.facet_spec(ea.SPHERICAL, W, H, 360.0), img, opt.degree)
del img, x, y, c
args = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=opt.degree)
fw = ea.ycbcr_forward("709")
res = {"commit": opt.commit, "frame": f"6x{face}x3", "degree": opt.degree, "reps": opt.reps}
rows, npix = 6 * face, 6 * face * face
steps8 = ea.ycbcr_steps(8)
rgb_steps = ea.sample_steps(8)

if opt.only in (None, "device"):
    import torch
    frame = torch.from_numpy(ea.render(args, src)).cuda()
    stream = torch.cuda.Stream()
    steps10 = ea.ycbcr_steps(16, 10)

    def planes(sub, inter, dt):
        ch, cw = (rows + sub[1] - 1) // sub[1], (face + sub[0] - 1) // sub[0]
        yp = torch.empty((rows, face), dtype=dt, device="cuda")
        if inter:
            return yp, torch.empty((ch, cw, 2), dtype=dt, device="cuda")
        return yp, (torch.empty((ch, cw), dtype=dt, device="cuda"), torch.empty((ch, cw), dtype=dt, device="cuda"))

    def ycbcr_call(sub, inter, bits, shift, steps):
        out = planes(sub, inter, torch.uint8 if bits == 8 else torch.uint16)
        return lambda: ea.encode_ycbcr(frame, fw, sub, interleaved=inter, bits=bits, shift=shift, y_steps=steps[0],
                                       c_steps=steps[1], out=out, stream=stream)

    samples = torch.empty((rows, face, 3), dtype=torch.uint8, device="cuda")
    calls = {"encode_samples_rgb8": (lambda: ea.encode_samples(frame, rgb_steps, out=samples, stream=stream.cuda_stream), 15.0),
             "encode_ycbcr_nv12": (ycbcr_call((2, 2), True, 8, 0, steps8), 13.5),
             "encode_ycbcr_i420": (ycbcr_call((2, 2), False, 8, 0, steps8), 13.5),
             "encode_ycbcr_i444": (ycbcr_call((1, 1), False, 8, 0, steps8), 15.0),
             "encode_ycbcr_p010": (ycbcr_call((2, 2), True, 16, 6, steps10), 15.0)}
    res["device"] = {"iters": opt.device_iters}
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
    yd, cd = ea.encode_ycbcr(frame, fw, interleaved=True, y_steps=steps8[0], c_steps=steps8[1])
    yh, ch = ea.ycbcr_planes(frame.cpu().numpy(), fw, interleaved=True, y_steps=steps8[0], c_steps=steps8[1])
    res["device"]["same_bytes_as_the_host_form"] = bool(np.array_equal(yd.cpu().numpy(), yh) and np.array_equal(cd.cpu().numpy(), ch))
    del frame

if opt.only in (None, "host"):
    yh = np.zeros((rows, face), np.uint8)
    ch = np.zeros((rows // 2, face // 2, 2), np.uint8)
    rgb = np.zeros((rows, face, 3), np.uint8)

    def route_a():
        t0 = time.perf_counter()
        ea.render_samples(args, src, colour_steps=rgb_steps, out=rgb)
        return (time.perf_counter() - t0) * 1e3

    def route_b():
        t0 = time.perf_counter()
        ea.render_ycbcr(args, src, fw, interleaved=True, y_steps=steps8[0], c_steps=steps8[1], out=(yh, ch))
        return (time.perf_counter() - t0) * 1e3

    route_a(), route_b()
    a, b = [], []
    for _ in range(opt.reps):
        a.append(route_a())
        b.append(route_b())
    res["host"] = {"a_render_samples_rgb8_ms": stats(a), "b_render_ycbcr_nv12_ms": stats(b),
                   "bytes_to_the_host": {"a": rgb.nbytes, "b": yh.nbytes + ch.nbytes},
                   "b_median_below_a_min_by_more_than_a_spread": bool(statistics.median(b) < min(a) - (max(a) - min(a)))}

line = json.dumps(res)
print(line)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(line + "\n")
