"""What a geometry the library has not seen costs on its first frame: the plans of a lat/lon job are built when the
plan key changes (host: the tile rows' plan ids, the first loop's groups; device: the column tables and - since the
second loop reads its tile boxes from a table - eu5_boxplan_kernel), and cached after that.
The headline's source geometry (16384 x 8192 lat/lon, cubic, RGB; the container is allocated, not filled: no
coordinate depends on a pixel) rendered to cubemaps of several face sizes, device to device. Per face size the host
clock brackets the first eu_hip_render + eu_hip_sync and, after it, the mean of 20 cached frames. The first face
size warms the process up (kernel load, stream, queues) and is not reported.
Prints one JSON line; run it once per library (EU_HIP_LIB) for an A/B.
    python tools/first_frame_time.py [--out FILE] [--faces 4000 4096 4064 4032]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import envutil_amd as ea  # noqa: E402
from envutil_amd.api import lib_path  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--faces", type=int, nargs="+", default=[4000, 4096, 4064, 4032])
opt = ap.parse_args()

import torch  # noqa: E402

dev = torch.device("cuda:0")
L = ea.lib()
L.eu_hip_init(0)
NCH, DEG = 3, 3
src = ea.Source.alloc(ea.facet_spec(ea.SPHERICAL, 16384, 8192, 360.0, nchannels=NCH), DEG)
srcs = (C.c_void_p * 1)(src.handle)
out = torch.empty((6 * max(opt.faces), max(opt.faces), NCH), device=dev, dtype=torch.float32)
st = torch.cuda.Stream(device=dev)
with torch.cuda.stream(st):
    torch.zeros(1, device=dev)
st.synchronize()


def frame(tgt, face):
    rc = L.eu_hip_render(C.byref(tgt), srcs, 1, C.c_void_p(out.data_ptr()), face * NCH * 4, 1, C.c_void_p(st.cuda_stream))
    if rc:
        raise SystemExit("render failed: " + L.eu_hip_last_error().decode())
    L.eu_hip_sync()
    st.synchronize()


res = []
for k, face in enumerate(opt.faces):
    args = ea.arguments(ea.CUBEMAP, face, 6 * face, 90.0, spline_degree=DEG)
    tgt = args.target(NCH, 0, 6 * face, 0, None)
    t0 = time.perf_counter()
    frame(tgt, face)
    t1 = time.perf_counter()
    for _ in range(20):
        frame(tgt, face)
    t2 = time.perf_counter()
    if k:
        res.append({"face": face, "first_ms": round((t1 - t0) * 1e3, 3), "cached_ms": round((t2 - t1) * 1e3 / 20, 3)})
line = json.dumps({"lib": os.path.basename(lib_path()), "source": "16384x8192", "degree": DEG, "frames": res})
print(line)
if opt.out:
    with open(opt.out, "a") as f:
        f.write(line + "\n")
