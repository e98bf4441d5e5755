#!/usr/bin/env python3
"""A picture that changes, frame after frame, in one resident source: Source.reload* against a new Source.load* per
frame. Frames are NV12 surfaces (and float RGB pictures) that lie on the device, as a decoder leaves them; degree 3.

  load:    a new source per frame - container allocation, scratch, one synchronisation, the old container freed
  reload:  eu_hip_source_reload on a caller's stream; nothing is allocated, freed or waited for between frames

Prints one JSON line: host-clock milliseconds per frame (median over --rounds runs of --frames frames, each run ended
by a device synchronisation) and the algorithmic bytes of the decode, (bytes of the three planes) + 4 * NCH * N_src.
Kernel times come from a profiler run of this script (rocprofv3 --kernel-trace --stats -- python tools/reload_time.py)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import envutil_amd as ea  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if ea.device_count() < 1:
        raise SystemExit("reload_time.py needs a HIP device")
    w, h = a.width, a.height
    g = torch.Generator(device="cuda:0").manual_seed(1)
    ys = [torch.randint(16, 236, (h, w), dtype=torch.uint8, device="cuda:0", generator=g) for _ in range(2)]
    cs = [torch.randint(16, 241, (h // 2, w // 2, 2), dtype=torch.uint8, device="cuda:0", generator=g) for _ in range(2)]
    fl = [torch.rand((h, w, 3), dtype=torch.float32, device="cuda:0", generator=g) for _ in range(2)]
    torch.cuda.synchronize()
    fct = ea.facet_spec(ea.SPHERICAL, w, h, 360.0)
    m = ea.ycbcr_matrix("709")
    st = torch.cuda.Stream()

    def run(frame):
        times = []
        for _ in range(a.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.frames):
                frame(k & 1)
            ea.sync()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / a.frames)
        return statistics.median(times[1:])          # the first round warms up

    res = {"width": w, "height": h, "frames": a.frames, "rounds": a.rounds,
           "ycbcr_decode_bytes": w * h + 2 * (w // 2) * (h // 2) + 12 * w * h}
    keep = {}

    def load_ycbcr(k):
        keep["s"] = ea.Source.load_ycbcr(fct, ys[k], cs[k], m, spline_degree=3)

    def load_floats(k):
        keep["s"] = ea.Source.load(fct, fl[k], 3)

    res["load_ycbcr_ms"] = run(load_ycbcr)
    res["load_floats_ms"] = run(load_floats)
    src = keep.pop("s")
    res["reload_ycbcr_ms"] = run(lambda k: src.reload_ycbcr(ys[k], cs[k], m, stream=st))
    res["reload_floats_ms"] = run(lambda k: src.reload(fl[k], stream=st))
    # the last frame stands in the container: the same as a fresh load of it
    want = ea.Source.load(fct, fl[(a.frames - 1) & 1], 3)
    res["same_container"] = bool((src.download().view(np.uint32) == want.download().view(np.uint32)).all())
    ea.reload_scratch_release()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
