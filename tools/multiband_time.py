"""Multi-band blending against feathering on one multi-facet job: bench.py's six-fisheye workload (WORKLOADS["config5"]:
six 8192 x 8192 circular-fisheye facets, hfov 130, looking front / right / back / left / up / down, PTO lens a / b / c,
onto a 16384 x 8192 spherical target, bilinear) composed as `feather` and as `multiband` at --bands 1, 4 and 8, with
4-channel and with 3-channel facets.
What is measured is KERNEL time: eu_hip_render_timed's HIP events on the library's stream around --iters jobs into
device memory, after one untimed job; the sources are loaded once and shared. The jobs alternate, --reps times, after a
warm-up of every one of them; min, median and max over the repetitions are reported. Then, per number of bands, the
library's stage diagnostic (events around every launch, so the stages do not overlap and their sum is a little above
the job's time): kernel milliseconds of stage A, normalise, reduce, band and collapse, and for the three streaming
stages the NOMINAL bytes - every plane a kernel reads or writes counted once, whatever the caches do, the band kernel's
as if every pixel were covered - over the time, next to the prefilter's streaming figure (4.0 to 4.3 TB/s).
Nothing is promised about the numbers: they are what DESIGN.md 5 quotes. The scratch bytes of each job are reported.
Needs a HIP device. Prints one JSON line per job; --out FILE keeps them (a JSON list).
    python tools/multiband_time.py [--out profiles/multiband_times.json] [--reps 5] [--iters 5] [--facet 8192] [--channels 4,3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import envutil_amd as ea  # noqa: E402
from bench import WORKLOADS, synth_on_device  # noqa: E402  (the workload is bench.py's; nothing of it is edited)

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--facet", type=int, default=0, help="facet size in pixels, square (default: the workload's)")
ap.add_argument("--channels", default="4,3")
ap.add_argument("--bands", default="1,4,8")
opt = ap.parse_args()
if opt.reps < 3:
    sys.exit("at least three repetitions")
if ea.device_count() < 1:
    sys.exit("multiband_time.py needs a HIP device: there is nothing to time without one")
import torch  # noqa: E402

(sname, sw, sh, shfov), (tname, tw, th, thfov), _, degree, twine, ypr = WORKLOADS["config5"]
if opt.facet:
    tw, th = max(64, tw * opt.facet // sw), max(32, th * opt.facet // sh)
    sw = sh = opt.facet
sprj, tprj = ea.api.PROJECTION_NAMES.index(sname), ea.api.PROJECTION_NAMES.index(tname)
VIEWS = [(0, 0, 0), (90, 0, 0), (180, 0, 0), (270, 0, 0), (0, 90, 0), (0, -90, 0)]
BANDS = [int(b) for b in opt.bands.split(",")]
STAGES = ("stage_a", "normalise", "reduce", "band", "collapse")
PREFILTER_TBS = (4.0, 4.3)
L = ea.lib()
L.eu_hip_multiband_stage_times.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
dev = torch.device("cuda", 0)


def stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def run(nch):
    sources = []
    for v in VIEWS:
        img = synth_on_device(torch, dev, sw, sh, nch)
        if nch == 4:
            img[:, :, 3] = 1.0
        host = img.cpu().numpy()
        del img
        torch.cuda.empty_cache()
        sources.append(ea.Source.load(ea.facet_spec(sprj, sw, sh, shfov, nchannels=nch, yaw=v[0], pitch=v[1], roll=v[2],
                                                    lens=dict(a=0.01, b=-0.03, c=0.02)), host, degree))
        del host
        print(f"facet {len(sources)} of {len(VIEWS)} loaded ({nch} channels)", file=sys.stderr, flush=True)
    out = torch.empty((th, tw, nch), device=dev, dtype=torch.float32)
    common = dict(yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree, twine=0)
    jobs = {"feather": ea.arguments(tprj, tw, th, thfov, synopsis="feather", **common)}
    for b in BANDS:
        jobs[f"multiband{b}"] = ea.arguments(tprj, tw, th, thfov, synopsis="multiband", bands=b, **common)
    names = list(jobs)

    def once(s, iters):
        return ea.render_timed(jobs[s], sources, out.data_ptr(), iters, nch)

    share = {}
    for s in names:
        once(s, 2)
        ea.sync()
        frame = out[::16, ::16].cpu().numpy()
        share[s] = round(float((frame != 0).any(axis=2).mean()), 4)
        if share[s] < 0.5:
            sys.exit(f"{s}: the frame is mostly empty - no timing is kept")
    ms = {s: [] for s in names}
    for _ in range(opt.reps):
        for s in names:                          # the jobs alternate: a drift of the clocks hits all of them alike
            ms[s].append(once(s, opt.iters))
    st = {s: stats(ms[s]) for s in names}
    stages = {}
    handles = (C.c_void_p * len(sources))(*[s.handle for s in sources])
    for b in BANDS:
        a = jobs[f"multiband{b}"]
        t = a.target(nch)
        t_ms, t_bytes = (C.c_double * 5)(), (C.c_double * 5)()
        rc = L.eu_hip_multiband_stage_times(C.byref(t), handles, len(sources), C.c_void_p(out.data_ptr()), tw * nch * 4, opt.iters,
                                            t_ms, t_bytes)
        if rc:
            sys.exit(f"stage times: {L.eu_hip_last_error().decode()}")
        stages[f"multiband{b}"] = {
            "levels": ea.multiband_levels(tw, th, b, True),
            "scratch_bytes": ea.multiband_scratch_bytes(a, len(sources), nch),
            "stage_ms": {k: round(t_ms[i], 4) for i, k in enumerate(STAGES)},
            "stage_sum_ms": round(sum(t_ms), 4),
            "nominal_gbytes": {k: round(t_bytes[i] / 1e9, 3) for i, k in enumerate(STAGES)},
            "nominal_tbytes_per_s": {k: round(t_bytes[i] / 1e9 / t_ms[i], 3) if t_ms[i] > 0 else None
                                     for i, k in enumerate(STAGES) if k in ("reduce", "band", "collapse")}}
    res = {"job": f"six {sname} facets {sw}x{sh}, {nch} channels, lens polynomial -> {tname} {tw}x{th}, degree {degree}, no twining",
           "what": "kernel time per job, ms: HIP events around --iters jobs, min / median / max over the repetitions; stages: "
                   "events around every launch, nominal bytes over time",
           "repetitions": opt.reps, "iters": opt.iters, "covered_share": share, "kernel_ms": st,
           "over_feather": {s: round(st[s]["median"] / st["feather"]["median"], 3) for s in names if s != "feather"},
           "prefilter_streaming_tbytes_per_s": PREFILTER_TBS, "stages": stages,
           "all_ms": {s: [round(v, 4) for v in ms[s]] for s in names}}
    for s in sources:
        s.release()
    del out
    ea.multiband_scratch_release()
    torch.cuda.empty_cache()
    return res


results = []
for nch in (int(c) for c in opt.channels.split(",")):
    results.append(run(nch))
    print(json.dumps(results[-1]), flush=True)
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
