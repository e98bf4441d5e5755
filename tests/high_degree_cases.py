"""The sources, targets and jobs that hold spline degrees 4 to 9 to the CPU oracle: shared by tests/test_gpu_high_degree.py
(the device, bit for bit) and tests/test_high_degree_host.py (no GPU: every tap of every such job lies inside its
container, before anything goes to a device). TEST CODE, a helper and not a test.

Degrees above 3 have no templated kernel: they take the run-time-degree evaluator (eu_bspline_generic in
eu_render_dev.h, its copy in eu_render_layers.hip), the `default:` arm of every launcher's switch over the degree, and
from degree 6 on a prefilter of three and four poles."""
import numpy as np

import envutil_amd as ea
import euo
import jobs

DEGREES = (4, 6, 7, 8, 9)
CHANNELS = (1, 3, 4)
LENS = dict(a=0.01, b=-0.03, c=0.02, h=0.01, v=-0.02)

# name -> (projection, width, height, hfov, keywords of jobs.OracleSource / ea.facet_spec)
SOURCES = {
    "latlon": (euo.SPHERICAL, 128, 64, 360.0, {}),
    "cubemap": (euo.CUBEMAP, 32, 192, 90.0, {}),
    "biatan6": (euo.BIATAN6, 24, 144, 90.0, {}),
    "fisheye": (euo.FISHEYE, 96, 96, 190.0, dict(lens=LENS)),
    "rectilinear": (euo.RECTILINEAR, 97, 65, 80.0, {}),          # has misses
}
# 65 x 33: one live lane in the second 64-pixel tile; 72 x 36 crosses the seam and both poles; 16 x 96: rows by face
TARGETS = [(ea.RECTILINEAR, 65, 33, 90.0), (ea.SPHERICAL, 72, 36, 360.0), (ea.CUBEMAP, 16, 96, 90.0)]
YPRS = [(0.0, 0.0, 0.0), (30.0, 15.0, 7.5)]
VIEWS = [(0.0, 0.0, 0.0), (30.0, 15.0, 7.5), (-40.0, 20.0, -5.0, 67.5)]


def cube(prj):
    return prj in (euo.CUBEMAP, euo.BIATAN6)


def image(name, nch, seed=31):
    prj, w, h, hfov, kw = SOURCES[name]
    return jobs.synth_cubefaces(w, nch, seed=seed) if cube(prj) else jobs.synth_image(w, h, nch, seed=seed)


_oracle = {}


def oracle_source(name, nch, degree, seed=31, **more):
    """the CPU oracle's source: made once per key, shared, never written to"""
    key = (name, nch, degree, seed, tuple(sorted(more.items())))
    if key not in _oracle:
        prj, w, h, hfov, kw = SOURCES[name]
        _oracle[key] = jobs.OracleSource(prj, w, h, hfov, image(name, nch, seed), degree, **kw, **more)
    return _oracle[key]


def facet(name, nch):
    prj, w, h, hfov, kw = SOURCES[name]
    return ea.facet_spec(prj, w, h, hfov, nchannels=nch, **kw)


def args_of(target, ypr, degree, **kw):
    return ea.arguments(*target, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree, **kw)


def single_facet_jobs():
    """(source name, target, ypr): every source onto every target, upright and rotated"""
    return [(name, t, ypr) for name in SOURCES for t in TARGETS for ypr in YPRS]


# ---------------------------------------------------------------------------
# the window a degree-d evaluation reads, from a job's stage-2 coordinates. The evaluator gates the coordinate into
# [lower, upper] by the axis' boundary condition, takes floor (odd degrees) or round-half-away (even degrees) of it
# and reads texels  that - d // 2 ... that - d // 2 + d  of the core, both ends included
# ---------------------------------------------------------------------------

F = np.float32


def gate(c, bc, n):
    """the coordinate an axis of n core texels is evaluated at (float32, as eval.h's gates): REFLECT mirrors on
    -0.5 and n - 0.5, PERIODIC wraps into [-0.5, n - 0.5)"""
    c = np.asarray(c, np.float32)
    assert bc in (euo.REFLECT, euo.PERIODIC)
    if n == 1:
        return np.zeros_like(c)
    lower, w = F(-0.5), F(n)
    cc = (c - lower).astype(np.float32)
    if bc == euo.PERIODIC:
        out = (cc < 0) | (cc >= w)
        cm = np.fmod(cc, w).astype(np.float32)
        cm = np.where(cc < 0, cm + w, cm).astype(np.float32)
        cm = np.where(cm >= w, F(0), cm)
        cc = np.where(out, cm, cc)
    else:
        cc = np.abs(cc)
        cm = (w - np.abs(np.fmod(cc, F(2) * w).astype(np.float32) - w)).astype(np.float32)
        cc = np.where(cc >= w, cm, cc)
    return (cc + lower).astype(np.float32)


def window(g, degree):
    """(first, last) core texel read along one axis for gated coordinates g"""
    g = np.asarray(g, np.float32)
    base = np.floor(g) if degree & 1 else np.trunc(g + np.copysign(F(0.5), g).astype(np.float32))
    first = base.astype(np.int64) - degree // 2
    return first, first + degree


def check_taps_inside(name, degree, target, ypr, nch=1, support_min=8):
    """every tap of the job's hits lies inside the container; a cube source with the frame of `support_min`.
    Returns the number of hits"""
    prj, w, h, hfov, kw = SOURCES[name]
    more = dict(support_min=support_min) if cube(prj) else {}
    o = oracle_source(name, nch, degree, **more)
    crd = jobs.oracle_render(args_of(target, ypr, degree), o, stage=2)
    return check_windows(o, prj, w, h, crd, degree, f"{name} degree {degree} -> {target} {ypr}", support_min)


# ---------------------------------------------------------------------------
# the single-facet jobs of tests/test_gpu_high_degree.py beyond single_facet_jobs(): what the GPU module sends, the
# host module replays. A twined job evaluates the source at every tap's ray, not at the pixel's centre
# ---------------------------------------------------------------------------

TWINE_JOBS = [(TARGETS[0], YPRS[1]), (TARGETS[1], YPRS[1]), (TARGETS[2], YPRS[0])]      # test_twining: twine 2 and 3
TWINE_DEGREES = (4, 9)
FEWER_CHANNELS = (("latlon", 4, 3), ("fisheye", 3, 1), ("cubemap", 4, 1))              # on TARGETS[1], YPRS[1]
VIEW_SOURCES, LAYER_SOURCES, RAY_SOURCES = ("latlon", "cubemap"), ("latlon", "fisheye"), ("latlon", "cubemap", "fisheye")
BATCH_TARGETS = TARGETS[:2]           # views, layers (plain and twine 2) and rays (plain, and ninepacks with twine 3)
TRANSLATED_TARGET = (ea.RECTILINEAR, 150, 77, 60.0)
TRANSLATED_JOBS = (((5.0, -2.0, 0.0), 0), ((12.0, 4.0, 8.0), 0), ((12.0, 4.0, 8.0), 2))   # (ypr, twine)
TRANSLATED_DEGREES = (3, 6, 9)
RELOAD_SOURCE, RELOAD_DEGREE = (euo.SPHERICAL, 64, 32, 360.0), 8
RELOAD_JOB = (TARGETS[0], YPRS[1])


def view_args(target, view, degree, **kw):
    """the job that is view (yaw, pitch, roll[, hfov]) of a render_views call on `target`"""
    hfov = view[3] if len(view) == 4 else target[3]
    return ea.arguments(target[0], target[1], target[2], hfov, yaw=view[0], pitch=view[1], roll=view[2],
                        spline_degree=degree, **kw)


def translated_source(degree):
    """definitions64.translated_facet() with its picture: (oracle source, facet_spec)"""
    import definitions64 as d64
    f = d64.translated_facet()
    kw = dict(yaw=f.yaw, pitch=f.pitch, roll=f.roll, translation=f.translation)
    o = jobs.OracleSource(f.prj, f.w, f.h, f.hfov, d64.facet_image(f, 3), degree, **kw)
    return o, ea.facet_spec(f.prj, f.w, f.h, f.hfov, nchannels=3, **kw)


def single_target_args(degree):
    """a --single target: it recreates a fisheye facet, through the generic stepper; rendered from the lat/lon source"""
    kw = dict(yaw=10.0, pitch=-5.0, roll=3.0)
    a = ea.arguments.for_single(ea.facet_spec(euo.FISHEYE, 60, 44, 120.0, nchannels=3, **kw), spline_degree=degree)
    a.single_oracle = jobs.OracleSource(euo.FISHEYE, 60, 44, 120.0, jobs.synth_image(60, 44, 3, seed=5), degree, **kw)
    return a


def reload_pictures():
    prj, w, h, hfov = RELOAD_SOURCE
    return jobs.synth_image(w, h, 3, seed=1), jobs.synth_image(w, h, 3, seed=2)


# ---- the fuzz: its own draw function and seeds ----------------------------------------------------------------------

FUZZ_SOURCES = [euo.SPHERICAL, euo.CYLINDRICAL, euo.RECTILINEAR, euo.STEREOGRAPHIC, euo.FISHEYE, euo.CUBEMAP, euo.BIATAN6]
FUZZ_TARGETS = [ea.SPHERICAL, ea.CYLINDRICAL, ea.RECTILINEAR, ea.STEREOGRAPHIC, ea.FISHEYE, ea.CUBEMAP, ea.BIATAN6]
FUZZ_SEEDS = range(8)
FUZZ_JOBS_PER_SEED = 5


def draw_source(rng, nch, degree, seed, multi):
    """one facet at random: (oracle source, facet_spec, (projection, width, height), description). A single facet may
    be a cube or a full sphere; the facets of a multi-facet job are partial views with an orientation of their own"""
    prj = FUZZ_SOURCES[rng.integers(5 if multi else len(FUZZ_SOURCES))]
    kw = {}
    if cube(prj):
        w = int(rng.integers(12, 40))
        h, hfov = 6 * w, 90.0
        img = jobs.synth_cubefaces(w, nch, seed=seed)
    else:
        w, h = int(rng.integers(24, 120)), int(rng.integers(24, 100))
        hfov = float(rng.uniform(40.0, {euo.RECTILINEAR: 120.0, euo.STEREOGRAPHIC: 220.0, euo.FISHEYE: 250.0}.get(prj, 300.0)))
        if not multi and prj in (euo.SPHERICAL, euo.CYLINDRICAL) and rng.random() < 0.5:
            hfov = 360.0
            if prj == euo.SPHERICAL:
                h = w // 2
                w = 2 * h
        img = jobs.synth_image(w, h, nch, seed=seed)
        kw = dict(yaw=float(rng.uniform(-60, 60)), pitch=float(rng.uniform(-40, 40)), roll=float(rng.uniform(-20, 20)),
                  brighten=float(rng.choice([1.0, 0.5, 1.3])))
        if prj not in (euo.SPHERICAL, euo.CYLINDRICAL) and rng.random() < 0.4:
            kw["lens"] = dict(a=float(rng.uniform(-0.015, 0.015)), b=float(rng.uniform(-0.03, 0.03)), c=float(rng.uniform(-0.02, 0.02)))
    o = jobs.OracleSource(prj, w, h, hfov, img, degree, **kw)
    return o, ea.facet_spec(prj, w, h, hfov, nchannels=nch, **kw), (prj, w, h), f"{prj} {w}x{h} fov {hfov:.1f} {kw}"


def fuzz_jobs(seed):
    """the jobs of one seed, degrees drawn from 4 to 9: dicts of degree, nch, out_n, facets (draw_source's tuples),
    args and a description. Single-facet and multi-facet jobs, twining, crops, channel adaption"""
    rng = np.random.default_rng(94000 + seed)
    out = []
    for k in range(FUZZ_JOBS_PER_SEED):
        degree = int(rng.integers(4, 10))
        nch = int(rng.integers(1, 5))
        nf = int(rng.choice([1, 1, 1, 2, 3, 5]))
        facets = [draw_source(rng, nch, degree, seed * 1000 + 10 * k + i, nf > 1) for i in range(nf)]
        kw = dict(spline_degree=degree, twine=int(rng.choice([0, 0, 2, 3])))
        if nf > 1:
            kw["synopsis"] = str(rng.choice(["panorama", "hdr_merge"]))
        tprj = FUZZ_TARGETS[rng.integers(len(FUZZ_TARGETS))]
        if tprj in (ea.CUBEMAP, ea.BIATAN6):
            tw = int(rng.integers(8, 24))
            th, thf = 6 * tw, 90.0
        else:
            tw, th = int(rng.integers(8, 100)), int(rng.integers(8, 50))
            thf = float(rng.uniform(30.0, {ea.RECTILINEAR: 130.0, ea.STEREOGRAPHIC: 280.0}.get(tprj, 360.0)))
        if rng.random() < 0.25:
            x0, y0 = int(rng.integers(0, tw // 2)), int(rng.integers(0, th // 2))
            kw["crop"] = (x0, int(rng.integers(x0 + 1, tw + 1)), y0, int(rng.integers(y0 + 1, th + 1)))
        out_n = nch if rng.random() < 0.8 else int(rng.integers(1, 5))
        a = ea.arguments(tprj, tw, th, thf, yaw=float(rng.uniform(-180, 180)), pitch=float(rng.uniform(-60, 60)),
                         roll=float(rng.uniform(-30, 30)), **kw)
        what = (f"seed {seed} job {k}: degree {degree} nch {nch} -> {out_n}, facets {[f[3] for f in facets]}, "
                f"target {tprj} {tw}x{th} fov {thf:.1f} {kw}")
        out.append(dict(degree=degree, nch=nch, out_n=out_n, facets=facets, args=a, what=what))
    return out


# ---- coordinates and windows of any single-facet job ----------------------------------------------------------------

def job_coordinates(a, o):
    """(n, 3) source coordinates {x, y, face | 0 | -1 for a miss} of every evaluation a single-facet job makes: the
    oracle's stage 2 of an untwined job; for a twined job the coordinates of every tap's ray, the rays put together
    from the three steppers' rays (stages 1, 3 and 4) as the kernels and the oracle do (feather_model.tap_rays)"""
    if a.twine_spread is None:
        return jobs.oracle_render(a, o, stage=2).reshape(-1, 3)
    import feather_model as fm
    r00, r10, r01 = (jobs.oracle_render(a, o, stage=s) for s in (1, 3, 4))
    return np.concatenate([euo.source_coordinates(o.s, fm.tap_rays(r00, r10, r01, tap).reshape(-1, 3))
                           for tap in np.asarray(a.twine_spread, np.float32)])


def check_windows(o, prj, w, h, crd, degree, what, support_min=8):
    """every degree-d window of the hits among `crd` lies inside the container of source `o` (a cube source: inside
    the face's own section of the intermediate image, frame included). Returns the number of hits"""
    crd = np.asarray(crd, np.float32).reshape(-1, 3)
    hit = (crd[:, 2] >= 0) & np.isfinite(crd).all(1)
    x, y = crd[hit, 0], crd[hit, 1]
    if not hit.any():
        return 0
    if cube(prj):
        m = ea.cubemap_metrics(w, np.pi / 2, support_min)
        sec = m["section_px"]
        assert m["left_frame_px"] >= support_min, what
        assert o.container.shape[:2] == (6 * sec, sec), what
        face = crd[hit, 2].astype(np.int64)
        x0, x1 = window(x, degree)
        y0, y1 = window(y, degree)
        assert x0.min() >= 0 and x1.max() <= sec - 1, f"{what}: columns {x0.min()} .. {x1.max()} of {sec}"
        assert (y0 >= face * sec).all() and (y1 <= (face + 1) * sec - 1).all(), f"{what}: a window leaves its face's section"
        return int(hit.sum())
    g = ea.container_geometry(degree, o.bc[0], o.bc[1], w, h)
    assert o.container.shape[:2] == (g.shape[1], g.shape[0]), what
    for axis, (c, n) in enumerate(((x, w), (y, h))):
        first, last = window(gate(c, o.bc[axis], n), degree)
        assert first.min() >= -g.left[axis], f"{what}: axis {axis} reads {first.min()} with a frame of {g.left[axis]}"
        assert last.max() <= n - 1 + g.right[axis], f"{what}: axis {axis} reads {last.max()} of {n} + {g.right[axis]}"
    return int(hit.sum())


def check_job(name, degree, a, what, nch=1):
    """check_windows of job `a` on the source SOURCES[name]"""
    prj, w, h, hfov, kw = SOURCES[name]
    o = oracle_source(name, nch, degree)
    return check_windows(o, prj, w, h, job_coordinates(a, o), degree, f"{name} degree {degree}: {what}")
