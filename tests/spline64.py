"""A float64 B-spline of any degree, written from the definition alone. TEST CODE, a helper and not a test; numpy
only. Nothing here is taken from oracle/eu_oracle.c, from eu_setup_math.h, from eu_render_dev.h or from the
reference's program text: there are no poles, no recursive filter, no weight matrix and no split of a coordinate
into a whole number and a fraction, so no reading of that text which the oracle and the library share - a rounding
rule, a truncated start value, a window origin - can be shared by this file.

The basis is the centred cardinal B-spline B_d, by the Cox-de Boor recursion. The coefficients of a line of samples
s are the solution of the dense collocation system  sum_j B_d(j) c_ext[i - j] = s[i]  (numpy.linalg.solve), where
c_ext is the line continued by its boundary condition; an image is solved axis by axis. The value at (x, y) is
sum_k sum_l B_d(x - k) B_d(y - l) c_ext[l, k]  over every k, l for which the weight can differ from zero.

The boundary numbers are the oracle binding's public constants (tests/euo.py: MIRROR ... NATURAL).
"""
import functools

import numpy as np

MIRROR, PERIODIC, REFLECT, NATURAL = range(4)
MAX_DEGREE = 9


# ---------------------------------------------------------------------------
# the basis
# ---------------------------------------------------------------------------

def basis(d, t):
    """B_d(t), the centred cardinal B-spline of degree d: B_0 is 1 on [-1/2, 1/2), and
    B_d(t) = ((t + (d + 1) / 2) B_{d-1}(t + 1/2) + ((d + 1) / 2 - t) B_{d-1}(t - 1/2)) / d"""
    t = np.asarray(t, np.float64)
    # the recursion bottom up: level m holds B_m at t + (d - m) / 2 - i, i = 0 .. d - m, so that the two values a
    # B_m needs, B_{m-1} half a step to either side, are entries i and i + 1 of the level below
    at = [t + (d / 2.0 - i) for i in range(d + 1)]
    level = [((u >= -0.5) & (u < 0.5)).astype(np.float64) for u in at]
    for m in range(1, d + 1):
        h = (m + 1) / 2.0
        at = [t + ((d - m) / 2.0 - i) for i in range(d - m + 1)]
        level = [((u + h) * level[i] + (h - u) * level[i + 1]) / m for i, u in enumerate(at)]
    return level[0]


# ---------------------------------------------------------------------------
# boundary conditions: c_ext[m] as a row vector over the n coefficients of the line
# ---------------------------------------------------------------------------

def continuation(bc, n, m):
    """the row e with c_ext[m] = e . c, for any whole m"""
    e = np.zeros(n)
    if 0 <= m < n:
        e[m] = 1.0
    elif n == 1:
        e[0] = 1.0
    elif bc == PERIODIC:
        e[m % n] = 1.0
    elif bc == REFLECT:                     # c[-1 - k] = c[k]: period 2n
        m %= 2 * n
        e[m if m < n else 2 * n - 1 - m] = 1.0
    elif bc == MIRROR:                      # c[-k] = c[k]: period 2n - 2
        m %= 2 * n - 2
        e[m if m < n else 2 * n - 2 - m] = 1.0
    elif bc == NATURAL:                     # c[-k] = 2 c[0] - c[k], and the same about the last sample
        if m < 0:
            e = -continuation(bc, n, -m)
            e[0] += 2.0
        else:
            e = -continuation(bc, n, 2 * (n - 1) - m)
            e[n - 1] += 2.0
    else:
        raise ValueError(bc)
    return e


@functools.lru_cache(maxsize=None)
def collocation(d, n, bc):
    """the n x n matrix A with A c = s"""
    a = np.zeros((n, n))
    for j in range(-(d // 2), d // 2 + 1):
        b = float(basis(d, float(j)))
        for i in range(n):
            a[i] += b * continuation(bc, n, i - j)
    return a


def solve_axis(s, d, bc, axis):
    """coefficients along one axis of an array, every line the same system"""
    if d < 2:
        return s
    s = np.moveaxis(s, axis, 0)
    n = s.shape[0]
    c = np.linalg.solve(collocation(d, n, bc), s.reshape(n, -1)).reshape(s.shape)
    return np.moveaxis(c, 0, axis)


def extend_axis(c, bc, margin, axis):
    """c_ext for m in [-margin, n + margin) along one axis"""
    c = np.moveaxis(c, axis, 0)
    n = c.shape[0]
    ext = np.stack([continuation(bc, n, m) for m in range(-margin, n + margin)])
    out = (ext @ c.reshape(n, -1)).reshape((n + 2 * margin,) + c.shape[1:])
    return np.moveaxis(out, 0, axis)


# ---------------------------------------------------------------------------
# the full sphere: column x read top to bottom, followed by column x + W/2 read bottom to top, is one periodic
# line of 2H samples (a meridian circle through both poles). Rows are periodic.
# ---------------------------------------------------------------------------

def solve_sphere_columns(s, d):
    if d < 2:
        return s
    h, w = s.shape[:2]
    assert w % 2 == 0
    half = w // 2
    line = np.concatenate([s[:, :half], s[::-1, half:]], 0)              # (2h, w / 2, ...)
    c = solve_axis(line, d, PERIODIC, 0)
    return np.concatenate([c[:h], c[:h - 1:-1]], 1) if h > 0 else s       # rows h .. 2h-1 reversed: column x + w/2


def extend_sphere_columns(c, margin):
    """the continuation across a pole: row -1 - j is row j of column x + W/2"""
    h, w = c.shape[:2]
    assert margin <= h
    other = np.roll(c, w // 2, axis=1)
    return np.concatenate([other[:margin][::-1], c, other[h - margin:][::-1]], 0)


# ---------------------------------------------------------------------------
# the spline
# ---------------------------------------------------------------------------

FAULTS = ("tap_scaled", "even_window_shifted", "last_pole_dropped", "weights_exchanged")


def applies(fault, degree):
    """the degrees at which a fault changes anything"""
    return {"tap_scaled": True, "even_window_shifted": degree % 2 == 0, "last_pole_dropped": degree >= 4,
            "weights_exchanged": True}[fault]


class Spline64:
    """samples (h, w, nch) -> a function of (x, y), pixel centres at whole numbers. bc0 belongs to x, bc1 to y;
    sphere=True: periodic rows, columns stacked through the poles. `fault`: one of FAULTS, a deliberately wrong
    model that shows a check can fail"""

    def __init__(self, samples, degree, bc0, bc1, sphere=False, prefilter_degree=None, fault=None):
        assert 0 <= degree <= MAX_DEGREE and fault in (None,) + FAULTS
        s = np.asarray(samples, np.float64)
        if s.ndim == 2:
            s = s[..., None]
        pdeg = degree if prefilter_degree is None else prefilter_degree
        if fault == "last_pole_dropped" and pdeg >= 4:
            pdeg -= 2
        self.degree, self.fault = degree, fault
        self.h, self.w, self.nch = s.shape
        self.margin = degree // 2 + 3               # the taps of a point up to a texel outside the samples
        if sphere:
            bc0 = PERIODIC
            c = solve_sphere_columns(solve_axis(s, pdeg, PERIODIC, 1), pdeg)
            ext = extend_sphere_columns(c, self.margin)
        else:
            c = solve_axis(solve_axis(s, pdeg, bc0, 1), pdeg, bc1, 0)
            ext = extend_axis(c, bc1, self.margin, 0)
        self.coefficients = c
        self.extended = extend_axis(ext, bc0, self.margin, 1)

    def __call__(self, x, y, fault=None):
        """(n,) x, (n,) y -> (n, nch), float64. `fault`: one of the FAULTS of the evaluation, over the same coefficients"""
        x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
        d, m, fault = self.degree, self.margin, fault or self.fault
        if fault == "weights_exchanged":
            fx, fy = x - np.floor(x), y - np.floor(y)
            x, y = np.floor(x) + fy, np.floor(y) + fx
        half = (d + 1) / 2.0
        # every whole k with |x - k| <= (d + 1) / 2: d + 2 of them at the most
        k0 = np.ceil(x - half).astype(np.int64)
        l0 = np.ceil(y - half).astype(np.int64)
        t = np.arange(d + 2)
        ks, ls = k0[:, None] + t, l0[:, None] + t
        wx, wy = basis(d, x[:, None] - ks), basis(d, y[:, None] - ls)
        if fault == "tap_scaled":
            big = wx.argmax(1)
            wx[np.arange(len(x)), big] *= 1.0 + 2.0 ** -10
        if fault == "even_window_shifted" and d % 2 == 0:
            ks, ls = ks + 1, ls + 1
        assert ks.min() >= -m and ks.max() < self.w + m and ls.min() >= -m and ls.max() < self.h + m, "outside the samples"
        taps = self.extended[(ls + m)[:, :, None], (ks + m)[:, None, :]]          # (n, d + 2, d + 2, nch)
        return np.einsum("nl,nk,nlkc->nc", wy, wx, taps)


# ---------------------------------------------------------------------------
# what the CPU oracle measures against this model: the largest absolute difference per (source kind, degree),
# "plain" (a core under a pair of boundary conditions; a source that is not a full sphere) and "latlon" (the full
# sphere, whose prefilter stops at 0.0001 by design). Over plain_cases(), latlon_case() and gpu_cases(), which
# tests/test_spline64_oracle.py and tests/test_gpu_spline64.py share. Printed by print_envelopes64():
#     python -c "import sys; sys.path.insert(0, 'tests'); import spline64; spline64.print_envelopes64()"
# measured with the oracle, never with the library. The tests allow BIN_MARGIN times a row.
# ---------------------------------------------------------------------------

ENVELOPES64 = {
    ('plain', 0): 0.00e+00,
    ('latlon', 0): 0.00e+00,
    ('plain', 1): 1.50e-06,
    ('latlon', 1): 1.02e-07,
    ('plain', 2): 1.26e-06,
    ('latlon', 2): 1.61e-05,
    ('plain', 3): 1.36e-06,
    ('latlon', 3): 5.72e-05,
    ('plain', 4): 1.86e-06,
    ('latlon', 4): 2.10e-05,
    ('plain', 5): 1.18e-06,
    ('latlon', 5): 6.77e-05,
    ('plain', 6): 1.71e-06,
    ('latlon', 6): 3.52e-05,
    ('plain', 7): 2.36e-06,
    ('latlon', 7): 3.14e-05,
    ('plain', 8): 6.17e-06,
    ('latlon', 8): 3.99e-05,
    ('plain', 9): 1.40e-05,
    ('latlon', 9): 7.13e-05,
}

BIN_MARGIN = 2.0         # definitions64.BIN_MARGIN: the project's margin over a measured envelope

DEGREES = tuple(range(MAX_DEGREE + 1))
BOUNDARY_PAIRS = ((PERIODIC, REFLECT), (REFLECT, REFLECT), (MIRROR, MIRROR), (NATURAL, NATURAL))
CORES = ((40, 24, 3), (9, 7, 1))            # the second is shorter than the degree-9 horizon on both axes
CONTENTS = ("noise", "synth")


def tolerance(kind, degree):
    return BIN_MARGIN * ENVELOPES64[(kind, degree)]


def core_image(w, h, nch, content):
    if content == "noise":
        return np.random.default_rng(1000 * w + h).random((h, w, nch), dtype=np.float32)
    import jobs
    return jobs.synth_image(w, h, nch, seed=77)


def core_coordinates(w, h, degree, seed):
    """300 points inside the core, 50 of them within d / 2 + 1 of a border"""
    rng = np.random.default_rng(seed)
    crd = np.stack([rng.uniform(0.0, w - 1.0, 300), rng.uniform(0.0, h - 1.0, 300)], 1)
    near = degree / 2.0 + 1.0
    for i in range(50):
        axis, far_side = i % 2, (i // 2) % 2
        n = (w, h)[axis] - 1.0
        dist = rng.uniform(0.0, min(near, n))
        crd[i, axis] = n - dist if far_side else dist
    return crd.astype(np.float32)


def plain_cases():
    """(w, h, nch, content, bc0, bc1)"""
    return [(w, h, n, content, b0, b1) for w, h, n in CORES for content in CONTENTS for b0, b1 in BOUNDARY_PAIRS]


def solve_fault(fault):
    """the part of a fault that changes the coefficients; the rest changes the evaluation only"""
    return fault if fault == "last_pole_dropped" else None


@functools.lru_cache(maxsize=None)
def _plain_oracle(case, degree):
    import euo
    w, h, n, content, b0, b1 = case
    crd = core_coordinates(w, h, degree, seed=100 * w + degree)
    o = euo.BSpline(core_image(w, h, n, content), degree, b0, b1)
    o.prefilter(degree)
    return crd, o.eval(crd).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _plain_model(case, degree, fault):
    w, h, n, content, b0, b1 = case
    return Spline64(core_image(w, h, n, content), degree, b0, b1, fault=fault)


def oracle_plain(case, degree, fault=None):
    """(the oracle's values, the model's) of one plain case"""
    crd, got = _plain_oracle(case, degree)
    return got, _plain_model(case, degree, solve_fault(fault))(crd[:, 0], crd[:, 1], fault)


# the jobs of tests/test_gpu_spline64.py: sources that Source.load builds on the device. (name, kind, projection,
# w, h, hfov, lens); every source at yaw, pitch, roll 0
LENS = dict(a=0.02, b=0.0, c=-0.01, h=0.01, v=-0.02, g=0.003, t=-0.002)
SOURCES = {
    "latlon": ("latlon", 0, 64, 32, 360.0, None),                # SPHERICAL
    "fisheye": ("plain", 4, 96, 96, 180.0, LENS),                # FISHEYE
    "cylinder": ("plain", 1, 64, 24, 360.0, None),               # CYLINDRICAL
}
# (projection, w, h, hfov, yaw, pitch, roll) of the targets per source: rotated, so that no coordinate falls on
# half a texel by construction; widths that fill no tile. More than half of each frame hits its source
TARGETS = {
    "latlon": [(0, 40, 20, 360.0, 30.0, 15.0, 7.5), (2, 45, 23, 90.0, 170.0, 60.0, 10.0)],
    "fisheye": [(2, 45, 23, 100.0, 4.0, -3.0, 20.0), (0, 40, 20, 360.0, 30.0, 15.0, 7.5)],
    "cylinder": [(2, 45, 23, 70.0, 175.0, 3.0, 5.0), (1, 40, 20, 360.0, 30.0, 8.0, 3.0)],
}


def picture(w, h, nch, seed):
    """a smooth field with mild noise in [0.2, 0.8], float32 (h, w, nch), made here: the GPU module that uses it
    imports nothing of the oracle's. The last of 4 channels is 1, as an alpha channel would be"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    noise = np.random.default_rng(seed).random((h, w, nch))
    out = np.empty((h, w, nch), np.float32)
    for c in range(nch):
        smooth = 0.5 + 0.25 * np.sin(2 * np.pi * (3 + c) * x / w) * np.cos(2 * np.pi * (2 + c) * y / h)
        out[:, :, c] = smooth + 0.05 * noise[:, :, c] - 0.025
    if nch == 4:
        out[:, :, 3] = 1.0
    return out


def source_image(name, nch, negative=False):
    """the picture a source holds; negative: 1 - picture, the second layer of the render_layers jobs"""
    kind, prj, w, h, hfov, lens = SOURCES[name]
    img = picture(w, h, nch, seed=31)
    return np.float32(1.0) - img if negative else img


@functools.lru_cache(maxsize=None)
def source_model(name, nch, degree, fault=None, negative=False):
    """the model of a source; `fault`: solve_fault() of a fault, the others go to its call"""
    kind, prj, w, h, hfov, lens = SOURCES[name]
    img = source_image(name, nch, negative)
    if kind == "latlon":
        return Spline64(img, degree, PERIODIC, REFLECT, sphere=True, fault=fault)
    return Spline64(img, degree, PERIODIC if hfov == 360.0 and prj in (0, 1) else REFLECT, REFLECT, fault=fault)


def make_args(target, degree):
    import envutil_amd as ea
    prj, w, h, hfov, yaw, pitch, roll = target
    return ea.arguments(prj, w, h, hfov, yaw=yaw, pitch=pitch, roll=roll, spline_degree=degree)


def compare(frame, coordinates, model, fault=None):
    """a frame (h, w, nch) against the model at the stage-2 coordinates (h, w, 3) that produced it:
    (largest difference over the hits, share of hits, largest absolute value over the misses). No hit is left out"""
    crd = np.asarray(coordinates, np.float64).reshape(-1, 3)
    got = np.asarray(frame, np.float64).reshape(len(crd), -1)
    hit = crd[:, 2] >= 0
    want = model(crd[hit, 0], crd[hit, 1], fault)
    miss = float(np.abs(got[~hit]).max()) if (~hit).any() else 0.0
    return float(np.abs(got[hit] - want).max()), float(hit.mean()), miss


@functools.lru_cache(maxsize=None)
def _job_oracle(name, target, degree, nch, negative):
    import jobs
    kind, prj, w, h, hfov, lens = SOURCES[name]
    o = jobs.OracleSource(prj, w, h, hfov, source_image(name, nch, negative), degree, lens=lens)
    a = make_args(target, degree)
    return jobs.oracle_render(a, o), jobs.oracle_render(a, o, stage=2)


def oracle_job(name, target, degree, nch=3, fault=None, negative=False):
    """compare() of the CPU oracle's frame of one job"""
    frame, crd = _job_oracle(name, target, degree, nch, negative)
    return compare(frame, crd, source_model(name, nch, degree, solve_fault(fault), negative), fault)


def gpu_cases():
    """(source name, kind, target, degree, nch): degrees 0 to 9 at 3 channels, 1 and 4 channels at degree 9"""
    out = []
    for name, (kind, *_rest) in SOURCES.items():
        for target in TARGETS[name]:
            out += [(name, kind, target, degree, 3) for degree in DEGREES]
            out += [(name, kind, target, MAX_DEGREE, nch) for nch in (1, 4)]
    return out


def layer_cases():
    """the render_layers jobs: the first target of every source, two layers - the picture and its negative"""
    return [c for c in gpu_cases() if c[2] == TARGETS[c[0]][0]]


def measure_envelopes64(fault=None):
    """{(kind, degree): the largest difference between the CPU oracle and the model}"""
    table = {}
    for degree in DEGREES:
        worst = 0.0
        for case in plain_cases():
            got, want = oracle_plain(case, degree, fault)
            worst = max(worst, float(np.abs(got - want).max()))
        table[("plain", degree)] = worst
        table[("latlon", degree)] = 0.0
    for name, kind, target, degree, nch in gpu_cases():
        err, share, miss = oracle_job(name, target, degree, nch, fault)
        table[(kind, degree)] = max(table[(kind, degree)], err)
    for name, kind, target, degree, nch in layer_cases():
        err, share, miss = oracle_job(name, target, degree, nch, fault, negative=True)
        table[(kind, degree)] = max(table[(kind, degree)], err)
    return table


def print_envelopes64():
    """prints the ENVELOPES64 table from the CPU oracle; run on the CPU, pasted in above"""
    for k, v in measure_envelopes64().items():
        print(f"    {k!r}: {v:.2e},")
