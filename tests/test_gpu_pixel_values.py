"""The HIP library against the CPU oracle on the pixel VALUES real images hold (tests/pixel_values.py). The other GPU
tests vary geometry, degree, channel count and kernel family over one kind of data - a smooth 0.2 .. 0.8 field with
alpha 1.0; a kernel that flushed denormals, reordered a sum around a cancellation or mis-read a value gate would pass
them all. Here the geometry is the smallest the other files use to reach each path, and what varies is the data:

  impulse    zeros with a few lit texels: a prefilter's poles decay through the denormal range around each
  hdr        log-uniform 1e-6 .. 6e4
  signed     about +-1e3 with exact +0 and -0
  denormal   denormals of both signs
  big        +-1e37
  nonfinite  an ordinary image with 0.5 % of its texels +inf, -inf, NaN, +-3e38

and an alpha plane of exact zeros of both signs, denormals, the floats around 0.000001f, values above 1 and small
negatives, in aligned groups of 16 that are all zero, partly zero and free of zeros.

Finite classes: float32 bit patterns, 0 ULP (pixel_values.assert_bits). `nonfinite`: equal NaN masks, everything
else equal as uint32 (assert_bits_nan) - which bits a NaN carries is no part of the contract. Every
case also asserts, on the ORACLE's frame, that its data did what it is there for (pixel_values.assert_exercised and
the conditions next to the value gates): conditions on the inputs, never on the library's result.

Cells that are left out, because the REFERENCE has nothing defined to compare with:
  - `nonfinite` under any prefilter of degree 2 or more: one inf turns the whole container NaN. It runs at degrees
    0 and 1, and at degrees 2 and 3 with prefilter_degree=0, so that every kernel body sees non-finite coefficients;
  - `big` under a prefilter of degree 4 or more: zimt multiplies by the filter's whole gain first (385 at degree 4)
    and overflows itself. Sources of a higher spline degree are prefiltered at degree 3; the device set-up cases of
    degree 5 take +-1e34, the largest power of a thousand that degree's gain (120 per axis) leaves finite;
  - NaN through the tethered put stage (to_screen_t): the clamp's comparisons are all false and the table index is
    whatever the conversion of NaN to int gives. The tethered cases use the finite classes.
  - the 5 % denormal condition for `impulse` on the 33-pixel cube faces of the set-up cases: a cubic pole needs 66
    texels to fall to 1e-38, and every IR section is filtered by itself. The case runs, with the condition that the
    container holds denormals at all at degree 2; `impulse` has a cube of 128-pixel faces besides, where the 5 % hold at every degree.
  - the shares of 5 %, 90 % and one half where colours are multiplied by the alpha plane, facets are composed or a
    source misses part of the frame: the frame must then hold denormals at all, a NaN and an inf
    (pixel_values.assert_exercised(some=True))."""
import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
import pixel_values as pv
from test_hdr_merge import numpy_hdr_merge

pytestmark = pytest.mark.gpu

LENS = dict(a=0.01, b=-0.03, c=0.02)
VIEWS6 = [(0, 0, 0), (90, 0, 3), (180, 0, -2), (270, 0, 1), (0, 90, 0), (0, -90, 5)]


def pdeg_of(cls, degree):
    """the prefilter degree a source of this class gets (see the cells left out)"""
    if cls == "nonfinite":
        return 0
    if cls == "big":
        return min(degree, pv.BIG_PREFILTER_MAX)
    return degree


# a lit texel's tail is denormal where the pole's power lies between 1e-38 and 1e-45: 50 - 59 texels away at degree
# 2, 66 - 78 at degree 3, 83 - 98 at degree 4, 104 - 122 at degree 5 (Manhattan distance: the filter is separable). Lit
# texels on a lattice of twice that distance put such a ring around every one of them, wherever a target looks, and
# each tail crosses edges of the prefilter's 64-sample blocks - and their checkpoints - inside the denormal range
LATTICE_STEP = {2: 108, 3: 144, 4: 180, 5: 224}


def lattice(h, w, step):
    ys = list(range(step // 3, h, step)) or [h // 2]
    xs = list(range(step // 2, w, step)) or [w // 2]
    return [(y, x) for y in ys for x in xs]


def image(cls, prj, w, h, nch, seed=1, degree=3):
    """the class as an image of this source: impulses in a corner of every face of a cube (each section is filtered
    by itself), else on the lattice of the degree"""
    if cls == "nonfinite" and w * h < 2000:
        return pv.nonfinite(h, w, nch, seed, one_in=40)        # tiny facets: 0.5 % of 256 texels is one texel
    if cls == "impulse":
        if prj in (euo.CUBEMAP, euo.BIATAN6):
            return pv.impulse(h, w, nch, seed, lit=[(f * w + 2, 2) for f in range(6)])
        return pv.impulse(h, w, nch, seed, lit=lattice(h, w, LATTICE_STEP.get(degree, 144)))
    return pv.make(cls, h, w, nch, seed)


def adopt(o, prj, w, h, hfov, nch, degree, **kw):
    g = ea.Source.adopt(ea.facet_spec(prj, w, h, hfov, nchannels=nch, yaw=kw.get("yaw", 0.0), pitch=kw.get("pitch", 0.0),
                                      roll=kw.get("roll", 0.0), brighten=kw.get("brighten", 1.0), lens=kw.get("lens")),
                        o.container, degree, o.bc[0], o.bc[1])
    g.oracle = o
    return g


_pairs = {}


@pytest.fixture(scope="module", autouse=True)
def release_resident_sources():
    """the cached sources leave the device with the module"""
    yield
    for _, g in _pairs.values():
        g.release()
    _pairs.clear()
    _facets.clear()


def pair(cls, prj, w, h, hfov, nch, degree, alpha=False, seed=1, **kw):
    """(OracleSource, resident Source adopted from the oracle's container), as test_gpu_parity.make_pair; cached.
    alpha: pixel_values.alpha_plane in the last of 2 or 4 channels, the colours multiplied by it"""
    key = (cls, prj, w, h, hfov, nch, degree, alpha, seed, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _pairs:
        img = image(cls, prj, w, h, nch, seed, degree)
        if alpha:
            img = pv.with_alpha(img, seed, associated=True)
        o = jobs.OracleSource(prj, w, h, hfov, img, degree, pdeg_of(cls, degree), **kw)
        _pairs[key] = (o, adopt(o, prj, w, h, hfov, nch, degree, **kw))
    return _pairs[key]


def check(cls, a, g, o, what, nch=None, some=False, **kw):
    """one job on both sides, and the oracle's frame met the class (some: the substitute condition); returns that
    frame"""
    ref = jobs.oracle_render(a, o, nch=nch)
    got = ea.render(a, g, nch, **kw)
    pv.assert_class_bits(cls, got, ref, what)
    pv.assert_exercised(cls, ref, a.spline_degree, what, some=some)
    return ref


# ---- device set-up: the prefilter and the brace ------------------------------------------------------------------

SETUP = {
    "fullsphere": (euo.SPHERICAL, 330, 166, 360.0),         # PERIODIC rows, stacked PERIODIC columns
    "reflect": (euo.RECTILINEAR, 97, 401, 80.0),            # REFLECT x REFLECT, higher than wide
    "cylinder": (euo.CYLINDRICAL, 512, 130, 360.0),         # PERIODIC x REFLECT
    "cube33": (euo.CUBEMAP, 33, 198, 90.0),                 # the IR image of odd faces: NATURAL sections, the fill
    "cube128": (euo.CUBEMAP, 128, 768, 90.0),               # `impulse` only: sections a tail turns denormal in
}


@pytest.mark.parametrize("cls,shape,degree", [(c, s, d) for c in pv.FINITE for s in SETUP for d in (2, 3, 5)
                                              if s != "cube128" or c == "impulse"])
def test_device_setup(cls, shape, degree, monkeypatch):
    """Source.load(...).download() against the oracle's container, 1, 3 and 4 channels, with the streamed prefilter
    as it is by default (checkpoints, the causal result recomputed in the backward sweep), without checkpoints
    (EU_HIP_IIR_STREAM=3) and with one thread per line (0). `big` is +-1e34 at degree 5 (see the head of this file)"""
    prj, w, h, hfov = SETUP[shape]
    for nch in (1, 3, 4):
        img = image(cls, prj, w, h, nch, seed=nch, degree=degree)
        if cls == "big" and degree > pv.BIG_PREFILTER_MAX:
            img = pv.big(h, w, nch, seed=nch, top=pv.BIG_TOP_5)
        o = jobs.OracleSource(prj, w, h, hfov, img, degree)
        what = f"{cls} {shape} degree {degree} nch {nch}"
        assert np.isfinite(o.container).all(), what
        if cls == "impulse" and shape == "cube33":
            assert degree != 2 or pv.is_denormal(o.container).any(), what
        else:
            pv.assert_exercised(cls, o.container, degree, what)
            if cls == "impulse":
                # the tails are denormal across block edges of the streamed prefilter, whatever the blocks' alignment
                # (forward sweeps count from a line's start, backward ones from its end): at every one of the 64
                # alignments along an axis of 256 samples or more, at some along a shorter one
                for count, length in zip(pv.block_edge_alignments(o.container), (w, h)):
                    assert count == 64 if length >= 256 else count >= 1, (what, count, length)
        fct = ea.facet_spec(prj, w, h, hfov, nchannels=nch)
        for mode in (None, "3", "0"):
            if mode is None:
                monkeypatch.delenv("EU_HIP_IIR_STREAM", raising=False)
            else:
                monkeypatch.setenv("EU_HIP_IIR_STREAM", mode)
            g = ea.Source.load(fct, img, degree)
            pv.assert_bits(g.download(), o.container, f"{what} EU_HIP_IIR_STREAM {mode}")
            g.release()


def sample_tables(cls, bits):
    """a colour and an alpha table that hold the class"""
    n = 1 << bits
    return pv.make(cls, 1, n, 1, seed=bits).reshape(n).copy(), pv.make(cls, 1, n, 1, seed=bits + 1).reshape(n).copy()


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("cls", pv.FINITE)
def test_load_samples_with_tables_of_the_class(cls, bits):
    """integer samples decoded on the device through tables that hold the class: the container of
    OracleSource(table[samples]); degree 1 (the values themselves, braced) and degree 3 (prefiltered)"""
    colour, alpha = sample_tables(cls, bits)
    w, h = 67, 45
    for nch in (1, 3, 4):
        s = (pv.u32(h * w * nch, 5 + nch) % np.uint32(1 << bits)).astype(np.uint8 if bits == 8 else np.uint16).reshape(h, w, nch)
        px = colour[s]
        if nch == 4:
            px[..., 3] = alpha[s[..., 3]]
        for degree in (1, 3):
            o = jobs.OracleSource(euo.RECTILINEAR, w, h, 60.0, px, degree)
            what = f"{cls} {bits} bit nch {nch} degree {degree}"
            assert np.isfinite(o.container).all(), what
            if cls == "denormal":
                pv.assert_exercised(cls, o.container, degree, what)
            g = ea.Source.load_samples(ea.facet_spec(ea.RECTILINEAR, w, h, 60.0, nchannels=nch), s, colour, alpha,
                                       spline_degree=degree)
            pv.assert_bits(g.download(), o.container, what)
            g.release()


# ---- render: one case per kernel family, per class ---------------------------------------------------------------

LATLON = (euo.SPHERICAL, 256, 128, 360.0)


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("cls,degree", [(c, d) for c in pv.CLASSES for d in range(6) if c != "nonfinite" or d <= 3])
def test_general_kernel(cls, degree, direct, monkeypatch):
    """EU_HIP_KERNEL=1: the general kernel, staged through LDS and (EU_HIP_DIRECT=1) without; 1, 3 and 4 channels;
    `nonfinite` at degrees 0 to 3"""
    monkeypatch.setenv("EU_HIP_KERNEL", "1")
    if direct:
        monkeypatch.setenv("EU_HIP_DIRECT", "1")
    # targets that see the whole source: the share of denormals in the frame is then the source's
    tgt = (ea.CUBEMAP, 24, 144, 90.0) if degree % 2 else (ea.SPHERICAL, 200, 100, 360.0)
    for nch in (1, 3, 4):
        o, g = pair(cls, *LATLON, nch, degree)
        a = ea.arguments(*tgt, yaw=12, pitch=-33, roll=4, spline_degree=degree)
        check(cls, a, g, o, f"general {cls} degree {degree} nch {nch} direct {direct}")


@pytest.mark.parametrize("source", ["latlon", "cube"])
@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_packed_kernel(cls, degree, source, monkeypatch):
    """the packed kernels, 1 to 4 channels (EU_HIP_R4=0: never the staged ones); EU_HIP_HYBRID=2 splits a frame into
    runs wherever the layouts differ"""
    monkeypatch.setenv("EU_HIP_HYBRID", "2")
    monkeypatch.setenv("EU_HIP_R4", "0")          # cube sources of degree 2 and 3 go to the staged kernels by default
    for nch in (1, 2, 3, 4):
        if source == "latlon":
            o, g = pair(cls, *LATLON, nch, degree)
            a = ea.arguments(ea.CUBEMAP, 40, 240, 90.0, yaw=12, pitch=-33, roll=4, spline_degree=degree)
        else:
            o, g = pair(cls, euo.CUBEMAP, 64, 384, 90.0, nch, degree)
            a = ea.arguments(ea.SPHERICAL, 256, 128, 360.0, yaw=45, pitch=35.26, spline_degree=degree)
        check(cls, a, g, o, f"packed {cls} {source} degree {degree} nch {nch}")


STAGED_TARGETS = {"cubemap": (ea.CUBEMAP, 41, 246, 90.0), "rectilinear": (ea.RECTILINEAR, 200, 120, 100.0),
                  "spherical": (ea.SPHERICAL, 300, 150, 360.0)}
SWITCHES = [{}, {"EU_HIP_SHARE": "0"}, {"EU_HIP_BOXTAB": "0"}]


def staged(cls, o, g, a, nch, what, monkeypatch):
    ref = jobs.oracle_render(a, o)
    pv.assert_exercised(cls, ref, a.spline_degree, what)
    for sw in SWITCHES:
        for k in ("EU_HIP_SHARE", "EU_HIP_BOXTAB"):
            monkeypatch.delenv(k, raising=False)
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        pv.assert_class_bits(cls, ea.render(a, g, nch), ref, f"{what} {sw}")


@pytest.mark.parametrize("target", list(STAGED_TARGETS))
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_staged_kernel_latlon_source(cls, degree, target, monkeypatch):
    """EU_HIP_R4=1: the LDS-staging kernels, their column plans, the work list and the direct-gather kernel behind it,
    with shared rows and box tables as by default and each switched off; 3 and 4 channels, upright and rotated"""
    monkeypatch.setenv("EU_HIP_R4", "1")
    for nch in (3, 4):
        o, g = pair(cls, euo.SPHERICAL, 512, 256, 360.0, nch, degree)
        for ypr in ((0, 0, 0), (25, -10, 5)):
            a = ea.arguments(*STAGED_TARGETS[target], yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree)
            staged(cls, o, g, a, nch, f"staged {cls} {target} degree {degree} nch {nch} ypr {ypr}", monkeypatch)


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_staged_kernel_cube_source(cls, degree, monkeypatch):
    monkeypatch.setenv("EU_HIP_R4", "1")
    o, g = pair(cls, euo.CUBEMAP, 96, 576, 90.0, 3, degree)
    for a in (ea.arguments(ea.SPHERICAL, 400, 200, 360.0, spline_degree=degree),
              ea.arguments(ea.RECTILINEAR, 150, 110, 80.0, yaw=33, pitch=21, roll=-8, spline_degree=degree)):
        staged(cls, o, g, a, 3, f"staged {cls} cube source degree {degree} target {a.projection}", monkeypatch)


@pytest.mark.parametrize("twine", [2, 3])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_twining(cls, twine, monkeypatch):
    """the weighted sum over the taps, packed (lat/lon source) and general (EU_HIP_KERNEL=1) forms"""
    for degree, nch in ((1, 3), (3, 4), (3, 1)):
        o, g = pair(cls, *LATLON, nch, degree)
        a = ea.arguments(ea.SPHERICAL, 96, 48, 360.0, yaw=30, pitch=15, roll=7.5, spline_degree=degree, twine=twine)
        check(cls, a, g, o, f"twine {twine} {cls} degree {degree} nch {nch}")
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
        check(cls, a, g, o, f"twine {twine} {cls} degree {degree} nch {nch}, general")
        monkeypatch.delenv("EU_HIP_KERNEL")


@pytest.mark.parametrize("cls", pv.CLASSES)
def test_fisheye_mount_with_lens_polynomial(cls):
    """a 190 degree circular fisheye with the PTO polynomial, shift and shear, seen through a rectilinear window that
    it covers (so a frame of denormals stays one) and on the sphere (misses: exact zeros among the class)"""
    lens = dict(a=0.02, b=0.0, c=-0.01, h=0.01, v=-0.02, g=0.003, t=-0.002)
    for degree in (1, 3):
        o, g = pair(cls, euo.FISHEYE, 180, 180, 190.0, 3, degree, yaw=10, pitch=5, roll=-3, brighten=1.25, lens=lens)
        a = ea.arguments(ea.RECTILINEAR, 100, 80, 70.0, yaw=8, pitch=4, spline_degree=degree)
        check(cls, a, g, o, f"fisheye {cls} degree {degree}")
        a = ea.arguments(ea.SPHERICAL, 160, 80, 360.0, yaw=5, pitch=2, roll=1, spline_degree=degree)
        ref = check(cls, a, g, o, f"fisheye {cls} degree {degree} on the sphere", some=True)
        assert (jobs.bits(ref) == 0).all(axis=2).any(), "the sphere shows misses"


# ---- the value gates ----------------------------------------------------------------------------------------------

def alpha_seen(ref_alpha, what):
    """the alpha the oracle's frame holds is on every side of the gates: exact zeros, (0, 0.000001], above the gate,
    negative, above 1"""
    a = ref_alpha
    assert (a == 0).any() and ((a > 0) & (a <= pv.ALPHA_GATE)).any() and (a > pv.ALPHA_GATE).any(), what
    assert (a < 0).any() and (a > 1).any(), what


@pytest.mark.parametrize("src_n,out_n", [(s, t) for s in (1, 2, 3, 4) for t in (1, 2, 3, 4) if s != t])
def test_repix_with_the_alpha_plane(src_n, out_n):
    """repix_t's guarded division (alpha == 0 -> 0, else colour / alpha): alpha of both zeros, denormals (the quotient
    overflows to inf), negatives; degree 0 shows the plane's own values, degree 1 their blends; with twining"""
    for cls in ("hdr", "signed", "denormal", "nonfinite"):
        for degree in (0, 1):
            o, g = pair(cls, euo.RECTILINEAR, 128, 64, 100.0, src_n, degree, alpha=True, brighten=1.3)
            for twine in (0, 2):
                a = ea.arguments(ea.RECTILINEAR, 160, 80, 90.0, yaw=3, spline_degree=degree, twine=twine)
                check(cls, a, g, o, f"repix {src_n}->{out_n} {cls} degree {degree} twine {twine}", nch=out_n, some=True)
            if src_n in (2, 4) and cls != "nonfinite":
                a = ea.arguments(ea.RECTILINEAR, 160, 80, 90.0, yaw=3, spline_degree=degree)
                alpha_seen(jobs.oracle_render(a, o)[:, :, src_n - 1], f"repix {src_n} {cls} degree {degree}")


_facets = {}


def facets(cls, prj, w, h, hfov, nch, degree, count=6, lens=None, seed=0):
    """`count` facets looking front / right / back / left / up / down (then again, slightly turned), each another
    image of the class, with the alpha plane where they have alpha: (oracle sources, resident sources)"""
    key = (cls, prj, w, h, hfov, nch, degree, count, str(lens), seed)
    if key not in _facets:
        os_, gs = [], []
        for i in range(count):
            yaw, pitch, roll = VIEWS6[i % 6]
            kw = dict(yaw=yaw + 7.0 * (i // 6), pitch=pitch, roll=roll + 11.0 * (i // 6), brighten=1.0 + 0.05 * (i % 6), lens=lens)
            o, g = pair(cls, prj, w, h, hfov, nch, degree, alpha=True, seed=seed + 17 * i, **kw)
            os_.append(o)
            gs.append(g)
        _facets[key] = (os_, gs)
    return _facets[key]


@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_six_facet_panorama_with_alpha(cls, nch):
    """eu_synopsis (voronoi_syn_plus): layers composed through (1 - alpha) with alpha outside [0, 1], exactly 0 and
    exactly 1"""
    for degree in (0, 1):
        os_, gs = facets(cls, euo.RECTILINEAR, 80, 80, 100.0, nch, degree)
        for twine in (0, 2):
            a = ea.arguments(ea.SPHERICAL, 192, 96, 360.0, yaw=10, pitch=4, roll=-2, spline_degree=degree, twine=twine)
            ref = check(cls, a, gs, os_, f"six facets {cls} nch {nch} degree {degree} twine {twine}", nch=nch, some=True)
        if cls != "nonfinite":
            single = jobs.oracle_render(ea.arguments(ea.RECTILINEAR, 160, 160, 100.0, spline_degree=degree), os_[0])
            alpha_seen(single[:, :, nch - 1], f"facet 0 {cls} nch {nch}")
            assert (ref != 0).any()


@pytest.mark.parametrize("nch", [2, 4])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_seventy_two_tiny_facets_with_alpha(cls, nch):
    """eu_synopsis_big: more facets than mask bits, every layer found by a pass over all of them; 24 facets of 16 x 16
    three times over (equal z scores)"""
    os_, gs = facets(cls, euo.RECTILINEAR, 16, 16, 80.0, nch, 1, count=24)
    a = ea.arguments(ea.SPHERICAL, 96, 48, 360.0, yaw=7, spline_degree=1)
    check(cls, a, gs * 3, os_ * 3, f"72 facets {cls} nch {nch}", nch=nch, some=True)
    a = ea.arguments(ea.SPHERICAL, 65, 5, 360.0, spline_degree=1, twine=2)
    check(cls, a, gs * 3, os_ * 3, f"72 facets {cls} nch {nch} twined", nch=nch, some=True)


BRIGHTENS = (4.0, 1.0, 0.25)


def hdr_bracket(cls, nch, degree):
    """three exposures of one UNCLIPPED scene of the class seen by the same camera: scene / brighten, with the alpha
    plane (another one per exposure) where there is alpha. Nothing is clipped to [0, 1], so a grey value lies far
    beyond twice a facet's optimum and its quality is negative"""
    w, h = 96, 64
    scene = pv.make(cls, h, w, nch, seed=3)
    os_, gs = [], []
    for i, b in enumerate(BRIGHTENS):
        img = (scene / np.float32(b)).astype(np.float32)
        img = pv.with_alpha(img, seed=40 + i, associated=True)
        o = jobs.OracleSource(euo.RECTILINEAR, w, h, 70.0, img, degree, brighten=b)
        os_.append(o)
        gs.append(adopt(o, euo.RECTILINEAR, w, h, 70.0, nch, degree, brighten=b))
    return os_, gs


def hdr_conditions(os_, a1, nch, what):
    """tests/test_hdr_merge.numpy_hdr_merge run again on the facets' own pixels (single-facet renders of the oracle):
    some pixel's sum of qualities is <= 0, some pixel's is > 0, and with alpha some facet's alpha lies on either side
    of 0.000001, some is exactly 0 and some pixel's sum is exactly 0"""
    px = [jobs.oracle_render(a1, o) for o in os_]
    with np.errstate(all="ignore"):
        _, qsum = numpy_hdr_merge(px, BRIGHTENS, nch, with_qsum=True)
    assert (qsum <= 0).any() and (qsum > 0).any(), f"{what}: qsum <= 0 at {(qsum <= 0).sum()}, > 0 at {(qsum > 0).sum()} pixels"
    if nch in (2, 4):
        al = np.stack([v[:, :, nch - 1] for v in px])
        assert ((al > 0) & (al <= pv.ALPHA_GATE)).any() and (al > pv.ALPHA_GATE).any() and (al == 0).any(), what
        assert (qsum == 0).any(), what


@pytest.mark.parametrize("degree", [0, 1, 3])
@pytest.mark.parametrize("nch", [1, 2, 3, 4])
@pytest.mark.parametrize("cls", ["hdr", "signed"])
def test_hdr_merge_unclipped(cls, nch, degree):
    """eu_synopsis_hdr: the gates `a > 0.000001f`, `a == 0.0f` over a group of 16 lanes, `qsum > 0`, and std::max's
    operand order, with qualities that go negative and sums of them that are negative, zero and near zero"""
    os_, gs = hdr_bracket(cls, nch, degree)
    # the same camera as the facets, the frame a multiple of 16 wide: at degree 0 and 1 the groups of 16 lanes see
    # the alpha plane's own groups - all zero, partly zero, free of zeros
    a = ea.arguments(ea.RECTILINEAR, 96, 64, 70.0, spline_degree=degree, synopsis="hdr_merge")
    ref = jobs.oracle_render(a, os_)
    pv.assert_bits(ea.render(a, gs, nch), ref, f"hdr_merge {cls} nch {nch} degree {degree}")
    a1 = ea.arguments(ea.RECTILINEAR, 96, 64, 70.0, spline_degree=degree)
    hdr_conditions(os_, a1, nch, f"hdr_merge {cls} nch {nch} degree {degree}")
    if nch in (2, 4) and degree < 2:
        kinds = pv.group_kinds(jobs.oracle_render(a1, os_[0])[:, :, nch - 1])
        assert min(kinds) > 0, f"groups of 16 all zero / partly / free of zeros: {kinds}"
    # a rotated, wider target with twining: holes, and facets seen at an angle
    b = ea.arguments(ea.RECTILINEAR, 150, 100, 90.0, yaw=2, pitch=1, roll=-3, spline_degree=degree, twine=2, synopsis="hdr_merge")
    pv.assert_bits(ea.render(b, gs, nch), jobs.oracle_render(b, os_), f"hdr_merge {cls} nch {nch} degree {degree}, rotated, twined")


@pytest.mark.parametrize("mix,out_n", [((3, 4), 4), ((2, 4, 1, 3), 4), ((4, 3), 3), ((4, 2), 2), ((3, 1), 1)])
@pytest.mark.parametrize("cls", ["hdr", "signed", "nonfinite"])
def test_mixed_channel_counts_in_one_job(cls, mix, out_n):
    """every facet adapts through repix_t inside the synopsis; panorama and hdr_merge"""
    sets = {n: facets(cls, euo.RECTILINEAR, 72, 72, 95.0, n, 1, seed=21) for n in set(mix)}
    os_ = [sets[mix[i % len(mix)]][0][i] for i in range(6)]
    gs = [sets[mix[i % len(mix)]][1][i] for i in range(6)]
    for synopsis in ("panorama", "hdr_merge"):
        a = ea.arguments(ea.SPHERICAL, 176, 88, 360.0, yaw=20, pitch=-6, roll=3, spline_degree=1, synopsis=synopsis)
        check(cls, a, gs, os_, f"mixed {mix}->{out_n} {cls} {synopsis}", nch=out_n, some=True)


# ---- the other entry points: one general and one packed case each ------------------------------------------------

VIEWS = [(0.0, 0.0, 0.0), (30.0, 15.0, 7.5), (-40.0, 20.0, -5.0, 270.0)]


def view_args(target, view, **kw):
    tprj, tw, th, thfov = target
    return ea.arguments(tprj, tw, th, view[3] if len(view) == 4 else thfov, yaw=view[0], pitch=view[1], roll=view[2], **kw)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_render_views(cls, general, monkeypatch):
    """three views of one resident source in one call, one with another hfov, against the oracle's frame of each"""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    degree = 3 if cls != "nonfinite" else 1
    target = (ea.SPHERICAL, 130, 65, 360.0)
    o, g = pair(cls, *LATLON, 3, degree)
    got = ea.render_views(ea.arguments(*target, spline_degree=degree), VIEWS, g)
    for k, v in enumerate(VIEWS):
        ref = jobs.oracle_render(view_args(target, v, spline_degree=degree), o)
        pv.assert_class_bits(cls, got[k], ref, f"render_views {cls} view {k} general {general}")
        pv.assert_exercised(cls, ref, degree, f"render_views {cls} view {k}")


@pytest.mark.parametrize("synopsis", ["panorama", "hdr_merge"])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_render_views_multi(cls, synopsis):
    """three views of a six-facet job with alpha in one call"""
    target = (ea.SPHERICAL, 130, 65, 360.0)
    for nch in (3, 4):
        os_, gs = facets(cls, euo.FISHEYE, 64, 64, 140.0, nch, 1, lens=LENS)
        got = ea.render_views(ea.arguments(*target, spline_degree=1, synopsis=synopsis), VIEWS, gs, nchannels=nch)
        for k, v in enumerate(VIEWS):
            ref = jobs.oracle_render(view_args(target, v, spline_degree=1, synopsis=synopsis), os_, nch=nch)
            pv.assert_class_bits(cls, got[k], ref, f"render_views_multi {cls} {synopsis} nch {nch} view {k}")
            pv.assert_exercised(cls, ref, 1, f"render_views_multi {cls} {synopsis} nch {nch} view {k}", some=True)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("cls", pv.CLASSES)
def test_render_rays(cls, general, monkeypatch):
    """`act` alone at the oracle's own rays of a job (3 inputs) and at its ninepacks with the job's taps (9)"""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    degree = 3 if cls != "nonfinite" else 1
    o, g = pair(cls, *LATLON, 3, degree)
    a = ea.arguments(ea.SPHERICAL, 200, 100, 360.0, yaw=30, pitch=15, roll=7.5, spline_degree=degree)
    ref = jobs.oracle_render(a, o)
    pv.assert_class_bits(cls, ea.render_rays(g, jobs.oracle_render(a, o, stage=1)), ref, f"render_rays {cls}, 3 inputs")
    pv.assert_exercised(cls, ref, degree, f"render_rays {cls}")
    a = ea.arguments(ea.RECTILINEAR, 129, 97, 90.0, yaw=30, pitch=15, roll=7.5, spline_degree=degree, twine=2)
    nine = np.concatenate([jobs.oracle_render(a, o, stage=k) for k in (1, 3, 4)], axis=2)
    ref = jobs.oracle_render(a, o)
    pv.assert_class_bits(cls, ea.render_rays(g, nine, taps=a.twine_spread), ref, f"render_rays {cls}, 9 inputs")
    pv.assert_exercised(cls, ref, degree, f"render_rays {cls}, 9 inputs")


# ---- tethered words: the clamp gate and the truncation of to_screen --------------------------------------------

@pytest.mark.parametrize("nch", [1, 2, 3, 4])
@pytest.mark.parametrize("cls", pv.FINITE)
def test_tethered_words(cls, nch):
    """the finite classes scaled so that channels fall below 0, at -0, at 0, inside (0, 1), at 1 and above 1 - alpha
    included, which the other tests hold at 1 or inside [0, 1] - packed and general kernels, degree 1 (the values
    themselves at texel centres, and their blends) and degree 3. NaN is left out: see the head of this file."""
    for degree in (1, 3):
        img = pv.scaled_unit(cls, 128, 256, nch, seed=nch)
        o = jobs.OracleSource(euo.SPHERICAL, 256, 128, 360.0, img, degree)
        g = adopt(o, euo.SPHERICAL, 256, 128, 360.0, nch, degree)
        for tprj, tw, th, thfov in [(ea.SPHERICAL, 256, 128, 360.0), (ea.RECTILINEAR, 333, 77, 90.0)]:
            a = ea.arguments(tprj, tw, th, thfov, spline_degree=degree, tethered=True)
            got, ref = ea.render(a, g), jobs.oracle_render(a, o)
            assert got.dtype == np.uint32 and got.shape == (th, tw)
            assert np.array_equal(got, ref), f"{cls} nch {nch} degree {degree}: {(got != ref).sum()} words differ"
            if tprj == ea.SPHERICAL:
                # the source's own grid: the floats behind the words are on every side of both clamps
                f = jobs.oracle_render(ea.arguments(tprj, tw, th, thfov, spline_degree=degree), o)
                assert (f > 1).any() and ((f > 0) & (f < 1)).any() and (f == 0).any(), "the floats behind the words"
                assert (f < 0).any() or cls == "impulse" and degree == 1
                assert ((ref & 0xFF) == 0).any() and ((ref & 0xFF) == 255).any()
                assert len(np.unique(ref & 0xFF)) > 50 or cls == "impulse"
        o2 = jobs.OracleSource(euo.RECTILINEAR, 200, 150, 80.0, pv.scaled_unit(cls, 150, 200, nch, seed=7), degree)
        g2 = adopt(o2, euo.RECTILINEAR, 200, 150, 80.0, nch, degree)
        a = ea.arguments(ea.SPHERICAL, 300, 150, 360.0, spline_degree=degree, twine=2, tethered=True, crop=(100, 220, 40, 110))
        assert np.array_equal(ea.render(a, g2), jobs.oracle_render(a, o2)), f"{cls} nch {nch}: general kernel, twined, cropped"
