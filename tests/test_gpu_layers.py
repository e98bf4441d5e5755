"""Many pictures of one geometry in one call: ea.render_layers (eu_hip_render_layers) against ea.render of every
layer alone, which is the library's existing path and itself pinned to the CPU oracle. Float32 bit patterns, 0 ULP,
no pixel left out. The layers take the geometries of test_gpu_rays.SOURCES with jobs.synth_image(..., seed=31 + k)
as layer k's picture."""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
import jobs
import pixel_values as pv
from test_gpu_parity import SRC_H, SRC_W, TARGETS, assert_bits
from test_gpu_rays import SOURCES
from test_gpu_views import GENERAL, PACKED, WIDTHS

pytestmark = pytest.mark.gpu

# The twined groups of the library as built (eu_hip_layers_group: EU_LAYERS_GROUP of eu_select.h). The shipped group
# is 1, and then the counts below are 1, 2 and 3: every group is full, and the partial last group of the twined
# kernels - `eu_layers_in_group() < EU_LAYERS_GROUP` - does NOT occur in this suite. It occurs, with a second group
# behind a full one, when the same tests run on a library built with -DEU_LAYERS_GROUP=2 or 4 (EU_HIP_LIB, a
# tools/mkvariant.sh library): the counts follow the library. tests/test_layers_host.py walks the group arithmetic
# the kernels call for groups of 1, 2 and 4 whatever the build.
G = int(ea.lib().eu_hip_layers_group())
assert G in (1, 2, 4)

_layers, _refs = {}, {}


def facet_of(name, nch=None, brighten=None):
    prj, w, h, hfov, n, degree, kw, _ = SOURCES[name]
    return ea.facet_spec(prj, w, h, hfov, nchannels=nch or n, yaw=kw.get("yaw", 0.0), pitch=kw.get("pitch", 0.0),
                         roll=kw.get("roll", 0.0), brighten=kw.get("brighten", 1.0) if brighten is None else brighten,
                         lens=kw.get("lens"))


def layers_of(name, count):
    """`count` sources of the geometry SOURCES[name], layer k carrying synth_image(seed=31 + k): made once, shared"""
    have = _layers.setdefault(name, [])
    prj, w, h, hfov, nch, degree, kw, _ = SOURCES[name]
    while len(have) < count:
        k = len(have)
        have.append(ea.Source.load(facet_of(name), jobs.synth_image(w, h, nch, seed=31 + k), degree))
    return have[:count]


def reference(key, g, a, nch=None):
    """ea.render of one layer. key: (name in SOURCES, layer index, ...) - computed once per (layer, job), shared,
    read-only; None for sources a test made for itself"""
    if key is None:
        return ea.render(a, g, nchannels=nch)
    if key not in _refs:
        r = ea.render(a, g, nchannels=nch)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def check_layers(name, layers, target, what, nch=None, distinct=True, check=assert_bits, **kw):
    tprj, tw, th, thfov = target
    a = ea.arguments(tprj, tw, th, thfov, yaw=30.0, pitch=15.0, roll=7.5, **kw)
    got = ea.render_layers(a, layers, nchannels=nch)
    assert got.shape == (len(layers), th, tw, nch or layers[0].fct.nchannels)
    for k, g in enumerate(layers):
        shared = name in SOURCES and g is layers_of(name, k + 1)[k]
        ref = reference((name, k, target, nch, tuple(sorted(kw.items()))) if shared else None, g, a, nch)
        check(got[k], ref, f"{what}: target {target}, layer {k} of {len(layers)}")
    # the comparison means something: the layers show different pictures
    assert not distinct or all((jobs.bits(got[k]) != jobs.bits(got[0])).any() for k in range(1, len(layers))), what
    return got


# ---- frames -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PACKED + GENERAL)
def test_every_layer_is_the_frame_of_render(name, monkeypatch):
    """all eight TARGETS, three layers per call; the packed-eligible sources again under EU_HIP_KERNEL=1"""
    degree = SOURCES[name][5]
    layers = layers_of(name, 3)
    for target in TARGETS:
        check_layers(name, layers, target, name, spline_degree=degree)
        if name in PACKED:
            monkeypatch.setenv("EU_HIP_KERNEL", "1")
            check_layers(name, layers, target, name + ", EU_HIP_KERNEL=1", spline_degree=degree)
            monkeypatch.delenv("EU_HIP_KERNEL")


@pytest.mark.parametrize("name", ["latlon d1 n3", "latlon d0"])
def test_tile_tails_and_second_segments(name):
    layers = layers_of(name, 3)
    for target in WIDTHS:
        check_layers(name, layers, target, name, spline_degree=SOURCES[name][5])


@pytest.mark.parametrize("name", ["latlon d3 n3", "rectilinear lens"])
@pytest.mark.parametrize("twine", [2, 3])
@pytest.mark.parametrize("count", sorted({1, G, G + 1, 2 * G + 1}))
def test_twining(name, twine, count):
    """a full group, a partial group, a second group; the targets the views test twines"""
    layers = layers_of(name, count)
    for target in [TARGETS[2], TARGETS[5], TARGETS[0], TARGETS[3], TARGETS[6]]:
        check_layers(name, layers, target, f"{name} twine {twine}", spline_degree=SOURCES[name][5], twine=twine)


def test_brighten_per_layer():
    """a bracket: colour channels scaled by the layer's own factor, alpha not"""
    name = "latlon d3 n4"
    w, h = SRC_W, SRC_H
    layers = [ea.Source.load(facet_of(name, brighten=b), pv.with_alpha(jobs.synth_image(w, h, 4, seed=31 + k), seed=3), 3)
              for k, b in enumerate((1.0, 0.8, 0.25))]
    for twine in (0, 2):
        kw = dict(twine=twine) if twine else {}
        for target in (TARGETS[2], TARGETS[0]):
            check_layers("bracket", layers, target, f"brighten, twine {twine}", spline_degree=3, **kw)
    a = ea.arguments(*TARGETS[2], yaw=30.0, pitch=15.0, roll=7.5, spline_degree=3)
    got = ea.render_layers(a, layers)
    plain = ea.render(a, ea.Source.load(facet_of(name), pv.with_alpha(jobs.synth_image(w, h, 4, seed=32), seed=3), 3))
    assert_bits(got[1][..., 3], plain[..., 3], "alpha is not brightened")
    assert (jobs.bits(got[1][..., :3]) != jobs.bits(plain[..., :3])).any()


@pytest.mark.parametrize("src_n,out_n", [(3, 4), (4, 1)])
def test_channel_adaption(src_n, out_n):
    def imgs(w, h):
        out = []
        for k in range(3):
            img = jobs.synth_image(w, h, src_n, seed=31 + k)
            if src_n == 4:
                img[:, :, 3] = (np.indices((h, w))[1] % (7 + k) != 0).astype(np.float32)
            out.append(img)
        return out
    fct = ea.facet_spec(ea.RECTILINEAR, 128, 64, 100.0, nchannels=src_n, brighten=1.3)
    layers = [ea.Source.load(fct, img, 1) for img in imgs(128, 64)]
    target = (ea.SPHERICAL, 150, 75, 360.0)
    check_layers(f"repix rect {src_n}", layers, target, f"repix {src_n}->{out_n}", nch=out_n, spline_degree=1)
    check_layers(f"repix rect {src_n}", layers, target, f"repix {src_n}->{out_n} twined", nch=out_n, spline_degree=1, twine=2)
    # and a source of the packed kind: channel adaption sends it through the general form
    fct = ea.facet_spec(ea.SPHERICAL, SRC_W, SRC_H, 360.0, nchannels=src_n)
    layers = [ea.Source.load(fct, img, 3) for img in imgs(SRC_W, SRC_H)]
    check_layers(f"repix latlon {src_n}", layers, TARGETS[2], f"repix {src_n}->{out_n}, lat/lon", nch=out_n, spline_degree=3)


@pytest.mark.parametrize("d", [0, 1, 3])
@pytest.mark.parametrize("general", [False, True])
def test_one_layer_does_not_leak_into_another(d, general, monkeypatch):
    """an ordinary picture, one with inf / NaN / +-3e38 texels, one of denormals and one of impulses side by side:
    every layer equals its own render. The non-finite picture runs at degrees 0 and 1, the denormal and impulse
    pictures at degree 3 (and ride along at the others)."""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    w, h = 64, 32
    fct = ea.facet_spec(ea.SPHERICAL, w, h, 360.0)
    pictures = [jobs.synth_image(w, h, 3, seed=31), pv.make("denormal", h, w, 3, seed=2), pv.make("impulse", h, w, 3, seed=2)]
    if d <= 1:
        pictures.insert(1, pv.make("nonfinite", h, w, 3, seed=2, one_in=20))
    layers = [ea.Source.load(fct, img, d) for img in pictures]
    for twine in (0, 2):
        kw = dict(twine=twine) if twine else {}
        for target in (TARGETS[2], TARGETS[1]):
            got = check_layers(f"leak d{d}", layers, target, f"values, degree {d}, twine {twine}", check=pv.assert_bits_nan,
                               spline_degree=d, **kw)
            assert np.isfinite(got[0]).all(), "the ordinary layer picked up a neighbour's non-finite texels"
            if d <= 1:
                assert not np.isfinite(got[1]).all()
            assert (np.abs(got[-2]) < 1e-37).all(), "the denormal layer picked up a neighbour's values"


# ---- layout -----------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-12345.5)
LAYOUT_TARGET = TARGETS[2]          # rectilinear 129 x 97
LAYOUT_NAME = "latlon d3 n3"


def layout_job(count=3, **kw):
    layers = layers_of(LAYOUT_NAME, count)
    a = ea.arguments(*LAYOUT_TARGET, yaw=30.0, pitch=15.0, roll=7.5, spline_degree=3, **kw)
    refs = [reference((LAYOUT_NAME, k, LAYOUT_TARGET, None, tuple(sorted(dict(spline_degree=3, **kw).items()))), g, a)
            for k, g in enumerate(layers)]
    return layers, a, refs


def test_one_layer_and_no_layer():
    layers, a, refs = layout_job()
    got = ea.render_layers(a, layers[1:2])
    assert got.shape == (1, 97, 129, 3)
    assert_bits(got[0], refs[1], "one layer")
    assert ea.render_layers(a, [], nchannels=3).shape == (0, 97, 129, 3)
    # no layer, and a buffer that could hold one: untouched
    buf = np.full((1, 97, 129, 3), SENTINEL, np.float32)
    t = a.target(3)
    arr = (C.c_void_p * 1)(layers[0].handle)
    rc = ea.lib().eu_hip_render_layers(C.byref(t), arr, 0, buf.ctypes.data, 129 * 12, 97 * 129 * 12, 0, None)
    assert rc == 0
    assert (buf == SENTINEL).all()


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("twine", [0, 2])
def test_padded_rows_and_layers_numpy(general, twine, monkeypatch):
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    layers, a, refs = layout_job(**(dict(twine=twine) if twine else {}))
    big = np.full((3, 97 + 2, 129 + 5, 3), SENTINEL, np.float32)
    out = big[:, :97, :129]
    assert ea.render_layers(a, layers, out=out) is out
    for k in range(3):
        assert_bits(np.ascontiguousarray(out[k]), refs[k], f"padded, layer {k}")
    assert (big[:, 97:] == SENTINEL).all() and (big[:, :, 129:] == SENTINEL).all(), "the padding of `out` was written"


@pytest.mark.parametrize("general", [False, True])
def test_torch_output_padding_and_stream(general, monkeypatch):
    import torch
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    layers, a, refs = layout_job()
    dev = torch.device("cuda")
    # dense, on the library's stream
    out_t = torch.full((3, 97, 129, 3), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert ea.render_layers(a, layers, out=out_t) is out_t
    ea.sync()
    for k in range(3):
        assert_bits(out_t[k].cpu().numpy(), refs[k], f"torch dense, layer {k}")
    # padded rows and layers, on a stream of the caller's
    big = torch.full((3, 97 + 1, 129 + 3, 3), float(SENTINEL), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ea.render_layers(a, layers, out=big[:, :97, :129], stream=stream.cuda_stream)
    ea.sync()
    host = big.cpu().numpy()
    for k in range(3):
        assert_bits(np.ascontiguousarray(host[k, :97, :129]), refs[k], f"torch padded, layer {k}")
    assert (host[:, 97:] == SENTINEL).all() and (host[:, :, 129:] == SENTINEL).all(), "the padding of `out` was written"


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("twine", [0, 2])
def test_chunks_give_the_same_bits(on_device, twine, monkeypatch):
    """five layers in one launch (EU_HIP_LAYERS_MAX=0), by default (four and one), and in launches of one and of two
    (the last one partial)"""
    import torch
    layers, a, refs = layout_job(5, **(dict(twine=twine) if twine else {}))

    def run():
        if not on_device:
            return ea.render_layers(a, layers)
        out_t = torch.zeros((5, 97, 129, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ea.render_layers(a, layers, out=out_t)
        ea.sync()
        return out_t.cpu().numpy()

    default = run()
    for k in range(5):
        assert_bits(default[k], refs[k], f"layer {k}")
    for most in ("0", "1", "2"):
        monkeypatch.setenv("EU_HIP_LAYERS_MAX", most)
        assert_bits(run(), default, f"EU_HIP_LAYERS_MAX={most} against the default")


def test_the_same_source_twice():
    layers, a, refs = layout_job()
    got = ea.render_layers(a, [layers[0], layers[1], layers[0]])
    assert_bits(got[0], refs[0], "first")
    assert_bits(got[1], refs[1], "second")
    assert_bits(got[2], refs[0], "the first source again")


def test_render_and_its_caches_are_left_alone(monkeypatch):
    """a staged job J through ea.render, render_layers on another stream, J again: the launch counter counts the
    renders alone, and J's frame has the same bits"""
    import torch
    layers, a, refs = layout_job()
    monkeypatch.setenv("EU_HIP_R4", "1")
    j = ea.arguments(*LAYOUT_TARGET, yaw=11, pitch=-7, roll=3, spline_degree=3)
    first = ea.render(j, layers[0])
    n1 = ea.launch_count()
    stream = torch.cuda.Stream()
    out_t = torch.zeros((3, 97, 129, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ea.render_layers(a, layers, out=out_t, stream=stream.cuda_stream)
    ea.render_layers(ea.arguments(*LAYOUT_TARGET, spline_degree=3, twine=2), layers)
    assert ea.launch_count() == n1
    again = ea.render(j, layers[0])
    assert ea.launch_count() > n1
    ea.sync()
    assert_bits(again, first, "the job after render_layers calls")
    for k in range(3):
        assert_bits(out_t[k].cpu().numpy(), refs[k], f"layer {k}")


def test_two_caller_streams_with_a_render_between():
    """layers on stream A, a render on the library's stream, other layers on stream B: the second call must not
    rewrite the tables or the layer table under the first"""
    import torch
    layers, a, refs = layout_job(5)
    j = ea.arguments(*LAYOUT_TARGET, yaw=11, pitch=-7, roll=3, spline_degree=3)
    b = ea.arguments(*LAYOUT_TARGET, yaw=-20.0, pitch=5.0, roll=0.0, spline_degree=3)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    out_a = torch.zeros((3, 97, 129, 3), dtype=torch.float32, device="cuda")
    out_b = torch.zeros((2, 97, 129, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ea.render_layers(a, layers[:3], out=out_a, stream=sa.cuda_stream)
    between = ea.render(j, layers[0])
    ea.render_layers(b, layers[3:], out=out_b, stream=sb.cuda_stream)
    ea.sync()
    torch.cuda.synchronize()
    for k in range(3):
        assert_bits(out_a[k].cpu().numpy(), refs[k], f"stream A, layer {k}")
    for k in range(2):
        assert_bits(out_b[k].cpu().numpy(), ea.render(b, layers[3 + k]), f"stream B, layer {k}")
    assert_bits(between, ea.render(j, layers[0]), "the render between")


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_layers_that_do_not_agree_are_named():
    img = jobs.synth_image(64, 32, 3)
    a = ea.arguments(ea.RECTILINEAR, 40, 30, 80.0, spline_degree=1)
    base = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 32, 70.0), img, 1)
    others = {
        "field of view": ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 32, 75.0), img, 1),
        "size": ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0), jobs.synth_image(64, 48, 3), 1),
        "spline degree": ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 32, 70.0), img, 3),
        "channel count": ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 32, 70.0, nchannels=4), jobs.synth_image(64, 32, 4), 1),
        "orientation": ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 32, 70.0, yaw=5.0), img, 1),
        "source parameters": ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 32, 70.0, lens=dict(a=0.01, b=0.0, c=0.0, h=0.0, v=0.0)), img, 1),
    }
    for what, other in others.items():
        with pytest.raises(ea.EuError, match=f"error -2.*layer 2 differs.*{what}"):
            ea.render_layers(a, [base, base, other, other])
    assert ea.render_layers(a, [base, base]).shape == (2, 30, 40, 3)


def test_mask_for_and_translated_layers_are_refused():
    img = jobs.synth_image(64, 32, 3)
    a = ea.arguments(ea.SPHERICAL, 64, 32, 360.0, spline_degree=1)
    plain = ea.Source.load(ea.facet_spec(ea.SPHERICAL, 64, 32, 360.0), img, 1)
    masked = ea.Source.load(ea.facet_spec(ea.SPHERICAL, 64, 32, 360.0, masked=1), img, 1)
    with pytest.raises(ea.EuError, match="error -2.*layer 1.*mask_for"):
        ea.render_layers(a, [plain, masked])
    g = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0, translation=dict(x=0.1, z=0.05)), jobs.synth_image(64, 48, 3), 1)
    with pytest.raises(ea.EuError, match="error -3.*translation.*layer 0"):
        ea.render_layers(a, [g, g])
