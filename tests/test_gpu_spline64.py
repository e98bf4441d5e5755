"""The HIP library's pixels at spline degrees 0 to 9 against the float64 spline of tests/spline64.py - never against
the oracle, which this module does not load. Source.load builds the coefficients on the device, so the library's own
bracing and prefilter (three and four poles from degree 6 on) are in the product, and so are the run-time-degree
evaluator and, through render_layers, its copy.

ea.render(a, g, stage=2) gives the library's float32 source coordinates, ea.render(a, g) the pixels; the model is
evaluated in float64 at those coordinates. It has no split of a coordinate into a whole number and a fraction, so
the evaluator's rounding rule (floor for odd, round for even degrees) is not shared.

There is no number of the GPU's own: the tolerance is BIN_MARGIN x ENVELOPES64[(kind, degree)], which the CPU oracle
measures over these same jobs (tests/test_spline64_oracle.py), and the library is bit-identical to the oracle. At
least half of every frame hits the source, every miss is exactly zero, no hit is left out: the targets were chosen
for that and the CPU module checks it with the oracle."""
import pytest

import envutil_amd as ea
import spline64 as s64

pytestmark = pytest.mark.gpu

_sources = {}


def load(name, nch, degree):
    key = (name, nch, degree)
    if key not in _sources:
        kind, prj, w, h, hfov, lens = s64.SOURCES[name]
        spec = ea.facet_spec(prj, w, h, hfov, nchannels=nch, lens=lens)
        _sources[key] = ea.Source.load(spec, s64.source_image(name, nch), degree)
    return _sources[key]


@pytest.fixture(scope="module", autouse=True)
def release_sources():
    yield
    for s in _sources.values():
        s.release()
    _sources.clear()


def check(frame, crd, name, kind, degree, nch, what):
    err, share, miss = s64.compare(frame, crd, s64.source_model(name, nch, degree))
    print(what, kind, degree, nch, f"{err:.3g}", "bound", s64.tolerance(kind, degree), "hit", share)
    assert share >= 0.5, what
    assert miss == 0.0, what
    assert err <= s64.tolerance(kind, degree), f"{what}: {err:.3g} > {s64.tolerance(kind, degree):.3g}"


CASES = s64.gpu_cases()
FAMILIES = {"default": {}, "general": {"EU_HIP_KERNEL": "1"}}


@pytest.mark.parametrize("name", list(s64.SOURCES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_render(family, name, monkeypatch):
    """degrees 0 to 9 at 3 channels, 1 and 4 channels at degree 9; what the library picks by itself and the general
    kernel by name"""
    for k, v in FAMILIES[family].items():
        monkeypatch.setenv(k, v)
    n = 0
    for cname, kind, target, degree, nch in CASES:
        if cname != name:
            continue
        g = load(name, nch, degree)
        a = s64.make_args(target, degree)
        check(ea.render(a, g), ea.render(a, g, stage=2), name, kind, degree, nch, f"{family} {name} -> {target}")
        n += 1
    assert n == 2 * 12


@pytest.mark.parametrize("name", list(s64.SOURCES))
def test_render_layers(name):
    """render_layers with two layers runs the evaluator's copy (eu_render_layers.hip). The second layer holds the
    negative of the picture, so a kernel that gave both layers the first one's pixels would be far off; each layer
    is held to the model of its own samples"""
    kind, prj, w, h, hfov, lens = s64.SOURCES[name]
    n = 0
    for cname, ckind, target, degree, nch in s64.layer_cases():
        if cname != name:
            continue
        first = load(name, nch, degree)
        second = ea.Source.load(ea.facet_spec(prj, w, h, hfov, nchannels=nch, lens=lens),
                                s64.source_image(name, nch, negative=True), degree)
        try:
            a = s64.make_args(target, degree)
            out = ea.render_layers(a, [first, second])
            crd = ea.render(a, first, stage=2)
            check(out[0], crd, name, kind, degree, nch, f"layers {name}, layer 0")
            err, share, miss = s64.compare(out[1], crd, s64.source_model(name, nch, degree, negative=True))
            print("layers", name, "layer 1", degree, nch, f"{err:.3g}", "bound", s64.tolerance(kind, degree))
            assert share >= 0.5 and miss == 0.0 and err <= s64.tolerance(kind, degree), (name, degree, nch, err)
        finally:
            second.release()
        n += 1
    assert n == 12
