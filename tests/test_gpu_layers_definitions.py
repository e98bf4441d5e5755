"""ea.render_layers against the float64 model of tests/definitions64.py: two layers carrying two DIFFERENT polynomial
scenes, each held to the model of its own scene within that file's ENVELOPES - so the reference of the layered call
is not only the library's other path (tests/test_gpu_layers.py). The second scene is the first with its colour
channels rotated: polynomials of the same rows of coefficients, so the measured envelopes apply to it unchanged.
A layer that picked up the other's texels, weights or coordinates would be off by the scenes' difference, about 0.1."""
import numpy as np
import pytest

import definitions64 as d
import envutil_amd as ea

pytestmark = pytest.mark.gpu


def rolled_fields(rays, nch):
    """the scene of layer 1: channel c shows the polynomial of channel (c + 1) % 3"""
    assert nch == 3
    out = np.empty(rays.shape[:-1] + (nch,))
    for c in range(nch):
        out[..., c] = d.field(rays, (c + 1) % 3)
    return out


SCENES = (d.fields, rolled_fields)


@pytest.mark.parametrize("general", [False, True])
def test_two_layers_two_scenes(general, monkeypatch):
    """a lat/lon source pair at degree 3 onto the sphere (rotated), the upright cubemap and a window across the seam
    and a pole, in both kernel forms"""
    if general:
        monkeypatch.setenv("EU_HIP_KERNEL", "1")
    f, degree, nch = d.LATLON[256], 3, 3
    spec = ea.facet_spec(f.prj, f.w, f.h, f.hfov, nchannels=nch)
    rays = d.pixel_rays(f)
    layers = [ea.Source.load(spec, scene(rays, nch).astype(np.float32), degree) for scene in SCENES]
    try:
        for t, ypr in ((d.T_SPH, d.ROTATED), (d.T_CUBE48, d.UPRIGHT), (d.T_RECT, (170.0, 60.0, 10.0))):
            a = d.make_args(t, ypr, degree)
            out = ea.render_layers(a, layers)
            assert out.shape == (2, t[2], t[1], nch)
            assert np.abs(out[0] - out[1]).max() > 0.05, "the two layers show the same scene"
            for k, scene in enumerate(SCENES):
                j = d.judge(out[k], a, [f], nch, want=d.expected(a, nch, scene=scene))
                print("layer", k, t, ypr, "general", general, j.bins(), "outside", j.outside_max)
                assert j.covered_share >= 0.5 and j.outside_max == 0.0
                d.assert_within(j, d.kind_of(f), degree, f"layer {k} -> {t} {ypr} general {general}")
    finally:
        for s in layers:
            s.release()
