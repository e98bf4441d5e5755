"""envutil_hip --ray_map FILE: the single facet's image evaluated at the rays of a 3-channel PFM. GPU: the file
written holds the bits of ea.render_rays on the same rays. CPU: what the option cannot honour - an orientation,
a second facet, explicit twining - is refused with a message, not an abort."""
import numpy as np
import pytest

import envutil_amd as ea
from test_cli import bits, cli, read_pfm, synth, write_pfm  # noqa: F401  (cli is a fixture)


def some_rays(w, h, seed=5):
    """unnormalised rays all over the sphere"""
    rng = np.random.default_rng(seed)
    r = rng.normal(0.0, 1.0, (h, w, 3)).astype(np.float32)
    return r * rng.uniform(0.25, 4.0, (h, w, 1)).astype(np.float32)


FACET = ["--facet", "a.pfm", "spherical", "360", "0", "0", "0"]


# ---------------------------------------------------------------------------------- CPU

def test_refusals_are_messages(cli, tmp_path):
    write_pfm(tmp_path / "a.pfm", synth(64, 32, 3))
    write_pfm(tmp_path / "b.pfm", synth(64, 32, 3, seed=1))
    write_pfm(tmp_path / "rays.pfm", some_rays(33, 9))
    tail = ["--ray_map", "rays.pfm", "--output", "o.pfm"]
    cases = [
        (["--facet", "a.pfm", "spherical", "360", "10", "0", "0"] + tail, "yaw / pitch / roll"),
        (["--facet", "a.pfm", "spherical", "360", "0", "-5", "0"] + tail, "yaw / pitch / roll"),
        (["--facet", "a.pfm", "spherical", "360", "0", "0", "0.5"] + tail, "yaw / pitch / roll"),
        (FACET + ["--yaw", "30"] + tail, "yaw / pitch / roll"),
        (FACET + ["--pitch", "3"] + tail, "yaw / pitch / roll"),
        (FACET + ["--roll", "-3"] + tail, "yaw / pitch / roll"),
        (FACET + ["--facet", "b.pfm", "spherical", "360", "0", "0", "0"] + tail, "2 facets"),
        (FACET + ["--twine", "2"] + tail, "--twine"),
        (FACET + ["--twine", "5"] + tail, "--twine"),
    ]
    for argv, what in cases:
        r = cli(argv, tmp_path)
        assert r.returncode == 2, (argv, r.returncode, r.stderr)          # an error status, not a signal
        assert "--ray_map" in r.stderr and what in r.stderr, (argv, r.stderr)
        assert not (tmp_path / "o.pfm").exists()
    # a map that is no 3-channel PFM, and a missing one
    write_pfm(tmp_path / "grey.pfm", synth(33, 9, 1))
    r = cli(FACET + ["--ray_map", "grey.pfm", "--output", "o.pfm"], tmp_path)
    assert r.returncode == 2 and "3-channel PFM" in r.stderr
    r = cli(FACET + ["--ray_map", "nope.pfm", "--output", "o.pfm"], tmp_path)
    assert r.returncode == 2 and r.stderr.strip()
    # --twine 0 / 1 and no --twine are accepted as far as the arguments go: without a device the job then
    # fails with the library's message, with one it is rendered
    for extra in ([], ["--twine", "0"], ["--twine", "1"]):
        r = cli(FACET + extra + tail, tmp_path)
        if ea.device_count() > 0:
            assert r.returncode == 0, r.stderr
        else:
            assert r.returncode == 1 and "no HIP device" in r.stderr, (extra, r.returncode, r.stderr)


# ---------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("prj,w,h,hfov,nch,degree", [("spherical", 256, 128, 360.0, 3, 3),
                                                     ("rectilinear", 129, 97, 80.0, 4, 1),
                                                     ("cubemap", 32, 192, 90.0, 3, 2)])
def test_ray_map_file_holds_render_rays_bits(cli, tmp_path, prj, w, h, hfov, nch, degree):
    img = synth(w, h, nch, seed=3)
    write_pfm(tmp_path / "a.pfm", img)
    rays = some_rays(129, 97)
    rays[5, 7] = 0.0                       # a null ray and a non-finite one: misses
    rays[50, 128] = (np.nan, 1.0, 1.0)
    write_pfm(tmp_path / "rays.pfm", rays)
    r = cli(["--facet", "a.pfm", prj, str(hfov), "0", "0", "0", "--degree", str(degree),
             "--ray_map", "rays.pfm", "--output", "o.pfm"], tmp_path)
    assert r.returncode == 0, r.stderr
    got = read_pfm(tmp_path / "o.pfm")
    fct = ea.facet_spec(ea.api.PROJECTION_NAMES.index(prj), w, h, hfov, nchannels=nch)
    want = ea.render_rays(ea.Source.load(fct, img, degree), rays)
    assert got.shape == want.shape == (97, 129, nch)
    assert (bits(got) == bits(want)).all()
    assert (want[5, 7] == 0).all() and (want[50, 128] == 0).all() and (want != 0).any()
