"""The command line on Radiance pictures: a .hdr / .pic facet goes to the device as the file's quads and is decoded
there (io::read_rgbe -> eu_hip_source_load_rgbe), a .hdr / .pic output leaves it as quads (eu_hip_render_rgbe ->
io::write_rgbe). The files hold, byte for byte, what the float route gives: the same job from a PFM of the decoded
floats, and the numpy model's encoding (tests/rgbe_model.py) of the same job's .pfm."""
import numpy as np
import pytest

from test_cli import cli, write_pfm, read_pfm, rle_scanline      # noqa: F401  (cli: the fixture)
import rgbe_model as rm

pytestmark = pytest.mark.gpu

TO_CUBE = ["--projection", "cubemap", "--hfov", "90", "--width", "32", "--degree", "3", "--twine", "0"]


def write_hdr(path, q, packed=False, meta=b""):
    h, w = q.shape[:2]
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n" + meta + b"\n-Y %d +X %d\n" % (h, w)
    path.write_bytes(head + (b"".join(rle_scanline(q[y]) for y in range(h)) if packed else q.tobytes()))


def hdr_body(path, w, h):
    raw = path.read_bytes()
    head, body = raw.split(b"-Y %d +X %d\n" % (h, w), 1)
    return head, np.frombuffer(body, np.uint8).reshape(h, w, 4)


def env_quads(w=128, h=64, seed=12):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    q[..., 3] = rng.integers(120, 136, (h, w))
    q[3, 5:20] = 0                                   # black pixels, zero exponent
    return q


def test_hdr_facet_equals_pfm_of_its_decoded_floats(cli, tmp_path):
    q = env_quads()
    write_hdr(tmp_path / "flat.hdr", q)
    write_hdr(tmp_path / "packed.pic", q, packed=True)
    write_pfm(tmp_path / "env.pfm", rm.decode(q))
    out = {}
    for name in ("flat.hdr", "packed.pic", "env.pfm"):
        r = cli(["-v", "--facet", name, "spherical", "360", "0", "0", "0"] + TO_CUBE + ["--output", name[:-4] + "_cube.pfm"], tmp_path)
        assert r.returncode == 0, r.stderr
        out[name] = r.stdout
    assert "flat.hdr: RGBE pixels, decoded on the device" in out["flat.hdr"]
    assert "packed.pic: RGBE pixels, decoded on the device" in out["packed.pic"]
    assert "env.pfm: float pixels" in out["env.pfm"]
    want = (tmp_path / "env_cube.pfm").read_bytes()
    assert (tmp_path / "flat_cube.pfm").read_bytes() == want and (tmp_path / "packed_cube.pfm").read_bytes() == want
    assert len(set(want)) > 100


def test_hdr_facet_in_another_colour_space(cli, tmp_path):
    """--input_colour_space sRGB: the table route on the device, against the host's conversion of the PFM's floats"""
    q = env_quads(seed=13)
    q[..., 3] = 120 + q[..., 3] % 9                 # values up to 1, where the curve bends
    write_hdr(tmp_path / "env.hdr", q)
    write_pfm(tmp_path / "env.pfm", rm.decode(q))
    for name in ("env.hdr", "env.pfm"):
        r = cli(["-v", "--facet", name, "spherical", "360", "0", "0", "0", "--input_colour_space", "sRGB"] + TO_CUBE
                + ["--output", name[-3:] + "_cube.pfm"], tmp_path)
        assert r.returncode == 0, r.stderr
        assert f"converting {name} from sRGB to" in r.stdout
    assert (tmp_path / "hdr_cube.pfm").read_bytes() == (tmp_path / "pfm_cube.pfm").read_bytes()


def test_hdr_output_holds_the_models_encoding_of_the_pfm(cli, tmp_path):
    q = env_quads(seed=14)
    write_hdr(tmp_path / "env.hdr", q, packed=True)
    job = ["-v", "--facet", "env.hdr", "spherical", "360", "0", "0", "0"] + TO_CUBE
    r = cli(job + ["--output", "cube.pfm"], tmp_path)
    assert r.returncode == 0, r.stderr
    r = cli(job + ["--output", "cube.hdr"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "saved cube.hdr (32 x 192 x 3): RGBE pixels, encoded on the device" in r.stdout, r.stdout
    head, body = hdr_body(tmp_path / "cube.hdr", 32, 192)
    assert head == b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nProjection=cubemap\nHfov=90\n\n"
    frame = read_pfm(tmp_path / "cube.pfm")
    assert np.array_equal(body, rm.encode(frame)) and len(np.unique(body[..., 3])) > 4
    # six face files, a cropped row range of rectilinear, .pic
    r = cli(job + ["--output", "face_%s.hdr"], tmp_path)
    assert r.returncode == 0 and "encoded on the device" in r.stdout, r.stdout + r.stderr
    for k, name in enumerate(("left", "right", "top", "bottom", "front", "back")):
        head, face = hdr_body(tmp_path / f"face_{name}.hdr", 32, 32)
        assert np.array_equal(face, body[32 * k:32 * (k + 1)]), name
        assert b"Projection=rectilinear\nHfov=90\n" in head
    view = ["-v", "--facet", "env.hdr", "spherical", "360", "0", "0", "0", "--projection", "rectilinear", "--hfov", "80",
            "--width", "65", "--height", "33", "--yaw", "20", "--degree", "3", "--twine", "2"]
    assert cli(view + ["--output", "view.pfm"], tmp_path).returncode == 0
    r = cli(view + ["--output", "view.pic"], tmp_path)
    assert r.returncode == 0 and "encoded on the device" in r.stdout, r.stdout + r.stderr
    assert np.array_equal(hdr_body(tmp_path / "view.pic", 65, 33)[1], rm.encode(read_pfm(tmp_path / "view.pfm")))


def test_pipe_mode_keeps_an_rgbe_asset_resident(cli, tmp_path):
    write_hdr(tmp_path / "pano.hdr", env_quads(seed=15))
    jobs = "--yaw 0 --output v0.hdr\n--yaw 45 --output v45.hdr\n--yaw 45 --output v45.pfm\n"
    r = cli(["-v", "--facet", "pano.hdr", "spherical", "360", "0", "0", "0", "--projection", "rectilinear", "--hfov", "80",
             "--width", "96", "--height", "64", "--degree", "2", "--twine", "0", "-"], tmp_path, stdin=jobs)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("RGBE pixels, decoded on the device") == 1 and r.stdout.count("already resident") == 2
    assert r.stdout.count("RGBE pixels, encoded on the device") == 2
    a, b = hdr_body(tmp_path / "v0.hdr", 96, 64)[1], hdr_body(tmp_path / "v45.hdr", 96, 64)[1]
    assert not np.array_equal(a, b)
    assert np.array_equal(b, rm.encode(read_pfm(tmp_path / "v45.pfm")))


def test_ray_map_and_srgb_output_keep_the_float_route(cli, tmp_path):
    q = env_quads(seed=16)
    write_hdr(tmp_path / "env.hdr", q)
    facet = ["-v", "--facet", "env.hdr", "spherical", "360", "0", "0", "0", "--degree", "1"]
    rays = np.zeros((9, 14, 3), np.float32)
    rays[..., 0] = np.linspace(-1, 1, 14)[None, :]
    rays[..., 1] = np.linspace(-0.5, 0.5, 9)[:, None]
    rays[..., 2] = 1.0
    write_pfm(tmp_path / "rays.pfm", rays)
    assert cli(facet + ["--ray_map", "rays.pfm", "--output", "looked.pfm"], tmp_path).returncode == 0
    r = cli(facet + ["--ray_map", "rays.pfm", "--output", "looked.hdr"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "looked.hdr: float pixels, encoded on the host (a ray map's output)" in r.stdout, r.stdout
    assert "encoded on the device" not in r.stdout
    assert np.array_equal(hdr_body(tmp_path / "looked.hdr", 14, 9)[1], rm.encode(read_pfm(tmp_path / "looked.pfm")))
    # an output colour space that is not the working one: the host converts the floats, then encodes them
    r = cli(facet + TO_CUBE[:-4] + ["--twine", "0", "--output_colour_space", "sRGB", "--output", "srgb.hdr"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "srgb.hdr: float pixels, encoded on the host (the output's colour space is not the working one)" in r.stdout, r.stdout
    r = cli(facet + TO_CUBE[:-4] + ["--twine", "0", "--output", "linear.hdr"], tmp_path)
    assert r.returncode == 0 and "encoded on the device" in r.stdout, r.stdout + r.stderr
    assert not np.array_equal(hdr_body(tmp_path / "srgb.hdr", 32, 192)[1], hdr_body(tmp_path / "linear.hdr", 32, 192)[1])
    # four channels: write_one's message, as ever
    r = cli(facet + TO_CUBE[:-4] + ["--twine", "0", "--nchannels", "4", "--output", "four.hdr"], tmp_path)
    assert r.returncode != 0 and "3 channels" in r.stderr
