"""The command line on PNM / PAM inputs: the file's integer samples go to the device as they are and are decoded
there (io::read_samples + io::sample_tables -> eu_hip_source_load_samples). The output files hold, byte for byte,
what the same job gives from a PFM with the floats q / maxval - that division is correctly rounded in numpy as
in the tables, so the two inputs are the same image."""
import numpy as np
import pytest

from test_cli import cli, write_pfm      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def test_ppm_equals_pfm_of_the_same_floats(cli, tmp_path):
    rng = np.random.default_rng(21)
    q = rng.integers(0, 256, (45, 67, 3), dtype=np.uint8)
    (tmp_path / "in.ppm").write_bytes(b"P6\n67 45\n255\n" + q.tobytes())
    write_pfm(tmp_path / "in.pfm", q.astype(np.float32) / np.float32(255))
    out = {}
    for name in ("in.ppm", "in.pfm"):
        r = cli(["-v", "--facet", name, "rectilinear", "70", "10", "5", "2", "--projection", "spherical", "--hfov", "360",
                 "--width", "128", "--degree", "3", "--twine", "0", "--input_colour_space", "Linear", "--output", "o_" + name[3:] + ".pfm"],
                tmp_path)
        assert r.returncode == 0, r.stderr
        out[name] = r.stdout
    assert "in.ppm: 8-bit samples, decoded on the device" in out["in.ppm"]
    assert "in.pfm: float pixels" in out["in.pfm"]
    assert (tmp_path / "o_ppm.pfm").read_bytes() == (tmp_path / "o_pfm.pfm").read_bytes()


def test_16_bit_rgba_pam_in_a_pto_with_mask_and_crop(cli, tmp_path):
    rng = np.random.default_rng(22)
    q = rng.integers(0, 65536, (160, 160, 4), dtype=np.uint16)
    head = b"P7\nWIDTH 160\nHEIGHT 160\nDEPTH 4\nMAXVAL 65535\nTUPLTYPE RGB_ALPHA\nENDHDR\n"
    (tmp_path / "b.pam").write_bytes(head + q.astype(">u2").tobytes())
    write_pfm(tmp_path / "b.pfm", q.astype(np.float32) / np.float32(65535))
    for ext in ("pam", "pfm"):
        (tmp_path / f"{ext}.pto").write_text(
            'p f2 w300 h150 v360 n"TIFF"\n'
            f'i w160 h160 f3 v170 y-100 p-20 r0 S10,150,10,150 n"b.{ext}"\n'
            'k i0 t0 p"30 20 120 25 140 110 40 100"\n')
        r = cli(["-v", "--pto", f"{ext}.pto", "--output", f"o_{ext}.pfm", "--degree", "3", "--twine", "0",
                 "--input_colour_space", "Linear"], tmp_path)
        assert r.returncode == 0, r.stderr
        assert (f"b.{ext}: 16-bit samples, decoded on the device" if ext == "pam" else f"b.{ext}: float pixels") in r.stdout
    a, b = (tmp_path / "o_pam.pfm").read_bytes(), (tmp_path / "o_pfm.pfm").read_bytes()
    assert a == b
    # the mask and the crop took effect: the output has transparent and opaque parts
    alpha = np.frombuffer(a.split(b"\n", 3)[3], "<f4").reshape(150, 300, 4)[..., 3]
    assert (alpha == 0).any() and (alpha > 0).any()


def test_pipe_mode_keeps_a_sample_asset_resident(cli, tmp_path):
    rng = np.random.default_rng(23)
    q = rng.integers(0, 256, (64, 128, 3), dtype=np.uint8)
    (tmp_path / "pano.ppm").write_bytes(b"P6\n128 64\n255\n" + q.tobytes())
    jobs = "--yaw 0 --output v0.pfm\n--yaw 45 --output v45.pfm\n"
    r = cli(["-v", "--facet", "pano.ppm", "spherical", "360", "0", "0", "0", "--projection", "rectilinear", "--hfov", "80",
             "--width", "96", "--height", "64", "--degree", "2", "--twine", "0", "-"], tmp_path, stdin=jobs)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("8-bit samples, decoded on the device") == 1 and "already resident" in r.stdout
    assert (tmp_path / "v0.pfm").exists() and (tmp_path / "v45.pfm").exists()
