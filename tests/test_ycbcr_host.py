"""eu_hip_ycbcr_floats (ycbcr_floats), the host statement of the Y'CbCr feed, without a device. 1: bit for bit the
numpy float32 model of tests/ycbcr_model.py - tables looked up with numpy.take, products and sums as separate float32
operations - over 8- and 16-bit samples, every chroma subsampling, planar and interleaved chroma in both orders, padded
pitches, the smallest frames and both channel counts. 2: against the definitions - the reference codes of BT.709
limited range, and a round trip of a 17^3 grid of RGB through an 8-bit encode written here in float64 from Kr / Kb,
within the bound the quantisation and the matrix give. 3: ycbcr_matrix and ycbcr_tables are their float64 formulas.
4: the header's host loop as a stand-alone program over heap planes of exactly the frame's bytes
(tests/csrc/ycbcr_demo.cc: the program to build with -fsanitize=address,undefined when the loop changes)."""
import os
import subprocess

import numpy as np
import pytest

import envutil_amd as ea
import ycbcr_model as ym

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(w, h) for w in (1, 2, 3, 5) for h in (1, 2, 3, 5)] + [(64, 7)]
K = {"601": (0.299, 0.114), "709": (0.2126, 0.0722), "2020": (0.2627, 0.0593)}


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("bits", [8, 16])
def test_floats_equal_the_numpy_model(bits, nch):
    rng = np.random.default_rng(bits + nch)
    tables = [ea.ycbcr_tables(bits), ym.random_tables(rng, bits)]
    if bits == 16:
        tables.append(ea.ycbcr_tables(16, depth=10, msb_aligned=True))       # P010
    n = 0
    for (w, h) in SIZES:
        for sub_x in (1, 2):
            for sub_y in (1, 2):
                for layout in ("planar", "nv12", "nv21"):
                    for pad in (0, 3):
                        yt, ct = tables[n % len(tables)]
                        m = ea.ycbcr_matrix(("601", "709", "2020")[n % 3])
                        y, cb, cr = ym.planes(rng, h, w, sub_x, sub_y, bits, layout, pad)
                        got = ea.ycbcr_floats(y, (cb, cr), m, yt, ct, nch)
                        want = ym.floats(y, cb, cr, sub_x, sub_y, yt, ct, m, nch)
                        what = (w, h, sub_x, sub_y, layout, pad)
                        assert got.shape == (h, w, nch), what
                        assert (bits_of(got) == bits_of(want)).all(), what
                        n += 1
    assert n == len(SIZES) * 2 * 2 * 3 * 2


def test_interleaved_array_is_the_pair_of_its_halves():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (7, 9)).astype(np.uint8)
    c = rng.integers(0, 256, (4, 5, 2)).astype(np.uint8)
    m = ea.ycbcr_matrix("709")
    a = ea.ycbcr_floats(y, c, m, None, None)
    b = ea.ycbcr_floats(y, (c[..., 0].copy(), c[..., 1].copy()), m, None, None)
    assert (bits_of(a) == bits_of(b)).all()
    yt, ct = ea.ycbcr_tables(8)
    assert (bits_of(a) == bits_of(ym.floats(y, c[..., 0], c[..., 1], 2, 2, yt, ct, m))).all()
    with pytest.raises(ea.EuError):
        ea.ycbcr_floats(y, c[:3], m, None, None)          # 3 chroma rows fit neither 7 nor 4


def test_reference_codes_of_bt709_limited_range():
    m = ea.ycbcr_matrix("709")
    yt, ct = ea.ycbcr_tables(8)
    y = np.array([[235, 16]], np.uint8)
    c = np.array([[128, 128]], np.uint8)
    got = ea.ycbcr_floats(y, (c, c.copy()), m, yt, ct)
    assert (bits_of(got[0, 0]) == bits_of(np.ones(3, np.float32))).all()
    assert (bits_of(got[0, 1]) == bits_of(np.zeros(3, np.float32))).all()


@pytest.mark.parametrize("name", ["601", "709", "2020"])
def test_round_trip_of_an_rgb_grid_within_the_quantisation_bound(name):
    """RGB in [0, 1] -> 8-bit limited-range codes by the definitions, in float64 -> the library at 4:4:4. A code is
    off its exact value by at most half a step: 0.5 / 219 of luma, 0.5 / 224 of chroma, which the matrix scales; the
    float32 table entries, products and sums add at most four roundings of values below 2."""
    kr, kb = K[name]
    kg = 1.0 - kr - kb
    g = np.linspace(0.0, 1.0, 17)
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    yy = kr * rgb[:, 0] + kg * rgb[:, 1] + kb * rgb[:, 2]
    pb = (rgb[:, 2] - yy) / (2.0 * (1.0 - kb))
    pr = (rgb[:, 0] - yy) / (2.0 * (1.0 - kr))
    cy = np.rint(16.0 + 219.0 * yy).astype(np.uint8).reshape(1, -1)
    cb = np.rint(128.0 + 224.0 * pb).astype(np.uint8).reshape(1, -1)
    cr = np.rint(128.0 + 224.0 * pr).astype(np.uint8).reshape(1, -1)
    m = ea.ycbcr_matrix(name)
    got = ea.ycbcr_floats(cy, (cb, cr), m, *ea.ycbcr_tables(8)).reshape(-1, 3).astype(np.float64)
    m_rv, m_gu, m_gv, m_bu = (abs(float(v)) for v in m)
    fl = 4.0 * 2.0 ** -23
    bound = (0.5 / 219 + m_rv * 0.5 / 224 + fl, 0.5 / 219 + (m_gu + m_gv) * 0.5 / 224 + fl, 0.5 / 219 + m_bu * 0.5 / 224 + fl)
    err = np.abs(got - rgb).max(axis=0)
    print(name, "max error", err, "bound", bound)
    for c in range(3):
        assert err[c] <= bound[c], (name, c, err[c], bound[c])


def test_matrix_and_tables_are_their_formulas():
    for name, (kr, kb) in K.items():
        kg = 1.0 - kr - kb
        want = np.array([2 * (1 - kr), -2 * kb * (1 - kb) / kg, -2 * kr * (1 - kr) / kg, 2 * (1 - kb)]).astype(np.float32)
        assert (bits_of(np.array(ea.ycbcr_matrix(name), np.float32)) == bits_of(want)).all()
    with pytest.raises(ea.EuError):
        ea.ycbcr_matrix("240")
    for bits, depth, full, msb in ((8, 8, False, False), (8, 8, True, False), (16, 10, False, False), (16, 10, False, True),
                                   (16, 12, True, True), (16, 16, False, False)):
        yt, ct = ea.ycbcr_tables(bits, depth, full, msb)
        v = np.arange(1 << bits)
        c = (v >> (bits - depth) if msb else v).astype(np.float64)
        s = 2.0 ** (depth - 8)
        if full:
            wy, wc = c / (2.0 ** depth - 1), (c - 128 * s) / (2.0 ** depth - 1)
        else:
            wy, wc = (c - 16 * s) / (219 * s), (c - 128 * s) / (224 * s)
        assert (bits_of(yt) == bits_of(wy.astype(np.float32))).all() and (bits_of(ct) == bits_of(wc.astype(np.float32))).all()
    d8, d16 = ea.ycbcr_tables(8), ea.ycbcr_tables(16)
    assert d8[0].shape == (256,) and d16[1].shape == (65536,)


def test_host_loop_over_planes_of_exactly_their_bytes_host_program():
    exe = os.path.join(ROOT, "envutil_amd", "build", "ycbcr_demo")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "csrc", "ycbcr_demo.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout and "432 cases" in r.stdout
