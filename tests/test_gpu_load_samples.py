"""Integer samples as a source (eu_hip_source_load_samples, eu_decode.hip; Source.load_samples): the container is,
bit for bit, the one the float route builds from table[samples] gathered with numpy. Containers are compared as
uint32, so NaN entries of a table compare too. Sizes are chosen for the kernel's paths: a thread owns four floats
of a destination row behind the row's first 16-byte boundary, one thread the floats in front of it, and the
samples come out of aligned dwords - so odd widths, three channels and rows at every byte alignment matter."""
import numpy as np
import pytest

import envutil_amd as ea

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 63, 64, 65, 67, 257)
HEIGHTS = (1, 2, 3, 17)
MAXVAL16 = 1000


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tables(bits, seed=1):
    """distinct random colour and alpha tables: a swapped table or channel shows"""
    rng = np.random.default_rng(seed + bits)
    n = 1 << bits
    colour = (rng.random(n) * 2.0 - 0.5).astype(np.float32)
    alpha = (rng.random(n) + 2.0).astype(np.float32)
    return colour, alpha


def make_samples(h, w, nch, bits, seed):
    """random samples that hold, as far as the size allows, all 256 values, or 0, 1, maxval, maxval + 1 and 65535"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << bits, (h, w, nch), dtype=np.uint8 if bits == 8 else np.uint16)
    flat = s.reshape(-1)
    special = rng.permutation(256).astype(np.uint8) if bits == 8 else np.array([65535, 0, 1, MAXVAL16, MAXVAL16 + 1], np.uint16)
    k = min(flat.size, special.size)
    pos = rng.permutation(flat.size)[:k]
    flat[pos] = special[:k]
    return s


def gather(s, colour, alpha):
    """the float image of the samples: the alpha table for the last of 2 or 4 channels"""
    px = colour[s]
    if s.shape[2] in (2, 4):
        px[..., -1] = alpha[s[..., -1]]
    return np.ascontiguousarray(px, np.float32)


def flat_facet(w, h, nch):
    return ea.facet_spec(ea.RECTILINEAR, w, h, 60.0, nchannels=nch)


def same_container(a, b, what):
    ca, cb = a.download(), b.download()
    assert ca.shape == cb.shape, what
    bad = int((bits_of(ca) != bits_of(cb)).sum())
    assert bad == 0, f"{what}: {bad} of {ca.size} floats differ"


def check(fct, s, bits, degree, what, big_endian=False, pixels=None, **edit):
    colour, alpha = tables(bits)
    want = ea.Source.load(fct, gather(s, colour, alpha) if pixels is None else pixels, degree, **edit)
    given = s.byteswap() if big_endian else s             # the same values, stored high byte first
    got = ea.Source.load_samples(fct, given, colour, alpha, big_endian=big_endian, spline_degree=degree, **edit)
    same_container(got, want, what)


@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_flat_8_bit(nch):
    for h in HEIGHTS:
        for w in WIDTHS:
            check(flat_facet(w, h, nch), make_samples(h, w, nch, 8, 100 * h + w), 8, 1, (w, h, nch))


@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("nch", [1, 3, 4])
def test_flat_16_bit(nch, big_endian):
    for h in HEIGHTS:
        for w in WIDTHS:
            check(flat_facet(w, h, nch), make_samples(h, w, nch, 16, 100 * h + w), 16, 1, (w, h, nch, big_endian), big_endian)


@pytest.mark.parametrize("degree", [0, 1, 3])
def test_degrees(degree):
    for w, h in ((5, 3), (65, 17), (67, 2), (257, 3)):
        for nch, bits in ((3, 8), (4, 8), (2, 8), (3, 16), (4, 16)):
            check(flat_facet(w, h, nch), make_samples(h, w, nch, bits, w + nch), bits, degree, (w, h, nch, bits, degree), bits == 16)


def test_nan_table_entries():
    """no prefilter at degree 1: a NaN stays where its sample is, with its payload"""
    s = make_samples(17, 65, 4, 8, 3)
    colour, alpha = tables(8)
    colour[s[0, 0, 0]] = np.float32(np.nan)
    alpha.view(np.uint32)[s[3, 5, 3]] = 0x7fc01234
    fct = flat_facet(65, 17, 4)
    got = ea.Source.load_samples(fct, s, colour, alpha, spline_degree=1)
    same_container(got, ea.Source.load(fct, gather(s, colour, alpha), 1), "NaN entries")
    assert np.isnan(got.download()).any()


def test_default_tables():
    """without tables both are v / maxval in float32"""
    s = make_samples(9, 33, 4, 8, 5)
    fct = flat_facet(33, 9, 4)
    same_container(ea.Source.load_samples(fct, s, spline_degree=3), ea.Source.load(fct, s.astype(np.float32) / np.float32(255), 3), "8 bit")
    same_container(ea.Source.load_samples(fct, s, maxval=100, spline_degree=3), ea.Source.load(fct, s.astype(np.float32) / np.float32(100), 3), "maxval 100")
    s = make_samples(9, 33, 3, 16, 6)
    fct = flat_facet(33, 9, 3)
    same_container(ea.Source.load_samples(fct, s.astype(">u2"), spline_degree=3), ea.Source.load(fct, s.astype(np.float32) / np.float32(65535), 3), "16 bit, a big-endian array")


@pytest.mark.parametrize("bits", [8, 16])
def test_spherical_and_window(bits):
    """the periodic prefilter and, for the tiny sizes, the sequential brace; a rectilinear window of a larger image"""
    for w, h in ((2, 1), (4, 2), (64, 32)):
        for nch in (3, 4):
            fct = ea.facet_spec(ea.SPHERICAL, w, h, 360.0, nchannels=nch)
            check(fct, make_samples(h, w, nch, bits, w), bits, 3, ("spherical", w, h, nch), bits == 16)
    fct = ea.facet_spec(ea.RECTILINEAR, 200, 100, 70.0, nchannels=3, window=(67, 45, 20, 10))
    check(fct, make_samples(45, 67, 3, bits, 8), bits, 3, "window", bits == 16)


@pytest.mark.parametrize("bits", [8, 16])
def test_channel_gain(bits):
    """1 -> 2 and 3 -> 4 without an edit: the new channel is 1.0"""
    colour, alpha = tables(bits)
    for w, h in ((1, 1), (3, 2), (65, 17), (67, 5)):
        for pch in (1, 3):
            fct = flat_facet(w, h, pch + 1)
            s = make_samples(h, w, pch, bits, w + pch)
            px = np.concatenate([colour[s], np.ones((h, w, 1), np.float32)], 2)
            check(fct, s, bits, 3, ("gain", w, h, pch), bits == 16, pixels=px)
            # ... and against the float route's own way of gaining the channel
            check(fct, s, bits, 1, ("gain, edited float route", w, h, pch), bits == 16, pixels=colour[s])


@pytest.mark.parametrize("size", [(67, 45), (300, 200)])
def test_edit(size):
    """PTO masks and an elliptic crop, 3 -> 4 and 4 -> 4, against Source.load(..., masks=, crop=) on the gathered floats"""
    w, h = size
    poly = [(np.array([0.1, 0.7, 0.5, 0.2]) * w, np.array([0.2, 0.1, 0.8, 0.6]) * h)]
    crop = (w // 10, w - w // 8, h // 9, h - h // 7)
    for pch in (3, 4):
        for bits in (8, 16):
            fct = ea.facet_spec(ea.FISHEYE, w, h, 120.0, nchannels=4)
            s = make_samples(h, w, pch, bits, w + pch + bits)
            check(fct, s, bits, 3, ("edit", size, pch, bits), bits == 16, masks=poly, crop=crop, crop_kind=2)
            check(fct, s, bits, 1, ("mask only", size, pch, bits), False, masks=poly)


@pytest.mark.parametrize("bits", [8, 16])
def test_cubemap(bits):
    for face in (5, 16):
        fct = ea.facet_spec(ea.CUBEMAP, face, 6 * face, 90.0)
        check(fct, make_samples(6 * face, face, 3, bits, face), bits, 3, ("cubemap", face, bits), bits == 16)


def test_device_samples():
    """a torch uint8 tensor, views of one that start at byte offsets 1 and 3, a uint16 tensor"""
    import torch
    colour, alpha = tables(8)
    for nch, w, h in ((3, 67, 9), (4, 64, 5), (1, 257, 3)):
        s = make_samples(h, w, nch, 8, nch)
        fct = flat_facet(w, h, nch)
        want = ea.Source.load(fct, gather(s, colour, alpha), 3)
        for offset in (0, 1, 3):
            flat = torch.zeros(s.size + 8, dtype=torch.uint8, device="cuda:0")
            t = flat[offset:offset + s.size].view(h, w, nch)
            t.copy_(torch.from_numpy(s))
            assert t.data_ptr() % 4 == offset
            same_container(ea.Source.load_samples(fct, t, colour, alpha, spline_degree=3), want, ("device", nch, offset))
    colour, alpha = tables(16)
    s = make_samples(9, 67, 3, 16, 2)
    fct = flat_facet(67, 9, 3)
    want = ea.Source.load(fct, gather(s, colour, alpha), 3)
    flat = torch.zeros(2 * s.size + 8, dtype=torch.uint8, device="cuda:0")
    for offset in (0, 2):                                   # 16-bit samples lie at even addresses
        t8 = flat[offset:offset + 2 * s.size]
        t8.copy_(torch.from_numpy(s.reshape(-1).view(np.uint8)))
        t = t8.view(torch.uint16).view(9, 67, 3)
        assert t.data_ptr() % 4 == offset
        same_container(ea.Source.load_samples(fct, t, colour, alpha, spline_degree=3), want, ("device, 16 bit", offset))
    # masks on device samples
    fct = ea.facet_spec(ea.RECTILINEAR, 67, 9, 60.0, nchannels=4)
    poly = [(np.array([5.0, 40.0, 30.0]), np.array([1.0, 2.0, 8.0]))]
    want = ea.Source.load(fct, gather(s, colour, alpha), 3, masks=poly)
    same_container(ea.Source.load_samples(fct, t, colour, alpha, spline_degree=3, masks=poly), want, "device, masked")


def test_many_workgroups():
    """the wide path for many workgroups"""
    check(flat_facet(1024, 512, 3), make_samples(512, 1024, 3, 8, 1), 8, 3, "1024 x 512 x 3, 8 bit")
    check(flat_facet(1024, 512, 4), make_samples(512, 1024, 4, 16, 2), 16, 3, "1024 x 512 x 4, 16 bit", True)


FEED_CASES = {
    # name: (facet, plane width, plane height) - the smallest shapes at which the loader's branches differ
    "window": (lambda: ea.facet_spec(ea.RECTILINEAR, 300, 200, 80.0, nchannels=4, window=(131, 77, 40, 30)), 131, 77),
    "fullsphere": (lambda: ea.facet_spec(ea.SPHERICAL, 6, 3, 360.0, nchannels=4), 6, 3),
    "cubemap": (lambda: ea.facet_spec(ea.CUBEMAP, 64, 384, 90.0, nchannels=4), 64, 384),
}


@pytest.mark.parametrize("name", sorted(FEED_CASES))
def test_every_feed_builds_the_same_container(name):
    """One load pipeline, three feeds, five ways in: host floats and a device float tensor (through the edit), host
    and device uint8 samples, host big-endian uint16 samples of the same values with a 65536-entry table that starts
    with the 8-bit one. 3-channel input, 4-channel facet, degree 3. With a mask polygon and an elliptic crop all five
    containers are, bit for bit, Source.load of the floats widened and edited on the host; without an edit (the facet
    only gains its channel) they are the plain load of the widened floats, the sixth feed. The container's pitch
    differs from the plane's (window), the periodic prefilter with the sequential pole rows and brace runs
    (fullsphere), the face scratch and the cube build are used (cubemap)."""
    import torch
    make_facet, w, h = FEED_CASES[name]
    fct = make_facet()
    s = make_samples(h, w, 3, 8, 7 * w + h)
    colour, _ = tables(8)
    colour16 = np.concatenate([colour, tables(16)[0][256:]])
    assert colour16.shape == (65536,) and (bits_of(colour16[:256]) == bits_of(colour)).all()
    floats = np.ascontiguousarray(colour[s], np.float32)
    wide = np.concatenate([floats, np.ones((h, w, 1), np.float32)], 2)
    s16 = s.astype(np.uint16).byteswap()                   # the same values, 16 bit, stored high byte first
    poly = [(np.array([0.2, 0.7, 0.5], np.float32) * w, np.array([0.2, 0.3, 0.8], np.float32) * h)]
    crop = (w // 10, w - w // 8, h // 9, h - h // 7)
    ran = 0
    for edit in (dict(masks=poly, crop=crop, crop_kind=2), {}):
        prepared = wide.copy()
        if edit:
            ea.facet_alpha(prepared, poly, crop, 2)        # the library's host function, in place
            assert (prepared != wide).any(), "the edit changes something"
        want = ea.Source.load(fct, prepared, 3)            # eu_hip_source_load
        feeds = [
            ("host floats", lambda: ea.Source.load(fct, floats, 3, **edit)),
            ("device floats", lambda: ea.Source.load(fct, torch.from_numpy(floats).to("cuda:0"), 3, **edit)),
            ("host uint8", lambda: ea.Source.load_samples(fct, s, colour, spline_degree=3, **edit)),
            ("device uint8", lambda: ea.Source.load_samples(fct, torch.from_numpy(s).to("cuda:0"), colour,
                                                            spline_degree=3, **edit)),
            ("host uint16, big-endian", lambda: ea.Source.load_samples(fct, s16, colour16, big_endian=True,
                                                                       spline_degree=3, **edit)),
        ]
        if not edit:
            feeds.append(("plain load of the widened floats", lambda: ea.Source.load(fct, wide, 3)))
        first = None
        for what, load in feeds:
            got = load()
            same_container(got, want, (name, "edited" if edit else "channel gain", what))
            if first is not None:
                same_container(got, first, (name, what, "against", feeds[0][0]))
            first = first or got
            ran += 1
    assert ran == 11


def test_render():
    """spherical 256 x 128 to a 64-wide cubemap, degree 3: the same frame from either source"""
    colour, alpha = tables(8)
    s = make_samples(128, 256, 3, 8, 4)
    fct = ea.facet_spec(ea.SPHERICAL, 256, 128, 360.0)
    args = ea.arguments(ea.CUBEMAP, 64, 384, 90.0, spline_degree=3)
    got = ea.render(args, ea.Source.load_samples(fct, s, colour, alpha, spline_degree=3))
    want = ea.render(args, ea.Source.load(fct, gather(s, colour, alpha), 3))
    assert (bits_of(got) == bits_of(want)).all()
