"""Stream order around a container that is refilled in place ("A source refilled in place"): a reload goes
behind every render that still reads the container and behind the library's own stream, every render goes behind the
reloads of its sources, and the scratch of a reload is the next reload's only behind it. Every sequence issues its
calls back to back on several streams with no synchronisation between them, then eu_hip_sync() and
torch.cuda.synchronize(), and every output must be, bit for bit, what the same job gives alone.

None of these tests loops to provoke a race, and none should be "strengthened" with repetition: they pin results and
return codes for call sequences."""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
import jobs
import ycbcr_model as ym

pytestmark = pytest.mark.gpu

W, H = 1024, 512


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def pictures(torch):
    """three 1024 x 512 lat/lon RGB pictures that differ in every pixel, on the host and on the device"""
    host = [jobs.synth_image(W, H, 3, seed=s) for s in (11, 22, 33)]
    dev = [torch.from_numpy(p).to("cuda:0") for p in host]
    torch.cuda.synchronize()
    return host, dev


FCT = ea.facet_spec(ea.SPHERICAL, W, H, 360.0)
CUBE = ea.arguments(ea.CUBEMAP, 96, 576, 90.0, spline_degree=3)
RECT = ea.arguments(ea.RECTILINEAR, 64, 32, 90.0, yaw=30.0, pitch=10.0, spline_degree=3)


def render_dev(torch, args, src, stream):
    """eu_hip_render into a new device tensor, on `stream` (None: the library's own); returns the tensor at once"""
    out = torch.zeros((args.height, args.width, 3), device="cuda:0", dtype=torch.float32)
    t = args.target(3)
    rc = ea.lib().eu_hip_render(C.byref(t), (C.c_void_p * 1)(src.handle), 1, C.c_void_p(out.data_ptr()), args.width * 12, 1,
                                C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == 0, ea.lib().eu_hip_last_error()
    return out


def settle(torch):
    assert ea.lib().eu_hip_sync() == 0, ea.lib().eu_hip_last_error()
    torch.cuda.synchronize()


def same(t, want, what):
    got = t.cpu().numpy() if hasattr(t, "cpu") else t
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} floats differ"


@pytest.fixture(scope="module")
def wanted(pictures):
    host, _ = pictures
    out = []
    for p in host:
        s = ea.Source.load(FCT, p, 3)
        out.append({"cube": ea.render(CUBE, s), "rect": ea.render(RECT, s), "container": s.download()})
    return out


def test_render_behind_reload_behind_render_on_three_streams(torch, pictures, wanted):
    """render picture 0 on s1, reload picture 1 on s2, render on s3, reload picture 2 on s1, render on the library's
    stream: every render shows the picture that was current when it was called"""
    _, dev = pictures
    src = ea.Source.load(FCT, pictures[0][0], 3)
    s1, s2, s3 = (torch.cuda.Stream() for _ in range(3))
    torch.cuda.synchronize()
    a = render_dev(torch, CUBE, src, s1)
    src.reload(dev[1], stream=s2)
    b = render_dev(torch, CUBE, src, s3)
    c = render_dev(torch, RECT, src, s3)
    src.reload(dev[2], stream=s1.cuda_stream)
    d = render_dev(torch, CUBE, src, None)
    settle(torch)
    same(a, wanted[0]["cube"], "render on s1 before the first reload")
    same(b, wanted[1]["cube"], "render on s3 behind the reload on s2")
    same(c, wanted[1]["rect"], "second render on s3")
    same(d, wanted[2]["cube"], "render on the library's stream behind the reload on s1")
    same(src.download(), wanted[2]["container"], "the container at the end")


def test_reload_on_the_library_stream_between_renders_on_callers_streams(torch, pictures, wanted):
    _, dev = pictures
    src = ea.Source.load(FCT, pictures[0][0], 3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a = render_dev(torch, CUBE, src, s1)
    b = render_dev(torch, RECT, src, None)
    src.reload(dev[1])                      # device pixels, no stream: queued on the library's own, nothing waits
    c = render_dev(torch, CUBE, src, s2)
    d = render_dev(torch, RECT, src, None)
    settle(torch)
    same(a, wanted[0]["cube"], "render on s1 before the reload")
    same(b, wanted[0]["rect"], "render on the library's stream before the reload")
    same(c, wanted[1]["cube"], "render on s2 behind the reload")
    same(d, wanted[1]["rect"], "render on the library's stream behind the reload")


def test_two_sources_share_the_scratch_on_two_streams(torch):
    """two cubemap sources reloaded back to back on two streams: the faces of both go through ONE scratch buffer"""
    face = 128
    fct = ea.facet_spec(ea.CUBEMAP, face, 6 * face, 90.0)
    imgs = [jobs.synth_cubefaces(face, 3, seed=100 + s) for s in range(4)]
    dev = [torch.from_numpy(np.ascontiguousarray(p)).to("cuda:0") for p in imgs]
    want = [ea.Source.load(fct, p, 3).download() for p in imgs]
    srcs = [ea.Source.load(fct, imgs[0], 3), ea.Source.load(fct, imgs[1], 3)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    srcs[0].reload(dev[2], stream=s1)
    srcs[1].reload(dev[3], stream=s2)
    srcs[0].reload(dev[1], stream=s2)
    settle(torch)
    same(srcs[1].download(), want[3], "second source, reloaded on s2")
    same(srcs[0].download(), want[1], "first source, reloaded on s1 and then on s2")


def test_decoder_surfaces_to_views_without_a_host_synchronisation(torch):
    """NV12 surfaces on the device -> reload_ycbcr -> render_views, frame after frame on one stream, nothing between
    the calls: every frame's views are those of a fresh load of that frame"""
    rng = np.random.default_rng(9)
    w, h = 512, 256
    fct = ea.facet_spec(ea.SPHERICAL, w, h, 360.0)
    m = ea.ycbcr_matrix("709")
    args = ea.arguments(ea.RECTILINEAR, 96, 64, 80.0, spline_degree=3)
    views = [(0, 0, 0), (120, 20, 0), (-60, -30, 10)]
    frames = [ym.planes(rng, h, w, 2, 2, 8, "nv12") for _ in range(3)]
    want = [ea.render_views(args, views, ea.Source.load_ycbcr(fct, y, (cb, cr), m, spline_degree=3)) for y, cb, cr in frames]
    surfaces = []
    for y, cb, cr in frames:
        nv = np.stack([cb, cr], -1)
        surfaces.append((torch.from_numpy(np.ascontiguousarray(y)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(nv)).to("cuda:0")))
    src = ea.Source.load_ycbcr(fct, frames[0][0], (frames[0][1], frames[0][2]), m, spline_degree=3)
    outs = [torch.zeros(want[0].shape, device="cuda:0", dtype=torch.float32) for _ in frames]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    src.reload_ycbcr(surfaces[0][0], surfaces[0][1], m, stream=st)      # uploads the tables, once
    for k in range(3):
        src.reload_ycbcr(surfaces[k][0], surfaces[k][1], m, stream=st)
        ea.render_views(args, views, src, out=outs[k], stream=st.cuda_stream)
    settle(torch)
    for k in range(3):
        same(outs[k], want[k], f"views of frame {k}")


def test_a_stream_the_caller_has_destroyed(torch, pictures, wanted):
    """a reload on a stream that is destroyed once its work is done: the next reload, the next render and
    eu_hip_sync() return 0 - the library waits on events of its own and keeps no handle of the stream"""
    _, dev = pictures
    src = ea.Source.load(FCT, pictures[0][0], 3)
    hip = ea.lib()
    for f, at in ((hip.hipStreamCreate, [C.POINTER(C.c_void_p)]), (hip.hipStreamSynchronize, [C.c_void_p]),
                  (hip.hipStreamDestroy, [C.c_void_p])):
        f.restype, f.argtypes = C.c_int, at
    h = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(h)) == 0
    torch.cuda.synchronize()
    src.reload(dev[1], stream=h.value)
    assert hip.hipStreamSynchronize(h) == 0
    assert hip.hipStreamDestroy(h) == 0
    a = render_dev(torch, CUBE, src, None)
    src.reload(dev[2])
    b = render_dev(torch, RECT, src, torch.cuda.Stream())
    settle(torch)
    same(a, wanted[1]["cube"], "render behind the reload on the stream that is gone")
    same(b, wanted[2]["rect"], "render behind the next reload")
    ea.reload_scratch_release()
