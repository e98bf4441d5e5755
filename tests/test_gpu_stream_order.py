"""The order between streams around the device buffers that outlive a call ("Buffers that outlive a
call"): stepper and tap tables, the staged kernels' plans and work list, the tethered frame buffer, the ray taps,
the alpha row plan. Every sequence issues its calls back to back on several streams with no synchronisation
between them, then eu_hip_sync() and torch.cuda.synchronize(), and every output must be, bit for bit, what the
same job gives alone.

None of these tests loops to provoke a race, and none should be "strengthened" with repetition: they pin results
and return codes for call sequences that the library once ordered through one saved stream handle - wrongly, or
not at all - and now orders through events of its own."""
import ctypes as C

import numpy as np
import pytest

import envutil_amd as ea
import jobs
from envutil_amd import api
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

W, H = 512, 256


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def sources():
    """two 512 x 256 lat/lon RGB sources of degree 3 that differ in every pixel"""
    fct = ea.facet_spec(ea.SPHERICAL, W, H, 360.0)
    return [ea.Source.load(fct, jobs.synth_image(W, H, 3, seed=s), 3) for s in (12345, 777)]


@pytest.fixture
def staged(monkeypatch):
    monkeypatch.setenv("EU_HIP_R4", "1")


def render_dev(torch, args, src, stream, och=3):
    """eu_hip_render into a new device tensor, on `stream` (None: the library's own); returns the tensor at once"""
    shape = (args.height, args.width) if args.tethered else (args.height, args.width, och)
    out = torch.zeros(shape, device="cuda:0", dtype=torch.int32 if args.tethered else torch.float32)
    t = args.target(3)
    rc = ea.lib().eu_hip_render(C.byref(t), (C.c_void_p * 1)(src.handle), 1, C.c_void_p(out.data_ptr()),
                                args.width * (1 if args.tethered else och) * 4, 1,
                                C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == 0, ea.lib().eu_hip_last_error()
    return out


def settle(torch):
    assert ea.lib().eu_hip_sync() == 0, ea.lib().eu_hip_last_error()
    torch.cuda.synchronize()


def rect(yaw=0.0, **kw):
    return ea.arguments(ea.RECTILINEAR, 64, 32, 90.0, yaw=yaw, pitch=10.0, spline_degree=3, **kw)


def cube(px):
    return ea.arguments(ea.CUBEMAP, px, 6 * px, 90.0, spline_degree=3)


def three_streams_one_slot(torch, src, key1, key2):
    """job A (key 1) on s1, job B (key 1) on the library's stream, job C (key 2) on s2: C rewrites the tables A reads"""
    want1, want2 = ea.render(key1, src, 3), ea.render(key2, src, 3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a = render_dev(torch, key1, src, s1)
    b = render_dev(torch, key1, src, None)
    c = render_dev(torch, key2, src, s2)
    settle(torch)
    assert_bits(a.cpu().numpy(), want1, "job A, key 1 on s1")
    assert_bits(b.cpu().numpy(), want1, "job B, key 1 on the library's stream")
    assert_bits(c.cpu().numpy(), want2, "job C, key 2 on s2")


def test_three_streams_one_slot_packed(torch, sources):
    three_streams_one_slot(torch, sources[0], rect(30.0), rect(-75.0))


def test_three_streams_one_slot_staged(torch, sources, staged):
    three_streams_one_slot(torch, sources[0], cube(96), cube(80))


def test_ray_taps_under_a_render(torch, sources):
    """render_rays with tap table T1 on s1, a plain render on s2, render_rays with T2 on the library's stream: the
    second table is uploaded while the first call may still read the first"""
    src = sources[0]
    a = rect(30.0, twine=3)
    nine = np.concatenate([ea.render(a, src, 3, stage=k) for k in (1, 3, 4)], axis=2)
    t1, t2 = ea.make_spread(3, 3), ea.make_spread(7, 7, 1.0, 1.5, 0.02)
    want = [ea.render_rays(src, nine, taps=t) for t in (t1, t2)]
    assert (want[0].view(np.uint32) != want[1].view(np.uint32)).any()
    want_mid = ea.render(cube(96), src, 3)
    nine_t = torch.from_numpy(nine).to("cuda:0")
    outs = [torch.zeros(want[0].shape, device="cuda:0", dtype=torch.float32) for _ in range(2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ea.render_rays(src, nine_t, taps=t1, out=outs[0], stream=s1.cuda_stream)
    mid = render_dev(torch, cube(96), src, s2)
    ea.render_rays(src, nine_t, taps=t2, out=outs[1])
    settle(torch)
    assert_bits(outs[0].cpu().numpy(), want[0], "rays with T1 on s1")
    assert_bits(outs[1].cpu().numpy(), want[1], "rays with T2 on the library's stream")
    assert_bits(mid.cpu().numpy(), want_mid, "the render between them")


def test_tethered_frame_buffer_on_two_streams(torch, sources):
    """two EU_OUT_SRGBA8 jobs of one geometry - one plan key, one float frame buffer - from different sources,
    alternating on two streams: a frame buffer rewritten under the other job's post-pass would show"""
    a = rect(30.0, tethered=True)
    want = [ea.render(a, s, 3) for s in sources]
    assert (want[0] != want[1]).any()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = [render_dev(torch, a, sources[k & 1], streams[k & 1]) for k in range(6)]
    settle(torch)
    for k, o in enumerate(outs):
        got = o.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want[k & 1]), f"call {k}: {int((got != want[k & 1]).sum())} words differ"


def test_alpha_plan_on_two_streams(torch):
    """eu_hip_facet_alpha_dev with one edit on s1, then with another on s2: the second row plan is uploaded while the
    first edit may still read the first"""
    w, h = 200, 120
    edits = [([(np.array([20, 150, 90], np.float32), np.array([10, 30, 100], np.float32))], (10, 180, 5, 110), 1),
             ([(np.array([60, 190, 120, 30], np.float32), np.array([15, 60, 110, 70], np.float32))], (0, 200, 20, 100), 2)]
    want = [ea.facet_alpha_dev(None, p, c, k, shape=(h, w), nchannels=4) for p, c, k in edits]
    assert (want[0] != want[1]).any()
    planes = [torch.zeros((h, w), device="cuda:0", dtype=torch.float32) for _ in edits]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    hold = []
    for (p, c, k), plane, s in zip(edits, planes, streams):
        e, keep = api._facet_edit(p, c, k, 4, True)
        hold.append((e, keep))
        rc = ea.lib().eu_hip_facet_alpha_dev(None, w, h, 4, C.byref(e), C.c_void_p(plane.data_ptr()),
                                            C.c_void_p(s.cuda_stream))
        assert rc == 0, ea.lib().eu_hip_last_error()
    settle(torch)
    for k in (0, 1):
        assert_bits(planes[k].cpu().numpy(), want[k], f"alpha plane of edit {k}")


def test_a_stream_the_caller_has_destroyed(torch, sources):
    """A caller's stream that is idle and destroyed once its job is done: the next job that rewrites the tables, and
    eu_hip_sync(), return 0 - the library waits on events of its own and keeps no handle of the stream."""
    src = sources[0]
    key1, key2 = rect(15.0), rect(120.0)
    want1, want2 = ea.render(key1, src, 3), ea.render(key2, src, 3)
    hip = ea.lib()                     # dlsym through the library reaches the HIP runtime it is bound to
    for f, at in ((hip.hipStreamCreate, [C.POINTER(C.c_void_p)]), (hip.hipStreamSynchronize, [C.c_void_p]),
                  (hip.hipStreamDestroy, [C.c_void_p])):
        f.restype, f.argtypes = C.c_int, at

    class raw_stream:
        def __init__(self, handle):
            self.cuda_stream = handle

    h = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(h)) == 0
    torch.cuda.synchronize()
    a = render_dev(torch, key1, src, raw_stream(h.value))
    assert hip.hipStreamSynchronize(h) == 0
    assert hip.hipStreamDestroy(h) == 0
    b = render_dev(torch, key2, src, None)
    settle(torch)
    assert_bits(a.cpu().numpy(), want1, "the job on the stream that is gone")
    assert_bits(b.cpu().numpy(), want2, "the job with a new key behind it")
