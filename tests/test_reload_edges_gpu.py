"""eu_hip_source_reload of a source that keeps a distance plane (EU_LOAD_EDGES): the plane is refilled in the same
stream order as the container, at the same device address; a render queued behind the reload sees the new plane; an
unflagged source stays one. The plane itself is held to the model in tests/test_gpu_edges.py."""
import numpy as np
import pytest

import envutil_amd as ea
import jobs
from test_gpu_edges import W, H, MASKS, CROP

pytestmark = pytest.mark.gpu


def test_reload_refills_the_plane_in_stream_order():
    import torch
    rng = np.random.default_rng(2)
    fct = ea.facet_spec(ea.RECTILINEAR, W, H, 70.0, nchannels=4)
    rgb = [rng.random((H, W, 3), dtype=np.float32) for _ in range(2)]
    first = dict(masks=MASKS, crop=CROP, crop_kind=2)
    second = dict(masks=[(np.array([40.0, 55.0, 50.0, 35.0]), np.array([5.0, 9.0, 35.0, 30.0]))], crop=(0, 50, 6, 43), crop_kind=1)
    src = ea.Source.load(fct, rgb[0], 1, edges=True, **first)
    other = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, W, H, 70.0, nchannels=4, yaw=25.0), rgb[1], 1)
    a = ea.arguments(ea.SPHERICAL, 96, 48, 120.0, spline_degree=1, synopsis="feather", feather=8.0)
    before = ea.render(a, [src, other], 4)
    where = (src.device_ptr(), src.edge_device_ptr())
    assert where[1]
    st = torch.cuda.Stream()
    src.reload(rgb[1], stream=st, **second)
    # a render queued behind the reload, on another stream: it sees the new plane
    after = ea.render(a, [src, other], 4)
    fresh = ea.Source.load(fct, rgb[1], 1, edges=True, **second)
    assert (src.device_ptr(), src.edge_device_ptr()) == where
    assert (jobs.bits(src.edge_distance()) == jobs.bits(fresh.edge_distance())).all()
    assert (jobs.bits(src.download()) == jobs.bits(fresh.download())).all()
    assert (jobs.bits(after) == jobs.bits(ea.render(a, [fresh, other], 4))).all()
    assert (jobs.bits(after) != jobs.bits(before)).any()
    # once more: the scratch has grown, and the plane follows again
    src.reload(rgb[0], stream=st, **first)
    again = ea.Source.load(fct, rgb[0], 1, edges=True, **first)
    assert (jobs.bits(src.edge_distance()) == jobs.bits(again.edge_distance())).all()
    assert (src.device_ptr(), src.edge_device_ptr()) == where
    # an unflagged source stays one
    other.reload(rgb[0], **first)
    assert not other.has_edges and other.edge_device_ptr() is None
    ea.sync()
    ea.reload_scratch_release()
