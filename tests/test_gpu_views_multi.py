"""Many views of a multi-facet job in one call: ea.render_views with a list of sources (eu_hip_render_views_multi)
against ea.render of every view on the same list of sources - the library's existing multi-facet path, itself pinned
to the CPU oracle (test_gpu_parity, test_hdr_merge, test_mask_for). Float32 bit patterns, 0 ULP, every pixel of every
view. Three views per call, one of them with another hfov; the views of a call must differ from one another and a
useful share of every reference frame must be non-zero, so that equal frames mean something."""
import copy

import numpy as np
import pytest

import envutil_amd as ea
import euo
import jobs
from test_gpu_parity import assert_bits, facet_set
from test_hdr_merge import bracket

pytestmark = pytest.mark.gpu

LENS = dict(a=0.01, b=-0.03, c=0.02)
# width 130: a tile tail whose dead lanes take part in the ballots, and 65 rows: a partial tile row
T_SPH = (ea.SPHERICAL, 130, 65, 360.0)
# width 65: one live lane in the second tile; 77 rows
T_RECT = (ea.RECTILINEAR, 65, 77, 100.0)
# the second segment of 512 columns, where a lane's planar x starts again
T_513 = (ea.SPHERICAL, 513, 10, 360.0)
# rows that depend on the face
T_CUBE = (ea.CUBEMAP, 40, 240, 90.0)
T_BIATAN = (ea.BIATAN6, 24, 144, 90.0)


def views_of(hfov):
    """two orientations, and one with another hfov"""
    return [(0.0, 0.0, 0.0), (30.0, 15.0, 7.5), (-40.0, 20.0, -5.0, hfov * 0.75)]


_sets = {}


def fish(nch, degree):
    """six 64 x 64 fisheye facets of 140 degrees with the lens polynomial, looking front / right / back / left / up /
    down: they cover the sphere"""
    key = ("fish", nch, degree)
    if key not in _sets:
        _sets[key] = facet_set(euo.FISHEYE, 64, 64, 140.0, nch, degree, LENS)[1]
    return _sets[key]


def rect24(nch):
    """24 rectilinear 48 x 48 facets of 70 - 85 degrees (test_multi_facet_more_than_sixteen); the narrow ones leave
    holes between them on purpose: a hole is the synopsis' `no facet` result"""
    key = ("rect24", nch)
    if key not in _sets:
        gs = []
        for k in range(4):
            gs += facet_set(euo.RECTILINEAR, 48, 48, 70.0 + 5 * k, nch, 1, seed=40 + k)[1]
        _sets[key] = gs
    return _sets[key]


def reference(gs, target, view, nch, **kw):
    tprj, tw, th, thfov = target
    hfov = view[3] if len(view) == 4 else thfov
    a = ea.arguments(tprj, tw, th, hfov, yaw=view[0], pitch=view[1], roll=view[2], **kw)
    return ea.render(a, list(gs), nch)


def check_views(gs, target, what, nch=None, views=None, share=0.5, **kw):
    """render_views against render of every view; returns (frames, references)"""
    tprj, tw, th, thfov = target
    views = views_of(thfov) if views is None else views
    n = nch or gs[0].fct.nchannels
    a = ea.arguments(tprj, tw, th, thfov, **kw)
    got = ea.render_views(a, views, gs, nchannels=nch)
    assert got.shape == (len(views), th, tw, n)
    refs = []
    for k, v in enumerate(views):
        ref = reference(gs, target, v, n, **kw)
        assert_bits(got[k], ref, f"{what}: target {target}, view {k} {v}")
        lit = float((ref != 0).any(axis=-1).mean())
        assert lit >= share, f"{what}: view {k} shows the facets in {lit:.2f} of its pixels only"
        refs.append(ref)
    assert all((jobs.bits(got[k]) != jobs.bits(got[0])).any() for k in range(1, len(views))), what + ": views alike"
    return got, refs


# ---- facet counts -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("nfct", [2, 6])
def test_two_and_six_facets(nfct, nch):
    """six facets: the coordinates of every facet stay in LDS (nfct <= 16). Two facets (front and right) leave most
    of the sphere empty on purpose: the views look at them, a third of a frame is what they fill at least"""
    gs = fish(nch, 1)[:nfct]
    for target in (T_SPH, T_RECT):
        check_views(gs, target, f"{nfct} facets, {nch} channels", share=0.9 if nfct == 6 else 0.3, spline_degree=1)


@pytest.mark.parametrize("nch", [3, 4])
def test_seventeen_facets(nch):
    """beyond EU_MULTI_KEEP the winners' coordinates are recomputed instead of kept"""
    check_views(rect24(nch)[:17], T_SPH, f"17 facets, {nch} channels", spline_degree=1)
    check_views(rect24(nch), (ea.RECTILINEAR, 100, 50, 90.0), f"24 facets, {nch} channels", spline_degree=1)


@pytest.mark.parametrize("nch", [3, 4])
def test_seventy_two_facets(nch):
    """more facets than mask bits: eu_synopsis_big with alpha, the mask-free voronoi_syn without. Every facet three
    times over: equal z scores, the earlier one on top"""
    check_views(rect24(nch) * 3, (ea.SPHERICAL, 96, 48, 360.0), f"72 facets, {nch} channels", spline_degree=1)


def test_seventy_two_facets_twined():
    """eu_synopsis_big under the twine loop: 72 RGBA facets of 16 x 16 (four sets of six, every facet three times
    over), a 65 x 5 target - one live lane in the second tile - twine 2, two views"""
    gs = []
    for k in range(4):
        gs += facet_set(euo.RECTILINEAR, 16, 16, 70.0 + 5 * k, 4, 1, seed=40 + k)[1]
    check_views(gs * 3, (ea.SPHERICAL, 65, 5, 360.0), "72 facets twined", views=views_of(360.0)[:2], spline_degree=1,
                twine=2)


# ---- targets ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch", [3, 4])
def test_second_segment_and_face_dependent_rows(nch):
    gs = fish(nch, 1)
    for target in (T_513, T_CUBE, T_BIATAN):
        check_views(gs, target, f"{nch} channels", share=0.9, spline_degree=1)


@pytest.mark.parametrize("target", [(ea.CYLINDRICAL, 150, 70, 220.0), (ea.FISHEYE, 120, 90, 200.0),
                                    (ea.STEREOGRAPHIC, 110, 84, 240.0)])
def test_other_target_projections(target):
    """a multi-facet job always normalises: the cylindrical target's rays are normalised also without twining"""
    check_views(fish(4, 1), target, "six facets", share=0.9, spline_degree=1)
    check_views(fish(3, 1), target, "six facets twined", share=0.9, spline_degree=1, twine=2)


# ---- channels, degrees ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch", [1, 2, 3, 4])
def test_channel_counts(nch):
    """voronoi_syn for 1 and 3 channels, voronoi_syn_plus for 2 and 4"""
    check_views(fish(nch, 1), T_SPH, f"{nch} channels", share=0.9, spline_degree=1)


@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("degree", [0, 1, 3, 5])
def test_spline_degrees(degree, nch):
    """the instantiations for degrees 0 - 3 and the one with the run-time degree"""
    check_views(fish(nch, degree), T_RECT, f"degree {degree}, {nch} channels", share=0.9, spline_degree=degree)


@pytest.mark.parametrize("mix,out_n", [((3, 4), 4), ((4, 2), 2)])
@pytest.mark.parametrize("twine", [0, 2])
def test_mixed_channel_counts(mix, out_n, twine):
    """facets with different channel counts in one job (test_multi_facet_mixed_channel_counts): each adapts through
    repix_t. Where three feathered alpha facets meet at a corner of the cube all of them are transparent: holes"""
    sets = {n: facet_set(euo.RECTILINEAR, 72, 72, 95.0, n, 1, seed=21)[1] for n in set(mix)}
    gs = [sets[mix[i % len(mix)]][i] for i in range(6)]
    check_views(gs, (ea.SPHERICAL, 150, 75, 360.0), f"mixed channels {mix}->{out_n}", nch=out_n, share=0.7,
                spline_degree=1, twine=twine)


@pytest.mark.parametrize("nch", [3, 4])
def test_mask_for_set(nch):
    """--mask_for facet 1: it is painted white, the others black"""
    gs = facet_set(euo.FISHEYE, 64, 64, 140.0, nch, 1, LENS)[1]
    for i, s in enumerate(gs):
        f = copy.copy(s.fct)
        f.masked = int(i == 1)
        s.update_facet(f)
    # black facets are zero pixels: the white one is what the frames show, and only where it wins
    got, _ = check_views(gs, T_SPH, f"--mask_for, {nch} channels", share=0.02, spline_degree=1)
    assert all((got[k][..., 0] == 0.0).any() and (got[k][..., 0] != 0.0).any() for k in range(3)), "black and white"


# ---- twining, hdr_merge -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nch", [3, 4])
def test_twining_on_both_coordinate_paths(nch):
    """four facets (front, right, back, left: the poles stay empty on purpose) and seventeen"""
    check_views(fish(nch, 1)[:4], T_SPH, f"4 facets twined, {nch} channels", share=0.6, spline_degree=1, twine=2)
    check_views(rect24(nch)[:17], (ea.SPHERICAL, 96, 48, 360.0), f"17 facets twined, {nch} channels", spline_degree=1,
                twine=2)


@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("twine", [0, 2])
def test_hdr_merge_bracket(nch, twine):
    """three exposures of one scene with brighten 4 / 1 / 0.25, with and without alpha (holes in it); the views stay
    near the bracket's axis, what lies beside the facets is empty"""
    gs = bracket(euo.RECTILINEAR, 96, 64, 75.0, nch, 1, (4.0, 1.0, 0.25), with_gpu=True, alpha_holes=True)[1]
    views = [(0.0, 0.0, 0.0), (10.0, 5.0, 3.0), (-8.0, 4.0, -5.0, 45.0)]
    check_views(gs, (ea.RECTILINEAR, 100, 61, 60.0), f"hdr_merge, {nch} channels, twine {twine}", views=views,
                share=0.4, spline_degree=1, twine=twine, synopsis="hdr_merge")


# ---- chunks -----------------------------------------------------------------------------------------------------

CHUNK_VIEWS = [(12.0 * k, 5.0 * k - 10.0, 3.0 * k, 100.0 - 4 * k) for k in range(5)]


@pytest.mark.parametrize("on_device", [False, True])
def test_chunks_give_the_same_bits(on_device, monkeypatch):
    """five views of six facets: one view per chunk (a bound of 1 KiB, below one view's tables), chunks of 2, 2, 1
    (a bound that holds exactly two views), and all at once"""
    gs = fish(4, 1)
    tprj, tw, th, thfov = T_RECT
    a = ea.arguments(tprj, tw, th, thfov, spline_degree=1)
    per = 6 * (6 * tw + 24 * th) * 4
    two = -(-2 * per // 1024)
    assert 2 * per <= two * 1024 < 3 * per

    def run():
        if not on_device:
            return ea.render_views(a, CHUNK_VIEWS, gs)
        import torch
        out_t = torch.zeros((5, th, tw, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ea.render_views(a, CHUNK_VIEWS, gs, out=out_t)
        ea.sync()
        return out_t.cpu().numpy()

    whole = run()
    monkeypatch.setenv("EU_HIP_VIEWS_MAX_KB", "1")
    assert_bits(run(), whole, "one view per chunk against all at once")
    monkeypatch.setenv("EU_HIP_VIEWS_MAX_KB", str(two))
    assert_bits(run(), whole, "chunks of 2, 2, 1 against all at once")
    monkeypatch.delenv("EU_HIP_VIEWS_MAX_KB")
    for k, v in enumerate(CHUNK_VIEWS):
        assert_bits(whole[k], reference(gs, T_RECT, v, 4, spline_degree=1), f"view {k}")


# ---- output -----------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-12345.5)


def layout_job():
    gs = fish(4, 1)
    tprj, tw, th, thfov = T_RECT
    a = ea.arguments(tprj, tw, th, thfov, spline_degree=1)
    views = views_of(thfov)
    return gs, a, views, [reference(gs, T_RECT, v, 4, spline_degree=1) for v in views]


def test_fresh_and_padded_numpy_output():
    gs, a, views, refs = layout_job()
    fresh = ea.render_views(a, views, gs)
    big = np.full((3, 77 + 2, 65 + 5, 4), SENTINEL, np.float32)
    out = big[:, :77, :65]
    assert ea.render_views(a, views, gs, out=out) is out
    for k in range(3):
        assert_bits(fresh[k], refs[k], f"fresh, view {k}")
        assert_bits(np.ascontiguousarray(out[k]), refs[k], f"padded, view {k}")
    assert (big[:, 77:] == SENTINEL).all() and (big[:, :, 65:] == SENTINEL).all(), "the padding of `out` was written"
    # no view: nothing is written
    assert ea.render_views(a, [], gs).shape == (0, 77, 65, 4)


def test_padded_torch_output_on_two_streams_with_a_render_between():
    """views on stream A, a multi-facet render on the library's stream, other views on stream B: the second call must
    not rewrite the tables or the facets' parameters under the first"""
    import torch
    gs, a, views, refs = layout_job()
    others = [(12.0 * k, 5.0 * k - 10.0, 3.0 * k) for k in range(1, 4)]
    j = ea.arguments(*T_RECT, yaw=11, pitch=-7, roll=3, spline_degree=1)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    big_a = torch.full((3, 77 + 1, 65 + 3, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    big_b = torch.full((3, 77 + 1, 65 + 3, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ea.render_views(a, views, gs, out=big_a[:, :77, :65], stream=sa.cuda_stream)
    between = ea.render(j, gs, 4)
    ea.render_views(a, others, gs, out=big_b[:, :77, :65], stream=sb.cuda_stream)
    ea.sync()
    torch.cuda.synchronize()
    host_a, host_b = big_a.cpu().numpy(), big_b.cpu().numpy()
    for k in range(3):
        assert_bits(np.ascontiguousarray(host_a[k, :77, :65]), refs[k], f"stream A, view {k}")
        assert_bits(np.ascontiguousarray(host_b[k, :77, :65]), reference(gs, T_RECT, others[k], 4, spline_degree=1),
                    f"stream B, view {k}")
    for host in (host_a, host_b):
        assert (host[:, 77:] == SENTINEL).all() and (host[:, :, 65:] == SENTINEL).all(), "the padding of `out` was written"
    assert_bits(between, reference(gs, T_RECT, (11, -7, 3), 4, spline_degree=1), "the render between")


# ---- state ------------------------------------------------------------------------------------------------------

def test_render_and_its_tables_are_left_alone():
    """multi-facet job A through ea.render, render_views on other facets and another target size, A again: A has the
    same bits and the launch counter advanced by A's launches only"""
    gs_a = fish(3, 1)
    j = ea.arguments(ea.SPHERICAL, 120, 60, 360.0, yaw=11, pitch=-7, roll=3, spline_degree=1)
    n0 = ea.launch_count()
    first = ea.render(j, gs_a, 3)
    n1 = ea.launch_count()
    check_views(rect24(4)[:8], T_RECT, "other facets, another size", share=0.3, spline_degree=1)
    n2 = ea.launch_count()
    ea.render_views(ea.arguments(*T_RECT, spline_degree=1, twine=2), views_of(100.0), rect24(4)[:8])
    assert ea.launch_count() == n2, "render_views counted a launch"
    again = ea.render(j, gs_a, 3)
    assert ea.launch_count() - n2 == n1 - n0
    assert_bits(again, first, "job A after render_views calls")


def test_update_facet_between_two_calls():
    """the facets' parameters go up with every call: a facet turned and brightened between two calls changes the
    frames the way it changes render's"""
    gs = facet_set(euo.FISHEYE, 64, 64, 140.0, 4, 1, LENS)[1]
    before, _ = check_views(gs, T_SPH, "before update_facet", share=0.9, spline_degree=1)
    f = copy.copy(gs[0].fct)
    f.yaw, f.pitch, f.brighten = f.yaw + 20.0, f.pitch - 10.0, 1.7
    gs[0].update_facet(f)
    after, _ = check_views(gs, T_SPH, "after update_facet", share=0.9, spline_degree=1)
    assert all((jobs.bits(after[k]) != jobs.bits(before[k])).any() for k in range(3))


def test_a_list_of_one_is_that_source():
    g = fish(3, 1)[0]
    for target in (T_SPH, T_RECT):
        a = ea.arguments(*target, spline_degree=1)
        views = views_of(target[3])
        one = ea.render_views(a, views, g)
        assert_bits(ea.render_views(a, views, [g]), one, "a list of one")
        assert_bits(ea.render_views(a, views, (g,)), one, "a tuple of one")
        assert (one != 0).any()


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_unsupported_jobs():
    gs = list(fish(3, 1)[:2])
    img = jobs.synth_image(64, 48, 3)
    tr = ea.Source.load(ea.facet_spec(ea.RECTILINEAR, 64, 48, 70.0, translation=dict(x=0.1, z=0.05)), img, 1)
    with pytest.raises(ea.EuError, match="error -3.*translation"):
        ea.render_views(ea.arguments(ea.SPHERICAL, 64, 32, 360.0), [(0, 0, 0)], gs + [tr])
    a = ea.arguments(ea.BIATAN6, 24, 144, 90.0)
    with pytest.raises(ea.EuError, match="error -3.*1.75"):
        ea.render_views(a, [(0, 0, 0), (0, 0, 0, 135.0)], gs)
    d3 = fish(3, 3)[2]
    with pytest.raises(ea.EuError, match="error -2.*degree"):
        ea.render_views(ea.arguments(ea.SPHERICAL, 64, 32, 360.0), [(0, 0, 0)], gs + [d3])
