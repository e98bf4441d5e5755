"""Feathered seams (--synopsis feather, EU_SYN_FEATHER): the definition restated in numpy float32, operation by
operation, and the helpers that get its inputs from what the suite already holds bit for bit. The reference has no
blending and the oracle knows no feather: this model is the yardstick of tests/test_feather_model.py (its own
properties, no GPU) and tests/test_gpu_feather.py (the device against it, bit for bit). TEST CODE.

The definition, per output pixel (per tap ray of a twined job), float32, one operation at a time, facets in job order:
    a facet the ray misses contributes nothing (also a facet of another channel count)
    v  = the facet's pixel at the target's channel count (brighten, --mask_for paint, channel adaption included)
    dx = min(sx + 0.5, (window_width - 0.5) - sx), dy likewise; d = the smaller over the axes that have a border
    e  = clamp(d * float(1.0 / width_px), 2^-16, 1); 1 where no axis has a border
    no alpha:  q = e,       acc += v * q
    alpha a:   q = a * e,   acc += (a > 1e-6 ? v / a : 0) * q,   amax = max(amax, a)
    qsum += q
    one facet: v as it is.  Otherwise acc / qsum (0 unless qsum > 0), with alpha times amax and alpha = amax.
    no facet: zeros.
"""
import copy
import math

import numpy as np

import envutil_amd as ea
import euo
import jobs

F = np.float32
FLOOR = F(2.0 ** -16)
ALPHA_GATE = F(0.000001)
# target projections whose stepper gives the same ray with and without normalisation (eu_setup_math.h: stepper_form
# has EU_NORM_NONE for them). A multi-facet job always normalises, a single-facet job without twining never does: only
# for these targets does a single-facet job see the very rays the multi-facet job sees.
SAME_RAYS = (ea.SPHERICAL, ea.FISHEYE, ea.STEREOGRAPHIC)


def f32(x):
    return np.asarray(x, np.float32)


def borders(prj, hfov_deg, width, height):
    """(axis 0 has a border, axis 1 has one) for a source: none where the facet wraps or closes there"""
    hf = math.radians(hfov_deg)
    if prj in (euo.CUBEMAP, euo.BIATAN6) or (prj == euo.FISHEYE and hf >= 2.0 * math.pi):
        return False, False
    full = abs(hf - 2.0 * math.pi) < 1e-6
    periodic = prj in (euo.SPHERICAL, euo.CYLINDRICAL) and full
    sphere = prj == euo.SPHERICAL and full and width == 2 * height
    return not periodic, not sphere


def edge_weight(sx, sy, win, border, width_px=0.0):
    """step 4 of the definition for arrays of source coordinates; win = (window_width, window_height)"""
    sx, sy = f32(sx), f32(sy)
    if not (border[0] or border[1]):
        return np.ones(sx.shape, np.float32)
    wpx = float(width_px) if width_px > 0 else 0.5 * min(win[0], win[1])
    rcp = F(1.0 / wpx)                                   # the division in double, narrowed once
    lim_x, lim_y = F(F(win[0]) - F(0.5)), F(F(win[1]) - F(0.5))
    dx = np.minimum(f32(sx + F(0.5)), f32(lim_x - sx))
    dy = np.minimum(f32(sy + F(0.5)), f32(lim_y - sy))
    d = np.minimum(dx, dy) if border[0] and border[1] else dx if border[0] else dy
    e = f32(d * rcp)
    e = np.where(e < FLOOR, FLOOR, e)
    e = np.where(e > F(1.0), F(1.0), e)
    return f32(e)


def feather(facets, nch, width_px=0.0, details=False):
    """The frame from per-facet arrays. facets: a list of dicts with
        pixel (H, W, nch)   the facet's pixel at the target's channel count
        hit   (H, W) bool   the ray hits the facet
        sx, sy (H, W)       the source coordinate
        win   (w, h)        the facet's window size
        border (b0, b1)     the axes that have a border
    details: also return (qsum, count)."""
    shape = facets[0]["hit"].shape
    alpha = nch in (2, 4)
    ncol = nch - 1 if alpha else nch
    acc = np.zeros(shape + (ncol,), np.float32)
    qsum = np.zeros(shape, np.float32)
    amax = np.zeros(shape, np.float32)
    count = np.zeros(shape, np.int32)
    one = np.zeros(shape + (nch,), np.float32)
    with np.errstate(all="ignore"):
        for fc in facets:
            hit = np.asarray(fc["hit"], bool)
            v = f32(fc["pixel"])
            e = edge_weight(fc["sx"], fc["sy"], fc["win"], fc["border"], width_px)
            if alpha:
                a = v[:, :, nch - 1]
                q = f32(a * e)
                for c in range(ncol):
                    dc = np.where(a > ALPHA_GATE, f32(v[:, :, c] / a), F(0))
                    acc[:, :, c] = np.where(hit, f32(acc[:, :, c] + f32(dc * q)), acc[:, :, c])
                amax = np.where(hit, np.maximum(amax, a), amax)
            else:
                q = e
                for c in range(ncol):
                    acc[:, :, c] = np.where(hit, f32(acc[:, :, c] + f32(v[:, :, c] * q)), acc[:, :, c])
            qsum = np.where(hit, f32(qsum + q), qsum)
            first = hit & (count == 0)
            one[first] = v[first]
            count = count + hit
        out = np.zeros(shape + (nch,), np.float32)
        for c in range(ncol):
            t = f32(acc[:, :, c] / qsum)
            t = np.where(qsum > 0, t, F(0))
            if alpha:
                t = f32(t * amax)
            out[:, :, c] = t
        if alpha:
            out[:, :, nch - 1] = amax
    single = count == 1
    out[single] = one[single]
    out[count == 0] = 0
    return (out, qsum, count) if details else out


class Facet:
    """One facet of a feathered job, for the oracle and for the model: the OracleSource, its twin painted white - one
    channel, brighten 1: the facet's geometry alone, so its single-facet frame is 1 where the ray hits and 0 where
    not, whatever the facet's own pixels and alpha hold -, the window size and the border flags. gpu() adopts the
    oracle's container on the device."""

    def __init__(self, prj, width, height, hfov, pixels, degree, **kw):
        self.prj, self.width, self.height, self.hfov, self.degree, self.kw = prj, width, height, hfov, degree, dict(kw)
        self.o = jobs.OracleSource(prj, width, height, hfov, pixels, degree, **kw)
        pixels = np.asarray(pixels)
        kh = dict(kw, brighten=1.0, masked=1)
        self.white = jobs.OracleSource(prj, width, height, hfov, np.zeros(pixels.shape[:2] + (1,), np.float32), degree, **kh)
        win = kw.get("window")
        cube = prj in (euo.CUBEMAP, euo.BIATAN6)
        self.win = (win[0], win[1]) if win else (width, 6 * width if cube else height)
        self.border = borders(prj, hfov, width, height)
        self.nch = self.o.nch

    def _spec_kw(self):
        return {k: v for k, v in self.kw.items() if k not in ("prefilter_degree", "support_min", "tile")}

    def gpu(self):
        spec = ea.facet_spec(self.prj, self.width, self.height, self.hfov, nchannels=self.nch, **self._spec_kw())
        return ea.Source.adopt(spec, self.o.container, self.degree, self.o.bc[0], self.o.bc[1])

    def gpu_white(self):
        """the white twin on the device, for the route through caller-supplied rays"""
        kw = dict(self._spec_kw(), brighten=1.0, masked=1)
        spec = ea.facet_spec(self.prj, self.width, self.height, self.hfov, nchannels=1, **kw)
        return ea.Source.adopt(spec, self.white.container, self.degree, self.white.bc[0], self.white.bc[1])


def single_args(args):
    """the multi-facet job's target as a single-facet job sees it"""
    a = copy.copy(args)
    a.synopsis = "panorama"
    return a


def facet_arrays(args, fct, nch, **render_kw):
    """pixel, hit, sx, sy of one facet for every pixel of the job's frame, from single-facet oracle jobs with the
    multi-facet job's target: stage 0 at the target's channel count, stage 2, and stage 0 of the white twin"""
    assert args.projection in SAME_RAYS and not args.twine, "a single-facet job sees other rays than the multi-facet job"
    a = single_args(args)
    crd = jobs.oracle_render(a, fct.o, stage=2, **render_kw)
    white = jobs.oracle_render(a, fct.white, nch=1, **render_kw)[:, :, 0]
    return dict(pixel=jobs.oracle_render(a, fct.o, nch=nch, **render_kw), hit=white != 0, sx=crd[:, :, 0], sy=crd[:, :, 1],
                win=fct.win, border=fct.border)


def model_frame(args, facets, nch, details=False, **render_kw):
    """the feathered frame of the job `args` over `facets` (Facet objects), whole: no pixel is left out"""
    return feather([facet_arrays(args, f, nch, **render_kw) for f in facets], nch, args.feather, details=details)


# ---- the route through the rays -----------------------------------------------------------------------------------
# For jobs whose single-facet form sees other rays than the multi-facet job - a target whose stepper normalises
# (rectilinear, cylindrical, the cubes), a translated facet or a --single target (generic stepper), any twined job -
# the facets' arrays are taken at the multi-facet job's OWN rays: a single-facet TWINED job steps with normalisation,
# as every multi-facet job does, and its stages 1, 3 and 4 are the three steppers' rays. The pixel and the hit (the
# white twin) then come from eu_hip_render_rays, which is held to the oracle elsewhere, and the coordinates from the
# oracle's euo_source_coordinates. Needs a device.

def stepper_rays(args, fct):
    """r00, r10, r01 of the facet as the multi-facet job's steppers give them, (H, W, 3) each"""
    a = single_args(args)
    if a.twine_spread is None:
        a.twine_spread = ea.make_spread(2, 2, 1.0, 0.0, 0.0)          # any tap table: it makes the job a twined one
    return [jobs.oracle_render(a, fct.o, stage=s) for s in (1, 3, 4)]


def tap_rays(r00, r10, r01, tap):
    """eu_syn_ray: (r00 + cx * du) + cy * dv with the tap's x and y times the bias 4"""
    cx, cy = F(F(tap[0]) * F(4.0)), F(F(tap[1]) * F(4.0))
    du, dv = f32(r10 - r00), f32(r01 - r00)
    return f32(f32(r00 + f32(cx * du)) + f32(cy * dv))


def arrays_at_rays(rays, fct, g, gw, nch):
    crd = euo.source_coordinates(fct.o.s, rays.reshape(-1, 3)).reshape(rays.shape)
    hit = ea.render_rays(gw, np.ascontiguousarray(rays), nchannels=1)[..., 0] != 0
    assert (hit == (crd[..., 2] != -1)).all(), "the white twin and the oracle's mask disagree"
    return dict(pixel=ea.render_rays(g, np.ascontiguousarray(rays), nchannels=nch), hit=hit, sx=crd[..., 0], sy=crd[..., 1],
                win=fct.win, border=fct.border)


def model_frame_at_rays(args, facets, gs, gws, nch):
    """the feathered frame through the rays; a twined job: the model per tap, then the kernel's weighted sum"""
    rays = [stepper_rays(args, f) for f in facets]
    if args.twine_spread is None:
        return feather([arrays_at_rays(r[0], f, g, gw, nch) for r, f, g, gw in zip(rays, facets, gs, gws)], nch, args.feather)
    out = np.zeros(rays[0][0].shape[:2] + (nch,), np.float32)
    for tap in np.asarray(args.twine_spread, np.float32):
        help_ = feather([arrays_at_rays(tap_rays(*r, tap), f, g, gw, nch) for r, f, g, gw in zip(rays, facets, gs, gws)],
                        nch, args.feather)
        out = f32(out + f32(F(tap[2]) * help_))
    return out
