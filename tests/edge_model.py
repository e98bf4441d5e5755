"""Feathering to alpha edges (EU_LOAD_EDGES, --feather_edges): the definition of include/eu_hip.h restated in numpy -
the distance plane by brute force over every pair of pixels, the bilinear sample and the weight in float32, operation
by operation - and the feathered and multi-band frames with that weight in feather_model's and multiband_model's
place. The yardstick of tests/test_edge_model.py (its own properties, no GPU), tests/test_gpu_edges.py (the plane,
bit for bit) and tests/test_gpu_feather_edges.py (frames, bit for bit). TEST CODE.

    O        = { (u, v) : not (alpha(u, v) > 0) }                       (NaN, negative, both zeros: outside)
    D2(x, y) = min over O of dx^2 + (y - v)^2, dx = |x - u|, or min(|x - u|, w - |x - u|) where the rows close;
               2^31 - 1 without an outside pixel                         (an exact int32)
    D        = sqrt(float32(D2)), correctly rounded
    dm       = bilinear sample of D at (sx, sy) - 0.5; columns wrap where the rows close, else clamp; rows clamp
    d        = min(dm, the window ramp's d), dm alone without a bordered axis;  e = clamp(d * float(1 / width), 2^-16, 1)
"""
import numpy as np

import envutil_amd as ea
import euo
import feather_model as fm
import multiband_model as mm

F = np.float32
FAR = 2 ** 31 - 1


def outside(alpha):
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(alpha, np.float32) > 0)


def d2_brute(out, cyclic=False):
    """D2 by its definition: for every pixel the minimum over ALL outside pixels. out: (h, w) bool. int32 (h, w)."""
    out = np.asarray(out, bool)
    h, w = out.shape
    vo, uo = np.nonzero(out)
    d2 = np.full((h, w), FAR, np.int64)
    if not len(uo):
        return d2.astype(np.int32)
    x = np.arange(w, dtype=np.int64)
    dx = np.abs(x[:, None] - uo[None, :].astype(np.int64))               # (w, M)
    if cyclic:
        dx = np.minimum(dx, w - dx)
    dx2 = dx * dx
    for y in range(h):
        dy = (y - vo.astype(np.int64))
        d2[y] = (dx2 + (dy * dy)[None, :]).min(axis=1)
    assert d2.max() <= FAR
    return d2.astype(np.int32)


def d2_two_pass(out, cyclic=False):
    """the separable restatement: the row distance g, then the minimum of g(x, v)^2 + (y - v)^2 down each column"""
    out = np.asarray(out, bool)
    h, w = out.shape
    big = 1 << 20
    g = np.full((h, w), big, np.int64)
    x = np.arange(w, dtype=np.int64)
    for y in range(h):
        u = np.nonzero(out[y])[0].astype(np.int64)
        if len(u):
            dx = np.abs(x[:, None] - u[None, :])
            if cyclic:
                dx = np.minimum(dx, w - dx)
            g[y] = dx.min(axis=1)
    has = g < big
    d2 = np.full((h, w), FAR, np.int64)
    v = np.arange(h, dtype=np.int64)
    for y in range(h):
        cand = np.where(has, g * g + ((y - v) ** 2)[:, None], 1 << 62)
        m = cand.min(axis=0)
        d2[y] = np.where(has.any(axis=0), m, FAR)
    return d2.astype(np.int32)


def root(d2):
    """D = sqrt(float(D2)): int32 -> float32 to nearest, then IEEE's correctly rounded float32 square root"""
    return np.sqrt(np.asarray(d2, np.int32).astype(np.float32)).astype(np.float32)


def distance_plane(alpha, cyclic=False):
    return root(d2_brute(outside(alpha), cyclic))


def sample(D, sx, sy, cyclic):
    """dm at arrays of source coordinates, float32, one operation at a time"""
    D = np.asarray(D, np.float32)
    h, w = D.shape
    sx, sy = fm.f32(sx), fm.f32(sy)
    with np.errstate(all="ignore"):
        flx, fly = np.floor(sx), np.floor(sy)
        fx, fy = fm.f32(sx - flx), fm.f32(sy - fly)
        ok = np.isfinite(flx) & np.isfinite(fly)
        ix, iy = np.where(ok, flx, 0).astype(np.int64), np.where(ok, fly, 0).astype(np.int64)
        if cyclic:
            x0, x1 = np.mod(ix, w), np.mod(ix + 1, w)
        else:
            x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
        y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
        d00, d10, d01, d11 = D[y0, x0], D[y0, x1], D[y1, x0], D[y1, x1]
        top = fm.f32(d00 + fm.f32(fm.f32(d10 - d00) * fx))
        bot = fm.f32(d01 + fm.f32(fm.f32(d11 - d01) * fx))
        return fm.f32(fm.f32(top + fm.f32(fm.f32(bot - top) * fy)) - F(0.5))


def edge_weight(fc, width_px=0.0):
    """e of one facet's arrays (feather_model.feather documents them); fc["dist"]: its plane or None, fc["cyclic"]"""
    D = fc.get("dist")
    if D is None:
        return fm.edge_weight(fc["sx"], fc["sy"], fc["win"], fc["border"], width_px)
    sx, sy, win, border = fm.f32(fc["sx"]), fm.f32(fc["sy"]), fc["win"], fc["border"]
    wpx = float(width_px) if width_px > 0 else 0.5 * min(win[0], win[1])
    rcp = F(1.0 / wpx)
    d = sample(D, sx, sy, fc["cyclic"])
    if border[0] or border[1]:
        lim_x, lim_y = F(F(win[0]) - F(0.5)), F(F(win[1]) - F(0.5))
        dx = np.minimum(fm.f32(sx + F(0.5)), fm.f32(lim_x - sx))
        dy = np.minimum(fm.f32(sy + F(0.5)), fm.f32(lim_y - sy))
        dw = np.minimum(dx, dy) if border[0] and border[1] else dx if border[0] else dy
        d = np.minimum(d, dw)
    with np.errstate(all="ignore"):
        e = fm.f32(d * rcp)
    e = np.where(e < fm.FLOOR, fm.FLOOR, e)
    e = np.where(e > F(1.0), F(1.0), e)
    return fm.f32(e)


def feather(facets, nch, width_px=0.0, details=False):
    """feather_model.feather with edge_weight above in its e's place: everything behind e is unchanged"""
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
            v = fm.f32(fc["pixel"])
            e = edge_weight(fc, width_px)
            if alpha:
                a = v[:, :, nch - 1]
                q = fm.f32(a * e)
                for c in range(ncol):
                    dc = np.where(a > fm.ALPHA_GATE, fm.f32(v[:, :, c] / a), F(0))
                    acc[:, :, c] = np.where(hit, fm.f32(acc[:, :, c] + fm.f32(dc * q)), acc[:, :, c])
                amax = np.where(hit, np.maximum(amax, a), amax)
            else:
                q = e
                for c in range(ncol):
                    acc[:, :, c] = np.where(hit, fm.f32(acc[:, :, c] + fm.f32(v[:, :, c] * q)), acc[:, :, c])
            qsum = np.where(hit, fm.f32(qsum + q), qsum)
            first = hit & (count == 0)
            one[first] = v[first]
            count = count + hit
        out = np.zeros(shape + (nch,), np.float32)
        for c in range(ncol):
            t = fm.f32(acc[:, :, c] / qsum)
            t = np.where(qsum > 0, t, F(0))
            if alpha:
                t = fm.f32(t * amax)
            out[:, :, c] = t
        if alpha:
            out[:, :, nch - 1] = amax
    single = count == 1
    out[single] = one[single]
    out[count == 0] = 0
    return (out, qsum, count) if details else out


def stage_a(facets, nch, width_px=0.0):
    """multiband_model.stage_a fed the new q"""
    shape = facets[0]["hit"].shape
    alpha = nch in (2, 4)
    ncol = nch - 1 if alpha else nch
    X = np.zeros((len(facets),) + shape + (ncol,), np.float32)
    Q = np.zeros((len(facets),) + shape, np.float32)
    amax = np.zeros(shape, np.float32)
    count = np.zeros(shape, np.int32)
    with np.errstate(all="ignore"):
        for f, fc in enumerate(facets):
            hit = np.asarray(fc["hit"], bool)
            v = fm.f32(fc["pixel"])
            e = edge_weight(fc, width_px)
            if alpha:
                a = v[:, :, nch - 1]
                q = fm.f32(a * e)
                c = np.where((a > fm.ALPHA_GATE)[:, :, None], fm.f32(v[:, :, :ncol] / a[:, :, None]), F(0))
                amax = np.where(hit, np.maximum(amax, a), amax)
            else:
                q, c = e, v
            Q[f] = np.where(hit, q, F(0))
            X[f] = np.where((Q[f] > 0)[:, :, None], c, F(0))
            count = count + hit
    return X, Q, amax, count


def multiband(facets, nch, width_px=0.0, bands=0, wrap=False):
    X, Q, amax, count = stage_a(facets, nch, width_px)
    O = mm.blend(X, Q, bands, wrap, np.float32)
    out = np.zeros(count.shape + (nch,), np.float32)
    ncol = O.shape[2]
    if nch in (2, 4):
        out[:, :, :ncol] = O * amax[:, :, None]
        out[:, :, ncol] = amax
    else:
        out[:] = O
    out[count == 0] = 0
    return out


class Facet(fm.Facet):
    """A facet of 2 or 4 channels with PTO masks and a lens crop. `pixels` are the pixels as a file holds them; the
    oracle gets them through the host edit (eu_hip_facet_alpha, held to the device edit elsewhere), the device loads
    them with the edit - and, edges=True, with EU_LOAD_EDGES. alpha: the plane the prefilter reads; dist: its model D."""

    def __init__(self, prj, width, height, hfov, pixels, degree, masks=(), crop=None, crop_kind=0, edges=True, **kw):
        self.raw = np.ascontiguousarray(pixels, np.float32)
        self.masks, self.crop, self.crop_kind, self.edges = masks, crop, crop_kind, edges
        edited = self.raw.copy()
        if len(masks) or crop is not None:
            ea.facet_alpha(edited, masks, crop, crop_kind)
        self.alpha = edited[:, :, -1].copy()
        super().__init__(prj, width, height, hfov, edited, degree, **kw)
        self.cyclic = self.o.bc[0] == euo.PERIODIC
        self.dist = distance_plane(self.alpha, self.cyclic) if edges else None

    def gpu(self, edges=None):
        spec = ea.facet_spec(self.prj, self.width, self.height, self.hfov, nchannels=self.nch, **self._spec_kw())
        return ea.Source.load(spec, self.raw, self.degree, masks=self.masks, crop=self.crop, crop_kind=self.crop_kind,
                              edges=self.edges if edges is None else edges)


def with_plane(arrays, fct):
    return dict(arrays, dist=getattr(fct, "dist", None), cyclic=getattr(fct, "cyclic", False))


def facet_arrays(args, fct, nch, **render_kw):
    return with_plane(fm.facet_arrays(args, fct, nch, **render_kw), fct)


def model_frame(args, facets, nch, details=False, **render_kw):
    """the feathered frame of the job, through the single-facet stages (feather_model.model_frame)"""
    return feather([facet_arrays(args, f, nch, **render_kw) for f in facets], nch, args.feather, details=details)


def model_multiband(args, facets, nch, **render_kw):
    return multiband([facet_arrays(args, f, nch, **render_kw) for f in facets], nch, args.feather, args.bands, mm.wraps(args))


def model_frame_at_rays(args, facets, gs, gws, nch):
    """feather_model.model_frame_at_rays with the planes: generic stepper, rectilinear targets, twining. Needs a device."""
    rays = [fm.stepper_rays(args, f) for f in facets]

    def arrays(r, tap=None):
        rr = r[0] if tap is None else fm.tap_rays(*r, tap)
        return rr

    if args.twine_spread is None:
        return feather([with_plane(fm.arrays_at_rays(arrays(r), f, g, gw, nch), f) for r, f, g, gw in zip(rays, facets, gs, gws)],
                       nch, args.feather)
    out = np.zeros(rays[0][0].shape[:2] + (nch,), np.float32)
    for tap in np.asarray(args.twine_spread, np.float32):
        help_ = feather([with_plane(fm.arrays_at_rays(arrays(r, tap), f, g, gw, nch), f) for r, f, g, gw in zip(rays, facets, gs, gws)],
                        nch, args.feather)
        out = fm.f32(out + fm.f32(F(tap[2]) * help_))
    return out
