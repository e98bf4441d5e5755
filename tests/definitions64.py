"""A float64 model of what a rendered pixel is, written from the definitions alone: the projection
definitions, README.md:967-980 (axes RIGHT, DOWN, FORWARD; yaw right, pitch up, roll clockwise) and
the PanoTools lens-correction model. TEST CODE, a helper and not a test. Nothing here is taken from
oracle/eu_oracle.c, from eu_setup_math.h or from the reference's program text: a reading of that text
which the oracle and the library share cannot be shared by this file.

The scene is an analytic function of the unit ray direction (`field`). A source image holds it at
the source's pixel-centre rays (`source_image`), the frame a job should produce is the same function
at the target's rays (`expected`), and whatever lies between the two is the product under test.

The projection numbers are the library's public constants (envutil_amd.SPHERICAL ... BIATAN6).
"""
import math

import numpy as np

SPHERICAL, CYLINDRICAL, RECTILINEAR, STEREOGRAPHIC, FISHEYE, CUBEMAP, BIATAN6 = range(7)
CUBE = (CUBEMAP, BIATAN6)


# ---------------------------------------------------------------------------
# geometry (moved here from tests/test_gpu_geometry.py)
# ---------------------------------------------------------------------------

def rot(roll, pitch, yaw):
    """camera orientation: yaw to the right about DOWN, pitch upward about RIGHT, roll clockwise
    about FORWARD, applied roll first (column vectors): R = Ry(yaw) Rx(pitch) Rz(roll)"""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return ry @ rx @ rz


def planar_to_ray(prj, px, py):
    """pixel-centre planar coordinates -> ray (RIGHT, DOWN, FORWARD), float64"""
    if prj == SPHERICAL:
        return np.stack([np.cos(py) * np.sin(px), np.sin(py), np.cos(py) * np.cos(px)], -1)
    if prj == CYLINDRICAL:
        return np.stack([np.sin(px), py, np.cos(px)], -1)
    if prj == RECTILINEAR:
        return np.stack([px, py, np.ones_like(px)], -1)
    r = np.hypot(px, py)
    theta = r if prj == FISHEYE else 2.0 * np.arctan(r / 2.0)       # stereographic: r = 2 tan(theta / 2)
    phi = np.arctan2(px, py)                                           # from the DOWN axis towards RIGHT
    return np.stack([np.sin(theta) * np.sin(phi), np.sin(theta) * np.cos(phi), np.cos(theta)], -1)


def cube_ray(face, in0, in1):
    """in-face coordinates in [-1, 1] -> ray; faces LEFT0 RIGHT1 TOP2 BOTTOM3 FRONT4 BACK5"""
    one = np.ones_like(in0)
    table = [(-one, in1, in0), (one, in1, -in0), (-in0, -one, -in1), (-in0, one, in1), (in0, in1, one), (-in0, in1, -one)]
    out = np.zeros(in0.shape + (3,))
    for f, (x, y, z) in enumerate(table):
        m = face == f
        out[m] = np.stack([x, y, z], -1)[m]
    return out


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def extent(prj, w, h, hfov):
    """half extents from the definitions: the planar x of a ray hfov / 2 to the right, square pixels"""
    t = hfov / 2.0
    x1 = {SPHERICAL: t, CYLINDRICAL: t, FISHEYE: t, RECTILINEAR: math.tan(t),
          STEREOGRAPHIC: 2.0 * math.tan(t / 2.0), CUBEMAP: math.tan(t), BIATAN6: math.tan(t)}[prj]
    return x1, x1 * h / w


def target_rays_f64(prj, w, h, hfov_deg, dx=0.0, dy=0.0):
    """the rays of the pixel centres of a w x h frame, moved by (dx, dy) pixels in the frame's plane"""
    x1, y1 = extent(prj, w, h, math.radians(hfov_deg))
    xs = -x1 + (np.arange(w) + 0.5 + dx) * (2 * x1 / w)
    ys = -y1 + (np.arange(h) + 0.5 + dy) * (2 * y1 / h)
    px, py = np.meshgrid(xs, ys)
    if prj in CUBE:
        face = (np.arange(h) // w)[:, None] + np.zeros((1, w), int)
        in1 = py + (5 - 2 * face) * x1          # the face's own vertical coordinate in [-x1, x1]
        in0 = px
        if prj == BIATAN6:
            in0, in1 = np.tan(in0 * math.pi / 4.0), np.tan(in1 * math.pi / 4.0)
        return cube_ray(face, in0, in1)
    return planar_to_ray(prj, px, py)


# ---------------------------------------------------------------------------
# the inverse direction: ray -> planar -> pixel
# ---------------------------------------------------------------------------

def ray_to_planar(prj, rays):
    """ray -> (planar x, planar y, in front), the inverse of planar_to_ray"""
    x, y, z = rays[..., 0], rays[..., 1], rays[..., 2]
    ok = np.ones(x.shape, bool)
    if prj == SPHERICAL:
        return np.arctan2(x, z), np.arctan2(y, np.hypot(x, z)), ok
    if prj == CYLINDRICAL:
        return np.arctan2(x, z), y / np.hypot(x, z), ok
    if prj == RECTILINEAR:
        zz = np.where(z > 0, z, 1.0)
        return x / zz, y / zz, z > 0
    s = np.hypot(x, y)
    theta = np.arctan2(s, z)
    r = theta if prj == FISHEYE else 2.0 * np.tan(theta / 2.0)
    s = np.where(s > 0, s, 1.0)
    return r * x / s, r * y / s, ok


def ray_to_cube(rays):
    """ray -> (face, in0, in1): the face of the dominant axis, the inverse of cube_ray"""
    x, y, z = rays[..., 0], rays[..., 1], rays[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    face = np.where((ax >= ay) & (ax >= az), np.where(x < 0, 0, 1),
                    np.where(ay >= az, np.where(y < 0, 2, 3), np.where(z > 0, 4, 5)))
    m = np.maximum(np.maximum(ax, ay), az)
    x, y, z = x / m, y / m, z / m
    in0 = np.choose(face, [z, -z, -x, -x, x, -x])
    in1 = np.choose(face, [y, y, -z, z, y, y])
    return face, in0, in1


# ---------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------

# per channel: constant, x, y, z, yz, xz, xy, x^2 - z^2, y^2 - z^2, xyz. Degree <= 3; on the unit sphere the
# values stay within 0.5 +- 0.4
_COEF = np.array([[0.50, 0.18, 0.00, 0.00, 0.12, 0.00, 0.00, 0.10, 0.00, 0.08],
                  [0.48, 0.00, 0.16, 0.05, 0.00, 0.11, 0.00, 0.00, 0.09, -0.07],
                  [0.52, -0.06, 0.00, 0.17, 0.00, 0.00, 0.13, -0.05, 0.08, 0.06],
                  [0.45, 0.10, -0.12, 0.08, 0.06, -0.07, 0.00, 0.07, 0.00, 0.09]])


def field(rays, channel):
    """the scene: a polynomial of degree 3 in the components of the UNIT direction, one per channel"""
    u = unit(np.asarray(rays, np.float64))
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    c = _COEF[channel]
    return (c[0] + c[1] * x + c[2] * y + c[3] * z + c[4] * y * z + c[5] * x * z + c[6] * x * y
            + c[7] * (x * x - z * z) + c[8] * (y * y - z * z) + c[9] * x * y * z)


def fields(rays, nch):
    """(..., nch): `field` per colour channel, 1 in the alpha channel of 2- and 4-channel pixels"""
    out = np.empty(rays.shape[:-1] + (nch,))
    for c in range(nch):
        out[..., c] = 1.0 if nch in (2, 4) and c == nch - 1 else field(rays, c)
    return out


def plane_scene(points, channel):
    """a smooth function on a plane of 3D points (the translated-facet case): low-order polynomial in the
    point's coordinates"""
    x, y, z = points[..., 0], points[..., 1], points[..., 2]
    k = 0.1 * (channel + 1)
    return 0.5 + 0.07 * x - 0.05 * y + k * 0.1 * x * y + 0.02 * (x * x - y * y) + 0.03 * z


# ---------------------------------------------------------------------------
# the PanoTools lens model (https://wiki.panotools.org/Lens_correction_model):
#   r_src = (a r^3 + b r^2 + c r + d) r_dest,  d = 1 - (a + b + c),
# r in units of half the smaller side of the image; then the image-centre shift, then the shear
# x' = x + g y, y' = y + t x. All in the planar units of the facet (the shift as well: the facet
# carries it already converted from pixels).
# ---------------------------------------------------------------------------

def lens_forward(lens, px, py, r_unit):
    a, b, c = (lens.get(k, 0.0) for k in "abc")
    r = np.hypot(px, py) / r_unit
    f = ((a * r + b) * r + c) * r + (1.0 - (a + b + c))
    x, y = px * f + lens.get("h", 0.0), py * f + lens.get("v", 0.0)
    g, t = lens.get("g", 0.0), lens.get("t", 0.0)
    return x + g * y, y + t * x


def lens_inverse(lens, qx, qy, r_unit):
    """the ideal planar coordinate whose lens_forward image is (qx, qy): shear and shift undone in closed
    form, the radial polynomial by Newton's iteration in float64"""
    a, b, c = (lens.get(k, 0.0) for k in "abc")
    g, t = lens.get("g", 0.0), lens.get("t", 0.0)
    det = 1.0 - g * t
    x, y = (qx - g * qy) / det, (qy - t * qx) / det
    x, y = x - lens.get("h", 0.0), y - lens.get("v", 0.0)
    rs = np.hypot(x, y) / r_unit
    d = 1.0 - (a + b + c)
    r = rs.copy()
    for _ in range(60):
        p = (((a * r + b) * r + c) * r + d) * r - rs
        dp = ((4 * a * r + 3 * b) * r + 2 * c) * r + d
        r = r - p / dp
    f = np.where(rs > 0, r / np.where(rs > 0, rs, 1.0), 1.0 / d)
    return x * f, y * f


# ---------------------------------------------------------------------------
# facets, source images, expectations
# ---------------------------------------------------------------------------

class Facet:
    """what the model needs to know about a source image; angles in degrees"""

    def __init__(self, prj, w, h, hfov, yaw=0.0, pitch=0.0, roll=0.0, lens=None, brighten=1.0, translation=None):
        self.prj, self.w, self.h, self.hfov = prj, w, h, hfov
        self.yaw, self.pitch, self.roll = yaw, pitch, roll
        self.lens, self.brighten = lens, brighten
        self.translation = translation      # see translated_scene()

    @property
    def matrix(self):
        return rot(math.radians(self.roll), math.radians(self.pitch), math.radians(self.yaw))


def pixel_rays(fct):
    """world rays of the facet's pixel centres, (h, w, 3)"""
    x1, y1 = extent(fct.prj, fct.w, fct.h, math.radians(fct.hfov))
    if fct.lens and fct.prj not in CUBE:
        xs = -x1 + (np.arange(fct.w) + 0.5) * (2 * x1 / fct.w)
        ys = -y1 + (np.arange(fct.h) + 0.5) * (2 * y1 / fct.h)
        qx, qy = np.meshgrid(xs, ys)
        px, py = lens_inverse(fct.lens, qx, qy, min(x1, y1))
        local = planar_to_ray(fct.prj, px, py)
    else:
        local = target_rays_f64(fct.prj, fct.w, fct.h, fct.hfov)
    return local @ fct.matrix.T


def source_image(prj, w, h, hfov, nch, yaw=0.0, pitch=0.0, roll=0.0, lens=None):
    """the scene at the rays of the source's pixel centres, float32 (h, w, nch); all seven projections (the cube
    kinds as six stacked faces), any orientation; with `lens`, at the ray whose PanoTools image is the pixel"""
    return fields(pixel_rays(Facet(prj, w, h, hfov, yaw, pitch, roll, lens)), nch).astype(np.float32)


FAULTS = ("source_half_texel", "target_half_pixel", "cube_transposed", "yaw_sign", "weights_unnormalised")


def camera_rays(args, dx=0.0, dy=0.0, fault=None):
    """world rays of the job's pixel centres displaced by (dx, dy) pixels. `args`: envutil_amd.arguments (or
    anything with projection, width, height, hfov, yaw, pitch, roll in degrees)"""
    if fault == "target_half_pixel":
        dx, dy = dx + 0.5, dy + 0.5
    yaw = -args.yaw if fault == "yaw_sign" else args.yaw
    m = rot(math.radians(args.roll), math.radians(args.pitch), math.radians(yaw))
    return target_rays_f64(args.projection, args.width, args.height, args.hfov, dx, dy) @ m.T


def taps_of(args):
    t = getattr(args, "twine_spread", None)
    return None if t is None else np.asarray(t, np.float64).reshape(-1, 3)


def expected(args, nch, fault=None, scene=fields):
    """the frame the job should give: the scene at the float64 target rays under the camera rotation; for a
    twined job the weighted sum over the taps (x, y offsets in pixels of the target, weight) of the scene at
    the rays of the offset planar coordinates, the weights divided by their sum"""
    taps = taps_of(args)
    if taps is None:
        return scene(camera_rays(args, fault=fault), nch)
    total = 1.0 if fault == "weights_unnormalised" else taps[:, 2].sum()
    if fault == "weights_unnormalised":
        taps = taps * np.array([1.0, 1.0, 1.02])
    out = 0.0
    for dx, dy, wgt in taps:
        out = out + wgt / total * scene(camera_rays(args, dx, dy, fault=fault), nch)
    return out


def source_coordinates(fct, rays, fault=None):
    """world rays -> the facet's pixel coordinates in float64 (pixel centres at whole numbers):
    (cx, cy, hit, face | 0). For a cube facet cy counts within the face."""
    local = rays @ fct.matrix
    x1, y1 = extent(fct.prj, fct.w, fct.h, math.radians(fct.hfov))
    shift = 0.5 if fault == "source_half_texel" else 0.0
    if fct.prj in CUBE:
        face, in0, in1 = ray_to_cube(local)
        if fault == "cube_transposed":
            in0, in1 = np.where(face == 4, in1, in0), np.where(face == 4, in0, in1)
        if fct.prj == BIATAN6:
            in0, in1 = np.arctan(in0) * 4.0 / math.pi, np.arctan(in1) * 4.0 / math.pi
        cx = (in0 + x1) / (2 * x1) * fct.w - 0.5 + shift
        cy = (in1 + x1) / (2 * x1) * fct.w - 0.5 + shift
        return cx, cy, np.ones(cx.shape, bool), face
    px, py, ok = ray_to_planar(fct.prj, local)
    if fct.lens:
        px, py = lens_forward(fct.lens, px, py, min(x1, y1))
    cx = (px + x1) / (2 * x1) * fct.w - 0.5 + shift
    cy = (py + y1) / (2 * y1) * fct.h - 0.5 + shift
    hit = ok & (np.abs(px) <= x1) & (np.abs(py) <= y1)
    return cx, cy, hit, np.zeros(cx.shape, int)


def full_sphere(fct):
    return fct.prj == SPHERICAL and abs(fct.hfov - 360.0) < 1e-9 and fct.w == 2 * fct.h


def periodic(fct):
    return fct.prj in (SPHERICAL, CYLINDRICAL) and abs(fct.hfov - 360.0) < 1e-9


class Coverage:
    """per pixel of the job and per facet: hit (the float64 ray lands inside the image), border / seam / pole /
    edge (distances in source texels from the image border of a facet that has one, from the x = 0 / x = w seam
    of a periodic facet, from the poles of a full sphere, from the nearest edge of the cube face);
    np.inf where the facet has no such structure"""

    def __init__(self, hit, border, seam, pole, edge):
        self.hit, self.border, self.seam, self.pole, self.edge = hit, border, seam, pole, edge

    @property
    def covered(self):
        return self.hit.any(0)

    def depth(self):
        """how far inside (+) or outside (-) the best facet's image the ray is, in texels"""
        return self.border.max(0)


def coverage(args, facets, dx=0.0, dy=0.0, rays=None):
    """`rays`: the rays that reach the facets, where they are not the camera's own (a translated facet)"""
    if rays is None:
        rays = camera_rays(args, dx, dy)
    hit, border, seam, pole, edge = [], [], [], [], []
    for f in facets:
        cx, cy, h, _ = source_coordinates(f, rays)
        inf = np.full(cx.shape, np.inf)
        if f.prj in CUBE:
            e = np.minimum(np.minimum(cx + 0.5, f.w - 0.5 - cx), np.minimum(cy + 0.5, f.w - 0.5 - cy))
            hit.append(h), border.append(inf), seam.append(inf), pole.append(inf), edge.append(e)
            continue
        bx = inf if periodic(f) else np.minimum(cx + 0.5, f.w - 0.5 - cx)
        by = inf if full_sphere(f) else np.minimum(cy + 0.5, f.h - 0.5 - cy)
        b = np.minimum(bx, by)
        if f.prj == RECTILINEAR:
            b = np.where((rays @ f.matrix)[..., 2] > 0, b, -np.inf)
        hit.append(h), border.append(b), edge.append(inf)
        seam.append(np.minimum(cx + 0.5, f.w - 0.5 - cx) if periodic(f) else inf)
        pole.append(np.minimum(cy + 0.5, f.h - 0.5 - cy) if full_sphere(f) else inf)
    return Coverage(*(np.stack(v) for v in (hit, border, seam, pole, edge)))


def tier1(args, fct, image, degree, fault=None):
    """the same operation in high precision, for a non-cube facet: float64 source coordinates from the
    definitions, scipy's spline of the same degree over the same float32 samples in float64. The boundary
    schemes scipy can express: REFLECT (mode='reflect') and, for the x axis of a 360 degree facet, PERIODIC
    (mode='grid-wrap'); scipy takes one mode for both axes, so a periodic facet is wrapped in x by hand with a
    margin wider than the prefilter's reach and reflected in y. Returns (frame, hit)."""
    from scipy import ndimage
    assert fct.prj not in CUBE and taps_of(args) is None
    cx, cy, hit, _ = source_coordinates(fct, camera_rays(args, fault=fault), fault)
    img = np.asarray(image, np.float64)
    off = 0
    if periodic(fct):
        off = min(64, fct.w)
        img = np.concatenate([img[:, -off:], img, img[:, :off]], 1)
    out = np.zeros(cx.shape + (img.shape[2],))
    for c in range(img.shape[2]):
        out[..., c] = ndimage.map_coordinates(img[:, :, c], [cy, cx + off], order=degree, mode="reflect")
    return np.where(hit[..., None], out, 0.0), hit


BINS = ((0.0, 0.5), (0.5, 1.0), (1.0, 2.0), (2.0, 4.0), (4.0, 8.0), (8.0, np.inf))


def binned_max(err, dist):
    """max of err (h, w) or (h, w, c) over the pixels whose distance falls in each of BINS; None for an empty bin"""
    e = err if err.ndim == 2 else err.max(-1)
    out = []
    for lo, hi in BINS:
        m = (dist >= lo) & ((dist < hi) | (np.isinf(hi) & (dist == hi)))
        out.append(float(e[m].max()) if m.any() else None)
    return out


def coordinates_to_rays(fct, cx, cy, face):
    """the inverse of source_coordinates: pixel coordinates of the facet -> world rays"""
    x1, y1 = extent(fct.prj, fct.w, fct.h, math.radians(fct.hfov))
    if fct.prj in CUBE:
        in0 = (cx + 0.5) / fct.w * (2 * x1) - x1
        in1 = (cy + 0.5) / fct.w * (2 * x1) - x1
        if fct.prj == BIATAN6:
            in0, in1 = np.tan(in0 * math.pi / 4.0), np.tan(in1 * math.pi / 4.0)
        return cube_ray(face, in0, in1) @ fct.matrix.T
    px = (cx + 0.5) / fct.w * (2 * x1) - x1
    py = (cy + 0.5) / fct.h * (2 * y1) - y1
    if fct.lens:
        px, py = lens_inverse(fct.lens, px, py, min(x1, y1))
    return planar_to_ray(fct.prj, px, py) @ fct.matrix.T


def shifted(fault, args, fct, nch, image=None, degree=None):
    """the model with a deliberate fault, to show that a check can fail: what a renderer with that fault would
    give. `fault` is one of FAULTS: half a source texel, half a target pixel, the front cube face transposed, yaw
    with the wrong sign, tap weights that are not normalised. With `image` and `degree` (non-cube facets) the
    faulty renderer interpolates the samples as tier1 does; without, it looks the scene up exactly."""
    assert fault in FAULTS
    if fault in ("source_half_texel", "cube_transposed"):
        if image is not None and fct.prj not in CUBE:
            return tier1(args, fct, image, degree, fault)[0]
        assert taps_of(args) is None
        cx, cy, hit, face = source_coordinates(fct, camera_rays(args), fault)
        return np.where(hit[..., None], fields(coordinates_to_rays(fct, cx, cy, face), nch), 0.0)
    return expected(args, nch, fault)


# ---------------------------------------------------------------------------
# envelopes
# ---------------------------------------------------------------------------

def kind_of(fct):
    """the row of ENVELOPES a facet belongs to"""
    if fct.prj in CUBE:
        return ("cubemap" if fct.prj == CUBEMAP else "biatan6", fct.w)
    if full_sphere(fct):
        return ("latlon", fct.w)
    return ("plain", 0)


def structure_distance(cov):
    """texels from the nearest thing that disturbs the interpolation: the seam and the poles of a full sphere,
    the edge of a cube face, the image border of every facet the ray hits; inf where there is none"""
    inf = np.full(cov.hit.shape, np.inf)
    per_facet = np.minimum(np.minimum(cov.seam, cov.pole), np.minimum(cov.edge, cov.border))
    return np.where(cov.hit, per_facet, inf).min(0)


HIT_TEST_MARGIN = 0.05     # texels: this close to an image border float32 decides whether the ray hits


class Judgement:
    """one frame against the model: err per pixel (max over channels); the pixels that count (covered, and no
    facet that the ray hits has its image border within 2 texels); their distance from the nearest structure;
    the shares the tests bound; the pixels that lie more than two texels outside every facet"""

    def __init__(self, got, want, cov, need_all=False):
        got = np.asarray(got, np.float64)
        self.err = np.abs(got - want).max(-1)
        anyhit = cov.hit.any(0)
        near_border = ((cov.hit & (cov.border < 2.0)) | (np.abs(cov.border) < HIT_TEST_MARGIN)).any(0)
        # hdr_merge weighs every facet in, also one that the ray misses: it gives the scene where all of them hit
        self.counted = (cov.hit.all(0) if need_all else anyhit) & ~near_border
        self.covered_share = float(anyhit.mean())
        self.left_out_share = float((anyhit & ~self.counted).sum() / max(anyhit.sum(), 1))
        self.dist = structure_distance(cov)
        self.outside = ~anyhit & (cov.border < -2.0).all(0)
        self.outside_max = float(np.abs(got[self.outside]).max()) if self.outside.any() else 0.0

    def bins(self):
        return binned_max(np.where(self.counted, self.err, 0.0), np.where(self.counted, self.dist, -1.0))

    def max(self):
        return float(self.err[self.counted].max())

    def far_max(self):
        """over the counted pixels 8 texels and more from any structure"""
        return float(self.err[self.counted & (self.dist >= 8.0)].max())


def judge(got, args, facets, nch, want=None, need_all=None):
    facets = list(facets) if isinstance(facets, (list, tuple)) else [facets]
    cov = coverage(args, facets)
    if want is None:
        want = expected(args, nch)
    if need_all is None:
        need_all = getattr(args, "synopsis", "panorama") == "hdr_merge"
    return Judgement(got, np.where(cov.covered[..., None], want, 0.0), cov, need_all)


# What the CPU oracle measures against this model: max abs error over the case lists below, which
# tests/test_oracle_definitions.py and tests/test_gpu_definitions.py share. Printed by print_envelopes():
#     python -c "import sys; sys.path.insert(0, 'tests'); import definitions64; definitions64.print_envelopes()"
# ("floor", degree): the interpolation-exact cases, 8 texels and more from any structure.
# (kind, size, degree): per bin of BINS, the distance in texels from the seam and the poles (latlon), from the face
# edge (cubemap, biatan6), from the image border (plain: the first three bins are the pixels left out, and empty).
# ("twine", n): twined jobs over a plain source, degree 3, whole frame.
# bounds() derives the tolerances: floor x 4, bins x 2, the last bin (8 texels and more) held to the floor.
ENVELOPES = {
    ('floor', 2): 1.58e-06,
    ('latlon', 256, 2): [2.39e-05, 2.51e-05, 7.82e-06, 1.54e-06, 2.98e-07, 4.61e-07],
    ('latlon', 128, 2): [2.43e-05, 1.81e-05, 9.25e-06, 1.85e-06, 1.51e-06, 1.62e-06],
    ('cubemap', 64, 2): [3.16e-04, 2.41e-05, 5.52e-06, 8.18e-07, 4.50e-07, 6.52e-07],
    ('cubemap', 32, 2): [3.48e-04, 7.84e-05, 5.68e-05, 3.88e-06, 2.92e-06, 4.24e-06],
    ('biatan6', 64, 2): [2.19e-04, 6.53e-05, 3.36e-05, 6.60e-06, 4.67e-07, 5.08e-07],
    ('biatan6', 32, 2): [8.02e-04, 1.62e-04, 8.23e-05, 1.33e-05, 1.33e-06, 1.23e-06],
    ('plain', 0, 2): [0.00e+00, 0.00e+00, 0.00e+00, 2.39e-05, 7.27e-07, 4.12e-07],
    ('floor', 3): 3.33e-07,
    ('latlon', 256, 3): [8.09e-05, 8.51e-05, 2.92e-05, 6.62e-06, 5.33e-07, 4.30e-07],
    ('latlon', 128, 3): [8.19e-05, 6.40e-05, 3.20e-05, 6.62e-06, 7.00e-07, 4.48e-07],
    ('cubemap', 64, 3): [3.67e-04, 3.77e-05, 1.39e-05, 2.02e-06, 4.14e-07, 4.55e-07],
    ('cubemap', 32, 3): [4.65e-04, 1.03e-04, 8.28e-05, 5.66e-06, 5.53e-07, 5.04e-07],
    ('biatan6', 64, 3): [2.63e-04, 8.25e-05, 3.98e-05, 9.95e-06, 7.65e-07, 4.17e-07],
    ('biatan6', 32, 3): [9.96e-04, 2.00e-04, 1.47e-04, 2.45e-05, 2.76e-06, 3.39e-07],
    ('plain', 0, 3): [0.00e+00, 0.00e+00, 0.00e+00, 3.68e-05, 2.76e-06, 3.97e-07],
    ('twine', 2): 1.09e-06,
    ('twine', 3): 1.23e-06,
}

FLOOR_MARGIN, BIN_MARGIN = 4.0, 2.0


def floor_tolerance(degree):
    return FLOOR_MARGIN * ENVELOPES[("floor", degree)]


def bounds(kind, degree):
    """tolerance per bin of BINS for a source of this kind (kind_of) and spline degree"""
    row = ENVELOPES[kind + (degree,)]
    return [BIN_MARGIN * v for v in row[:-1]] + [floor_tolerance(degree)]


def assert_within(j, kind, degree, what=""):
    """every counted pixel within the envelope of its bin; returns the per-bin maxima"""
    got = j.bins()
    for (lo, hi), g, b in zip(BINS, got, bounds(kind, degree)):
        assert g is None or g <= b, f"{what}: {g:.3g} > {b:.3g} at {lo} to {hi} texels from the structure; bins {got}"
    return got


# ---------------------------------------------------------------------------
# the cases: shared by the CPU test of the oracle, the GPU test of the library and print_envelopes()
# ---------------------------------------------------------------------------

T_RECT = (RECTILINEAR, 150, 77, 80.0)
T_SPH = (SPHERICAL, 200, 100, 360.0)
T_CUBE48 = (CUBEMAP, 48, 288, 90.0)
T_CUBE24 = (CUBEMAP, 24, 144, 90.0)
UPRIGHT, ROTATED = (0.0, 0.0, 0.0), (30.0, 15.0, 7.5)

LENS = dict(a=0.02, b=0.0, c=-0.01, h=0.01, v=-0.02, g=0.003, t=-0.002)

# sources without seam, pole or face edge: the interpolation-exact kind. (facet, camera looking at its middle)
PLAIN = {
    "spherical": Facet(SPHERICAL, 128, 64, 180.0, 10.0, 5.0, 3.0),
    "cylindrical": Facet(CYLINDRICAL, 128, 64, 200.0, 5.0, -4.0, 2.0),
    "rectilinear": Facet(RECTILINEAR, 128, 96, 100.0, 20.0, -10.0, 5.0),
    "stereographic": Facet(STEREOGRAPHIC, 128, 128, 220.0, -10.0, 8.0, 30.0),
    "fisheye": Facet(FISHEYE, 128, 128, 200.0, 15.0, 5.0, -20.0),
    "fisheye lens": Facet(FISHEYE, 128, 128, 190.0, 10.0, 5.0, -3.0, lens=LENS),
    "rectilinear lens": Facet(RECTILINEAR, 128, 96, 80.0, -5.0, 3.0, 2.0, lens=dict(LENS, h=0.02, v=-0.01)),
}
LATLON = {256: Facet(SPHERICAL, 256, 128, 360.0), 128: Facet(SPHERICAL, 128, 64, 360.0)}
CUBES = {("cubemap", 64): Facet(CUBEMAP, 64, 384, 90.0), ("cubemap", 32): Facet(CUBEMAP, 32, 192, 90.0),
         ("biatan6", 64): Facet(BIATAN6, 64, 384, 90.0), ("biatan6", 32): Facet(BIATAN6, 32, 192, 90.0)}


def doubled(fct):
    """the same facet at twice the resolution"""
    return Facet(fct.prj, 2 * fct.w, 2 * fct.h, fct.hfov, fct.yaw, fct.pitch, fct.roll, fct.lens, fct.brighten)


def looking_at(fct, target=T_RECT, hfov=None, extra=(0.0, 0.0, 0.0)):
    """(target, ypr) of a camera that looks where the facet looks, plus `extra`"""
    t = target if hfov is None else target[:3] + (hfov,)
    return t, (fct.yaw + extra[0], fct.pitch + extra[1], fct.roll + extra[2])


def exact_cases():
    """(name, facet, target, ypr): every non-cube source projection where interpolation of degree 2 and 3 is
    exact to the float32 floor; lat/lon away from the seam (behind the camera) and the poles"""
    out = []
    for name, f in PLAIN.items():
        hfov = 60.0 if f.prj == RECTILINEAR else 80.0
        out.append((name, f) + looking_at(f, hfov=hfov))
        out.append((name + ", turned", f) + looking_at(f, hfov=hfov - 10.0, extra=(4.0, -3.0, 20.0)))
    for w, f in LATLON.items():
        out.append((f"latlon {w} interior", f, T_RECT, (40.0, 10.0, 5.0)))
    return out


def envelope_cases():
    """(kind, facet, target, ypr): frames that cross the seam, the poles, the cube face edges, and for the plain
    kind the image border"""
    out = []
    for w, f in LATLON.items():
        out += [(kind_of(f), f, T_SPH, UPRIGHT), (kind_of(f), f, T_SPH, ROTATED), (kind_of(f), f, T_CUBE48, UPRIGHT),
                (kind_of(f), f, (SPHERICAL, f.w, f.h, 360.0), UPRIGHT), (kind_of(f), f, T_RECT, (170.0, 60.0, 10.0))]
    for kind, f in CUBES.items():
        out += [(kind, f, T_SPH, UPRIGHT), (kind, f, T_SPH, ROTATED), (kind, f, T_RECT, ROTATED), (kind, f, T_CUBE48, ROTATED)]
    for name, hfov in (("rectilinear", 115.0), ("rectilinear lens", 95.0), ("cylindrical", 120.0)):
        out.append((("plain", 0), doubled(PLAIN[name])) + looking_at(PLAIN[name], hfov=hfov, extra=(2.0, 1.0, 5.0)))
    f = synopsis_facets()[0]
    out.append((("plain", 0), f) + looking_at(f, hfov=110.0))
    return out


def twine_cases():
    """(twine, facet, target, ypr, smaller target): 2 x 2 and 3 x 3 box spreads of width 1 over a plain source"""
    f = PLAIN["fisheye"]
    t, ypr = looking_at(f, extra=(3.0, 2.0, 10.0))
    return [(n, f, t, ypr, (t[0], t[1] // 2, t[2] // 2, t[3])) for n in (2, 3)]


def synopsis_facets():
    """six facets that all look at the same scene: four fisheyes round the horizon, a rectilinear one up and one
    down; between them they leave holes. 256 wide: the share of a facet within 2 texels of its border is 3 %"""
    fs = [Facet(FISHEYE, 256, 256, 95.0, 90.0 * k + 10.0, 5.0 * (-1) ** k, 7.0 * k) for k in range(4)]
    return fs + [Facet(RECTILINEAR, 256, 256, 80.0, 20.0, 88.0, 0.0), Facet(RECTILINEAR, 256, 256, 80.0, -30.0, -87.0, 15.0)]


def bracket_facets(n=3):
    """an exposure bracket: n facets, nearly the same view, brighten 1 to 2.5; each image holds the scene divided
    by its brighten, which stays below 1: nothing clips"""
    return [Facet(RECTILINEAR, 256, 192, 90.0, 0.25 * k, -0.125 * k, 0.0, brighten=1.0 + 1.5 * k / (n - 1)) for k in range(n)]


def lens_facets():
    """a job with lens-polynomial facets among its facets"""
    return [doubled(PLAIN["fisheye lens"]), doubled(PLAIN["rectilinear lens"]),
            Facet(STEREOGRAPHIC, 256, 256, 150.0, 170.0, -8.0, 30.0)]


def facet_image(fct, nch):
    """the image a facet holds: the scene at its pixel rays, divided by its brighten (colour channels)"""
    if fct.translation:
        return translated_image(fct, nch)
    img = fields(pixel_rays(fct), nch)
    ncol = nch - 1 if nch in (2, 4) else nch
    img[..., :ncol] /= fct.brighten
    return img.astype(np.float32)


def synopsis_cases():
    """(name, facets, target, ypr, synopsis)"""
    return [("panorama", synopsis_facets(), T_SPH, (5.0, 2.0, 1.0), "panorama"),
            ("panorama on a cube", synopsis_facets(), T_CUBE48, (8.0, 3.0, 2.0), "panorama"),
            ("hdr_merge", bracket_facets(), (RECTILINEAR, 150, 77, 100.0), (0.5, -0.2, 3.0), "hdr_merge"),
            ("lens facets", lens_facets(), T_SPH, (5.0, 2.0, 1.0), "panorama")]


def single_sources():
    """the single sources of the kernel-family cases"""
    return {"latlon256": LATLON[256], "latlon128": LATLON[128], "cubemap64": CUBES[("cubemap", 64)],
            "cubemap32": CUBES[("cubemap", 32)], "biatan6 64": CUBES[("biatan6", 64)], "fisheye": PLAIN["fisheye"],
            "rectilinear": PLAIN["rectilinear"]}


def jobs_of(f):
    """(target, ypr) for a single source: the four targets upright and rotated where the source covers the sphere,
    else windows that look at the facet, upright, turned, and one wide enough to show its borders"""
    if kind_of(f)[0] == "plain":
        hfov = 60.0 if f.prj == RECTILINEAR else 80.0
        return [looking_at(f, hfov=hfov), looking_at(f, hfov=hfov - 10.0, extra=(4.0, -3.0, 20.0)),
                looking_at(f, hfov=115.0, extra=(2.0, 1.0, 5.0))]
    return [(t, ypr) for t in (T_RECT, T_SPH, T_CUBE48, T_CUBE24) for ypr in (UPRIGHT, ROTATED)]


VIEWS = [(0.0, 0.0, 0.0), (30.0, 15.0, 7.5), (-100.0, -40.0, 20.0, 95.0)]
NEAR_VIEWS = [(0.0, 0.0, 0.0), (2.0, 1.0, 3.0), (-3.0, 2.0, -5.0, 95.0)]


def view_cases():
    """(name, facets, target, synopsis, views): three views (yaw, pitch, roll[, hfov]) rendered in one call"""
    return [("latlon256", [LATLON[256]], T_RECT, "panorama", VIEWS), ("cubemap64", [CUBES[("cubemap", 64)]], T_RECT, "panorama", VIEWS),
            ("six facets", synopsis_facets(), (SPHERICAL, 200, 100, 300.0), "panorama", VIEWS),
            ("six facets, bracket", bracket_facets(6), (RECTILINEAR, 150, 77, 100.0), "hdr_merge", NEAR_VIEWS)]


def view_jobs(t, views):
    """(target, ypr) of each view of a shared target"""
    return [(t[:3] + (v[3] if len(v) == 4 else t[3],), v[:3]) for v in views]


def all_envelope_jobs():
    """(kind, facets, target, ypr, synopsis): everything that is held to a row of ENVELOPES, on the CPU and on the GPU"""
    out = [(kind, [f], t, ypr, "panorama") for kind, f, t, ypr in envelope_cases()]
    out += [(kind_of(f), [f], t, ypr, "panorama") for f in single_sources().values() for t, ypr in jobs_of(f)]
    for name, fs, t, syn, views in view_cases():
        out += [(kind_of(fs[0]) if len(fs) == 1 else ("plain", 0), fs, tk, ypr, syn) for tk, ypr in view_jobs(t, views)]
    out += [(("plain", 0), fs, t, ypr, syn) for name, fs, t, ypr, syn in synopsis_cases()]
    return out


# ---------------------------------------------------------------------------
# a translated facet (PTO TrX, TrY, TrZ, Tpy, Tpp). The conventions, read from the reference's generic_r3 and
# tf3d_t and restated as geometry: the scene lies on the translation plane, which is at unit distance from the
# origin of model space with its normal along the FORWARD axis of the orientation (Tpy, Tpp) - yaw and pitch as for
# a camera; the target camera stands at the origin; the facet was taken from the point (tr_x, tr_y, tr_z) of model
# space (RIGHT, DOWN, FORWARD; facet_spec's z is already the negated PTO TrZ). A target ray that runs away from the
# plane sees nothing.
# ---------------------------------------------------------------------------

def plane_matrix(tr):
    return rot(math.radians(tr.get("tp_r", 0.0)), math.radians(tr.get("tp_p", 0.0)), math.radians(tr.get("tp_y", 0.0)))


def on_plane(origin, dirs, tr):
    """where the rays origin + t dirs meet the translation plane: (points, t > 0)"""
    n = plane_matrix(tr)[:, 2]
    nd = dirs @ n
    t = (1.0 - origin @ n) / np.where(nd != 0, nd, 1.0)
    ok = (nd != 0) & (t > 0)
    return origin + np.where(ok, t, 1.0)[..., None] * dirs, ok


def plane_fields(points, tr, nch):
    q = points @ plane_matrix(tr)          # in the plane's own frame: (x, y, 1)
    out = np.empty(points.shape[:-1] + (nch,))
    for c in range(nch):
        out[..., c] = 1.0 if nch in (2, 4) and c == nch - 1 else plane_scene(q, c)
    return out


def translated_facet():
    return Facet(RECTILINEAR, 128, 96, 90.0, 4.0, -2.0, 1.0, translation=dict(x=0.1, y=-0.05, z=0.08, tp_y=10.0, tp_p=-5.0))


def camera_position(fct):
    return np.array([fct.translation.get(k, 0.0) for k in "xyz"])


def translated_image(fct, nch):
    """the scene on the plane as the facet's camera sees it from where it stands"""
    pts, ok = on_plane(camera_position(fct), pixel_rays(fct), fct.translation)
    assert ok.all()
    return plane_fields(pts, fct.translation, nch).astype(np.float32)


def judge_translated(got, args, fct, nch):
    """the frame of a job over a translated facet against plain geometry: the target ray from the origin meets
    the plane at a point; the frame shows the scene there, where the facet's camera, looking from its own place,
    has that point in its image"""
    pts, ok = on_plane(np.zeros(3), camera_rays(args), fct.translation)
    cov = coverage(args, [fct], rays=pts - camera_position(fct))
    cov.hit &= ok
    want = np.where(cov.hit[0][..., None], plane_fields(pts, fct.translation, nch), 0.0)
    return Judgement(got, want, cov)


def measure_envelopes(render, make_args):
    """{key of ENVELOPES: measured maxima}. render(facets, degree, args, nch) -> frame;
    make_args(target, ypr, degree, **kw) -> the job's arguments"""
    table = {}

    def widen(key, got):
        row = table.setdefault(key, [0.0] * len(BINS))
        table[key] = [max(r, g or 0.0) for r, g in zip(row, got)]

    for degree in (2, 3):
        table[("floor", degree)] = 0.0
        for name, f, t, ypr in exact_cases():
            a = make_args(t, ypr, degree)
            j = judge(render([f], degree, a, 3), a, [f], 3)
            table[("floor", degree)] = max(table[("floor", degree)], j.far_max())
        for kind, fs, t, ypr, syn in all_envelope_jobs():
            for nch in (3, 4) if len(fs) > 1 else (3,):
                a = make_args(t, ypr, degree, synopsis=syn)
                widen(kind + (degree,), judge(render(fs, degree, a, nch), a, fs, nch).bins())
    for n, f, t, ypr, _ in twine_cases():
        a = make_args(t, ypr, 3, twine=n)
        table[("twine", n)] = judge(render([f], 3, a, 3), a, [f], 3).max()
    return table


def oracle_render(facets, degree, args, nch):
    """the CPU oracle's frame of the job (tests/jobs.py)"""
    import jobs
    srcs = [jobs.OracleSource(f.prj, f.w, f.h, f.hfov, facet_image(f, nch), degree, yaw=f.yaw, pitch=f.pitch,
                              roll=f.roll, lens=f.lens, brighten=f.brighten, translation=f.translation) for f in facets]
    return jobs.oracle_render(args, srcs if len(srcs) > 1 else srcs[0])


def make_args(target, ypr, degree, **kw):
    import envutil_amd as ea
    return ea.arguments(*target, yaw=ypr[0], pitch=ypr[1], roll=ypr[2], spline_degree=degree, **kw)


def print_envelopes():
    """prints the ENVELOPES table from the CPU oracle; run on the CPU, pasted in above"""
    for k, v in measure_envelopes(oracle_render, make_args).items():
        v = f"{v:.2e}" if isinstance(v, float) else "[" + ", ".join(f"{x:.2e}" for x in v) + "]"
        print(f"    {k!r}: {v},")
