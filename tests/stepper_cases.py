"""The jobs of tests/test_stepper_pinned.py, tests/test_gpu_stepper_pinned.py and tests/golden/make_stepper_golden.py:
one list, so that the CPU oracle, the HIP library and the committed fixture are held to the reference's steppers
(stepper.h through oracle/_ref, tests/refz.py) on the same inputs. TEST CODE.

A case is a target (projection, size, hfov -> extent), a camera orientation, a facet orientation, plain or twined,
and optionally a crop window. Sizes walk every path of zimt's driver at 16 lanes and segments of 512: 1 and 15 (the
capped init and stuff()), 16, 17, 512, 513 (a one-pixel second segment), 1037 (two segment restarts and a 13-lane
tail), 2048; cube targets at 37, 100 and 529 (a segment restart in every row of six faces)."""
import math
import types

import numpy as np

import euo

# (projection, hfov in degrees): rectilinear at 5 degrees has a tiny delta, so drift over a segment shows
TARGETS = [(euo.SPHERICAL, 360.0), (euo.SPHERICAL, 100.0), (euo.CYLINDRICAL, 360.0), (euo.RECTILINEAR, 100.0),
           (euo.RECTILINEAR, 5.0), (euo.STEREOGRAPHIC, 200.0), (euo.FISHEYE, 220.0)]
CUBE_TARGETS = [(euo.CUBEMAP, 90.0), (euo.BIATAN6, 90.0)]
SIZES = [(1, 1), (15, 3), (16, 4), (17, 6), (512, 2), (513, 7), (1037, 19), (2048, 2)]
CUBE_SIZES = [(37, 222), (100, 600), (529, 3174)]
# (camera yaw, pitch, roll), (facet yaw, pitch, roll), degrees
ORIENTATIONS = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                ((33.0, -21.0, 7.0), (0.0, 0.0, 0.0)),
                ((180.0, 90.0, 0.0), (0.0, 0.0, 0.0)),
                ((33.0, -21.0, 7.0), (40.0, -15.0, 20.0))]
BIAS = 0.25                     # deriv_stepper's default (stepper.h:1617)
TAPS = np.array([[0.25, 0.25, 0.5], [-0.25, -0.25, 0.5]], np.float32)   # any tap table makes the oracle's job twined


class Case:
    def __init__(self, prj, hfov, w, h, cam, fct, twined, crop=None):
        self.prj, self.hfov, self.w, self.h = prj, hfov, w, h
        self.cam, self.fct, self.twined, self.crop = cam, fct, twined, crop
        self.name = "%s%g_%dx%d_c%g.%g.%g_f%g.%g.%g_%s" % ((euo.PRJ_NAMES[prj], hfov, w, h) + cam + fct
                                                          + ("twined" if twined else "plain",))
        if crop:
            self.name += "_crop%d.%d.%d.%d" % crop

    @property
    def extent(self):
        return euo.get_extent(self.prj, self.w, self.h, math.radians(self.hfov))

    @property
    def basis(self):
        """rotate(r_camera, r_facet^-1) as envutil_payload.cc makes it, through the oracle's euo_make_r3 /
        euo_rotate_r3: the reference does this with Imath, so the basis is an INPUT of the pinned steppers"""
        cy, cp, cr = (math.radians(v) for v in self.cam)
        fy, fp, fr = (math.radians(v) for v in self.fct)
        return euo.rotate_r3(euo.make_r3(cr, cp, cy), euo.make_r3(fr, fp, fy, inverse=True)).reshape(9)

    @property
    def offset(self):
        return (self.crop[0], self.crop[2]) if self.crop else (0, 0)

    @property
    def out_shape(self):
        """(width, height) of the processed frame"""
        return (self.crop[1] - self.crop[0], self.crop[3] - self.crop[2]) if self.crop else (self.w, self.h)

    def oracle_args(self):
        """what jobs.oracle_render reads of an envutil_amd.arguments"""
        return types.SimpleNamespace(projection=self.prj, width=self.w, height=self.h, extent=tuple(self.extent),
                                     yaw=self.cam[0], pitch=self.cam[1], roll=self.cam[2],
                                     twine_spread=TAPS if self.twined else None,
                                     store_cropped=self.crop is not None, p_crop=self.crop)

    def meta(self):
        """the inputs as one float64 vector, for the fixture"""
        return np.array([self.prj, self.w, self.h, int(self.twined)] + list(self.extent) + list(self.cam)
                        + list(self.fct) + list(self.crop or (0, 0, 0, 0)), np.float64)


def _cases():
    out = []
    for ti, (prj, hfov) in enumerate(TARGETS):
        for si, (w, h) in enumerate(SIZES):
            for twined in (False, True):
                # every orientation meets every target and every size over the list
                cam, fct = ORIENTATIONS[(ti + si + int(twined)) % 4]
                out.append(Case(prj, hfov, w, h, cam, fct, twined))
    for ti, (prj, hfov) in enumerate(CUBE_TARGETS):
        for si, (w, h) in enumerate(CUBE_SIZES):
            for twined in (False, True):
                cam, fct = ORIENTATIONS[(ti + si + 2 * int(twined) + 1) % 4]
                out.append(Case(prj, hfov, w, h, cam, fct, twined))
    # crop windows: x offsets 500, 1019 and 7 are multiples neither of 16 nor of 512, and 600 processed columns
    # put a segment restart at frame column 1012
    for prj, hfov in TARGETS[::2] + TARGETS[1::2]:
        k = len(out)
        cam, fct = ORIENTATIONS[1 + k % 3]
        out.append(Case(prj, hfov, 1600, 40, cam, fct, bool(k % 2), crop=(500, 1100, 3, 30)))
    for ti, (prj, hfov) in enumerate(CUBE_TARGETS):
        for twined in (False, True):
            out.append(Case(prj, hfov, 100, 600, ORIENTATIONS[3 - ti][0], ORIENTATIONS[3 - ti][1], twined,
                            crop=(7, 93, 150, 500)))
    # one small cropped ninepack for the fixture
    out.append(Case(euo.SPHERICAL, 360.0, 1600, 40, ORIENTATIONS[3][0], ORIENTATIONS[3][1], True,
                    crop=(1019, 1043, 3, 9)))
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def in_fixture(c):
    """the jobs whose reference arrays tests/golden/stepper_golden.npz holds in full: every projection at widths 15
    to 37 (the cube targets' ninepacks at 37 x 222 would be 300 KB each: those stay with their digests), one job
    past a segment boundary, one cropped ninepack"""
    if c.crop:
        return c.out_shape == (24, 6)
    if c.prj in (euo.CUBEMAP, euo.BIATAN6):
        return c.w == 37 and not c.twined
    return 15 <= c.w <= 17 or (c.w == 513 and c.prj == euo.SPHERICAL and c.hfov == 360.0 and not c.twined)
