"""tests/golden/stepper_golden.npz: what the reference's own steppers (stepper.h through oracle/_ref/libref_zimt.so,
refz.stepper_rays / refz.deriv_rays) emit for the small jobs of tests/stepper_cases.py (in_fixture), with the inputs
they were given. Numbers only. Per job NAME:
    NAME/meta   float64: projection, width, height, twined, extent x0 x1 y0 y1, camera yaw pitch roll,
                facet yaw pitch roll (degrees), crop x0 x1 y0 y1 (zeros: none)
    NAME/basis  float64 (9,): rows xx, yy, zz - rotate(r_camera, r_facet^-1) from the oracle's euo_make_r3 /
                euo_rotate_r3; an INPUT of the reference (it makes its own with Imath), not pinned by it
    NAME/rays   float32 (rows, width, 3): S<float, 16, false> of a plain job, or
    NAME/nine   float32 (rows, width, 9): deriv_stepper<float, 16, S>, bias .25, of a twined job
The larger jobs are covered by their digests (tests/golden/stepper_digests.json). Where the reference checkout exists,
after building:
    python tests/golden/make_stepper_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refz  # noqa: E402
from stepper_cases import BIAS, CASES, in_fixture  # noqa: E402

if not refz.available():
    raise SystemExit("oracle/_ref/libref_zimt.so is not built")
out = {}
for c in CASES:
    if not in_fixture(c):
        continue
    kw = dict(offset=c.offset, out_shape=c.out_shape)
    out[c.name + "/meta"] = c.meta()
    out[c.name + "/basis"] = c.basis
    if c.twined:
        out[c.name + "/nine"] = refz.deriv_rays(c.prj, c.w, c.h, c.extent, c.basis, BIAS, **kw)
    else:
        out[c.name + "/rays"] = refz.stepper_rays(c.prj, False, c.w, c.h, c.extent, c.basis, **kw)
path = os.path.join(HERE, "stepper_golden.npz")
np.savez_compressed(path, **out)
print("wrote stepper_golden.npz:", len(out) // 3, "jobs,", os.path.getsize(path), "bytes")
