"""tests/golden/ref_digests.json, stepper_digests.json (the keys "stepper_...") and pixel_value_digests.json (the keys "pixval_..."): the SHA-256 (refz.digest) of every result of the reference library
(oracle/_ref/libref_zimt.so) that the tests marked 'ref' compare with through refz.same - recorded by running
those tests live. Where the reference checkout exists, after building:
    python tests/golden/make_ref_digests.py"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refz  # noqa: E402

if not refz.available():
    raise SystemExit("oracle/_ref/libref_zimt.so is not built")
refz.RECORDING = True
tests = os.path.dirname(HERE)
rc = pytest.main(["-q", "-p", "no:cacheprovider"] + [os.path.join(tests, f) for f in (
    "test_oracle_vs_ref.py", "test_oracle_pixel_values.py", "test_stepper_pinned.py", "test_mask_pinned.py::test_live", "test_imageprep.py::test_binomial_matches_zimt_live")])
if rc != 0:
    raise SystemExit("the live tests failed: nothing written")
stepper = {k: v for k, v in refz.RECORDED.items() if k.startswith("stepper_")}
pixval = {k: v for k, v in refz.RECORDED.items() if k.startswith("pixval_")}
rest = {k: v for k, v in refz.RECORDED.items() if k not in stepper and k not in pixval}
json.dump(dict(sorted(rest.items())), open(refz.DIGESTS, "w"), indent=0)
json.dump(dict(sorted(stepper.items())), open(refz.STEPPER_DIGESTS, "w"), indent=0)
json.dump(dict(sorted(pixval.items())), open(refz.PIXEL_DIGESTS, "w"), indent=0)
print("wrote ref_digests.json:", len(rest), "digests; stepper_digests.json:", len(stepper), "digests;",
      "pixel_value_digests.json:", len(pixval), "digests")
