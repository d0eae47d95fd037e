"""CPU checks (-m "not gpu") of the planted frames the valid-range pipeline tests run on (tests/helpers/valid_pipeline_cases.py),
with the numpy twin (tests/helpers/valid_np.py) alone, and of the two calls' presence in the header and the binding.

The premises: the ranged EQUALIZE and PERCENTILE tables differ from the unranged ones; the validity mask has both values, between
10 % and 50 % of it zero; ANDed with the hood mask it is neither of the two; at factor 2 an output pixel is invalid because of
exactly one of its four source pixels.  The GPU tests assert the same on the frames they build from their rendered scene."""
import os
import re

import numpy as np
import pytest

from helpers import valid_np as vnp
from helpers import valid_pipeline_cases as cases
from orbslam2_nmi_amd import capi, synthetic as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (5, 9, 11)      # test_valid_stream.py's frames


@pytest.mark.parametrize("f", cases.FACTORS)
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planted_frames_meet_their_premises(size, f):
    w, h = size
    for seed in SEEDS:
        gray = sy.camera_frame(sy.scene(w, h, seed), seed + 1)
        px = cases.frame(gray, f, seed)
        assert px.shape == (f * h, f * w) and px.dtype == np.uint16
        assert (px == 0).any() and int((px == 65535).sum()) == cases.DEAD
        ok = vnp.valid(px, cases.RANGE)
        assert int(px[ok].min()) >= 9000 and int(px[ok].max()) <= cases.RANGE[1]
        cases.premises(px, f)


def test_nothing_valid_is_an_all_zero_table_and_mask():
    w, h = cases.SIZES[0]
    px = np.zeros((h, w), np.uint16)
    px[::5, ::7] = 65535
    for tm in cases.tone_maps().values():
        if not vnp.tiled(tm) and vnp.from_frame(tm):
            assert (vnp.table(px, tm, cases.RANGE)[0] == 0).all()
    assert (vnp.mask(px, 1, cases.RANGE) == 0).all()


def test_header_and_binding_have_the_two_calls():
    with open(os.path.join(ROOT, "include", "nmi_hip.h")) as fh:
        header = fh.read()
    for name in ("nmi_level_set_valid_range", "nmi_stream_set_valid_range"):
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in capi.EXPORTED_SYMBOLS
    assert callable(getattr(capi.NmiLevel, "set_valid_range", None)) and callable(getattr(capi.NmiStream, "set_valid_range", None))
    assert "take no valid range" not in header and "a valid range in captured levels and streams" not in header
