"""examples/level_pipeline.cpp --color with a raw sensor format (-m gpu): the camera frame as a Bayer mosaic or as packed YUV
4:2:2, read raw by the levels (nmi_level_set_frame_format / _set_frame_reduction) and turned grey on the device, exits 0 and
reports the winner of the grey run of the same scene."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "level_pipeline")
pytestmark = pytest.mark.gpu


def run(args):
    if not os.access(EXE, os.X_OK):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PIPELINE OK" in r.stdout
    return r.stdout


def winner(out):
    """relocalized, failed, iterations, stop and the recovered translation of the run."""
    m = re.search(r"^(relocalized=\d+ failed=\d+ iterations=\d+ stop=\d+  recovered t = \([^)]*\))", out, re.M)
    assert m, out
    return m.group(1)


def test_bayer_pipeline_reports_the_grey_runs_winner():
    out = run(["4", "--color", "bayer-rggb"])
    assert "raw sensor frame: BAYER_RGGB, 848 x 480 in rows of 1024 bytes" in out
    assert winner(out) == winner(run(["4"]))


def test_reduced_yuyv_pipeline_reports_the_grey_runs_winner():
    out = run(["4", "--color", "yuyv", "--reduce", "2"])
    assert "full-size raw sensor frame: YUYV, 1696 x 960 in rows of 3584 bytes" in out
    grey = run(["4", "--reduce", "2"])
    assert winner(out) == winner(grey)
    pick = lambda o: [l for l in o.splitlines() if l.startswith(("NmiKernel:", "relocalized="))]
    assert pick(out) == pick(grey)      # the luma bytes are the grey frame: every score is the grey run's


def test_an_unknown_format_is_refused():
    r = subprocess.run([EXE, "2", "--color", "nv12"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--color takes" in r.stderr
