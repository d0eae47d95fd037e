"""examples/level_pipeline.cpp --color (-m gpu): the camera frame as a padded colour image, read raw by the levels
(nmi_level_set_frame_format) and turned grey on the device, still recovers the planted offset; with --files the channel order
is the settings file's Camera.RGB."""
import os
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


@pytest.mark.parametrize("color, name", [("rgb", "RGB"), ("bgra", "BGRA")])
def test_color_pipeline_recovers_planted_offset(color, name):
    out = run(["4", "--color", color])
    assert f"colour frame: {name}, 848 x 480 in rows of" in out


def test_color_order_from_settings_file(tmp_path):
    """The written settings file has no Camera.RGB: it reads as 0, BGR, whatever order --color names."""
    subprocess.check_call([EXE, "--write-files", str(tmp_path)], stdout=subprocess.DEVNULL)
    out = run(["2", "--files", str(tmp_path), "--color", "rgba"])
    assert "colour frame: BGRA" in out
