"""examples/level_pipeline.cpp --reduce (-m gpu): the camera frame rendered at F times the search size, read raw by the levels
(nmi_level_set_frame_reduction) and reduced on the device, still recovers the planted offset -- grey and in colour, for cloud and
mesh maps, plain and masked levels; with --files the settings file describes the full-size camera and goes through
nmi_config_reduce."""
import os
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "examples", "level_pipeline")
pytestmark = pytest.mark.gpu


def build():
    if not os.access(EXE, os.X_OK):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def run(args):
    build()
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PIPELINE OK" in r.stdout
    return r.stdout


@pytest.mark.parametrize("extra", [[], ["--mesh"], ["--masked"], ["--mesh", "--masked"]], ids=["cloud", "mesh", "cloud-masked", "mesh-masked"])
@pytest.mark.parametrize("color, name", [(None, "GRAY"), ("rgb", "RGB")])
def test_reduced_pipeline_recovers_planted_offset(color, name, extra):
    out = run(["4", "--reduce", "2", *(["--color", color] if color else []), *extra])
    if color:
        assert f"full-size colour frame: {name}, 1696 x 960 in rows of" in out
    else:
        assert "full-size frame: GRAY, 1696 x 960, reduced 2x to 848 x 480" in out


def test_larger_factor_in_four_channels():
    out = run(["2", "--reduce", "4", "--color", "bgra"])
    assert "full-size colour frame: BGRA, 3392 x 1920 in rows of" in out


def test_full_size_settings_file_goes_through_config_reduce(tmp_path):
    build()
    subprocess.check_call([EXE, "--reduce", "2", "--write-files", str(tmp_path)], stdout=subprocess.DEVNULL)
    text = (tmp_path / "settings.yaml").read_text()
    assert "Camera.Width: 1696" in text and "Camera.Height: 960" in text and "NMI.Render.PointSize: 6.0" in text
    out = run(["2", "--files", str(tmp_path), "--reduce", "2"])
    assert "full-size frame: GRAY, 1696 x 960" in out
    # read without --reduce the file is a camera of another size than the program searches at
    r = subprocess.run([EXE, "2", "--files", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "1696 x 960" in r.stderr
