"""examples/level_pipeline.cpp --files with a fisheye settings file (-m gpu): Camera.type "KannalaBrandt8" and Camera.k1 .. k4
make the camera's frame a fisheye one and set nmi_level_set_distortion_fisheye on the level, which still recovers the planted
offset; a settings file without the key runs as before."""
import os
import subprocess

import pytest

from test_color_demo import EXE, run

pytestmark = pytest.mark.gpu

KB8 = 'Camera.type: "KannalaBrandt8"\nCamera.k1: -0.01372\nCamera.k2: -0.02073\nCamera.k3: 0.03443\nCamera.k4: -0.01995\n'


@pytest.mark.parametrize("mode", [[], ["--masked"]], ids=["plain", "masked"])
def test_fisheye_settings_file_runs_a_fisheye_level(tmp_path, mode):
    if not os.access(EXE, os.X_OK):
        subprocess.check_call(["make", "-C", os.path.dirname(EXE)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.check_call([EXE, "--write-files", str(tmp_path)], stdout=subprocess.DEVNULL)
    if not mode:
        assert "fisheye lens" not in run(["1", "--files", str(tmp_path)])   # no Camera.type: as before
    with open(os.path.join(tmp_path, "settings.yaml"), "a") as f:
        f.write(KB8)
    out = run(["2", "--files", str(tmp_path)] + mode)
    assert "fisheye lens: k1 -0.01372 k2 -0.02073 k3 0.03443 k4 -0.01995" in out
