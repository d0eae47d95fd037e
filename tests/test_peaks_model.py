"""CPU tests of the ranked-peaks rule (include/nmi_hip.h, "Ranked peaks"): the numpy model (tests/helpers/peaks_np.py) against
literal answers on hand-written tables, the host twin nmi_find_peaks (include/nmi_host.h) == the model on every case of the case
list, with == on every key, and nmi_find_peaks under ASan / UBSan in a stand-alone program (tests/native/find_peaks.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import peaks_np as pk
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi, hostapi as H


@pytest.fixture(scope="module", autouse=True)
def _built():
    nmi_build.build()


def key(score, index):
    return np.uint64(capi.key_pack(float(np.float32(score)), int(index)))


def keys_list(pairs, K):
    return [key(s, i) for s, i in pairs] + [np.uint64(0)] * (K - len(pairs))


def test_model_keys_are_nmi_key_pack():
    t = np.array([0.0, -0.0, 0.5, -1e-9, np.nan, np.inf, 2.0, -np.inf, 1e-45], np.float32)
    assert pk.keys_of(t).tolist() == [capi.key_pack(float(v), i) for i, v in enumerate(t)]


def test_two_maxima_one_cell_apart():
    """3 x 3: 0.9 in the centre, 0.8 right of it, 0.1 .. elsewhere.  Radius 0: a plain top-K, both are peaks; radius 1: the
    centre's box is the whole table."""
    num = (3, 3, 1, 1, 1, 1)
    t = np.array([0.10, 0.11, 0.12,
                  0.13, 0.90, 0.80,
                  0.14, 0.15, 0.16], np.float32)
    got = pk.find_peaks(t, num, 4, (0,) * 6)
    assert got[0].tolist() == keys_list([(0.90, 4), (0.80, 5), (0.16, 8), (0.15, 7)], 4) and got[1] == 4
    got = pk.find_peaks(t, num, 4, (1,) * 6)
    assert got[0].tolist() == keys_list([(0.90, 4)], 4) and got[1] == 1
    # radius 1 on axis 0 only: the centre takes its row; 0.16 takes 0.15 with it, 0.14 is two steps from it; 0.12 takes 0.11
    got = pk.find_peaks(t, num, 5, (1, 0, 0, 0, 0, 0))
    assert got[0].tolist() == keys_list([(0.90, 4), (0.16, 8), (0.14, 6), (0.12, 2), (0.10, 0)], 5) and got[1] == 5
    got = pk.find_peaks(t, num, 6, (1, 0, 0, 0, 0, 0))
    assert got[0].tolist() == keys_list([(0.90, 4), (0.16, 8), (0.14, 6), (0.12, 2), (0.10, 0)], 6) and got[1] == 5


def test_row_end_neighbours_are_not_box_neighbours():
    """4 x 3: the cell at sx = 3 of row 0 and the cell at sx = 0 of row 1 are linear neighbours (3, 4) and two steps apart on
    axis 0: at radius (1, 0, ...) both are peaks.  At radius 1 on both axes the second is inside the first's box on axis 1 but
    not on axis 0: still both."""
    num = (4, 3, 1, 1, 1, 1)
    t = np.full(12, 0.1, np.float32)
    t[3], t[4] = 0.9, 0.8
    for radius in ((1, 0, 0, 0, 0, 0), (1,) * 6):
        keys, count = pk.find_peaks(t, num, 2, radius)
        assert keys.tolist() == keys_list([(0.9, 3), (0.8, 4)], 2) and count == 2, radius


def test_all_equal_table_gives_the_lattice():
    """Equal scores: the lowest index wins, so the peaks are the lattice of stride radius + 1 from index 0, in index order."""
    num = (5, 4, 1, 3, 1, 2)
    radius = (1, 2, 0, 1, 5, 0)
    t = np.full(int(np.prod(num)), 0.5, np.float32)
    at = pk.coordinates(num)
    on = np.all([at[a] % (radius[a] + 1) == 0 for a in range(6)], axis=0)
    want = np.flatnonzero(on)
    assert want.size == 3 * 2 * 1 * 2 * 1 * 2
    keys, count = pk.find_peaks(t, num, 64, radius)
    assert count == want.size and keys.tolist() == keys_list([(0.5, i) for i in want], 64)


@pytest.mark.parametrize("content", ["random", "equal", "zeros", "holes", "negative", "nan"])
def test_k1_is_the_first_tie_of_find_max_elements(content):
    for num in pk.SHAPES[:9]:
        t = pk.table(num, content)
        ties, n, mx = H.find_max_elements(t, cap=1)
        keys, count = pk.find_peaks(t, num, 1, (1,) * 6)
        got, host_count = H.find_peaks(t, num, 1, (1,) * 6)
        assert got.tolist() == keys.tolist() and host_count == count
        if n == 0:   # every cell negative or NaN
            assert count == 0 and keys[0] == 0
        else:
            assert count == 1 and capi.key_unpack(int(keys[0])) == (ties[0], mx)


@pytest.mark.parametrize("num", pk.SHAPES[:9], ids=pk.shape_id)
def test_radius_zero_is_the_keys_sorted(num):
    for content in pk.CONTENTS:
        allkeys = np.sort(pk.keys_of(pk.table(num, content)))[::-1]
        allkeys = allkeys[allkeys != 0][:pk.MAX_K]
        keys, count = pk.ranked(num, content, (0,) * 6)
        assert count == allkeys.size and keys[:count].tolist() == allkeys.tolist() and not keys[count:].any(), content


@pytest.mark.parametrize("num", pk.SHAPES, ids=pk.shape_id)
def test_host_twin_equals_the_model(num):
    for content, radius, K in pk.cases(num):
        want = pk.prefix(pk.ranked(num, content, radius), K)
        keys, count = H.find_peaks(pk.table(num, content), num, K, radius)
        assert count == want[1] and keys.tolist() == want[0].tolist(), (content, radius, K)


def test_model_prefixes_are_the_smaller_k():
    """What prefix() relies on: peak j does not depend on K."""
    num = (3, 3, 3, 3, 3, 3)
    for content in ("random", "holes", "corners"):
        for radius in pk.RADII:
            for K in (1, 2, 63):
                want = pk.find_peaks(pk.table(num, content), num, K, radius)
                got = pk.prefix(pk.ranked(num, content, radius), K)
                assert got[1] == want[1] and got[0].tolist() == want[0].tolist()


def test_host_twin_refuses():
    t = np.ones(3, np.float32)
    for num, K, radius in [((3, 1, 1, 1, 1, 0), 1, (0,) * 6), ((3, 1, 1, 1, 1, 1), 0, (0,) * 6), ((3, 1, 1, 1, 1, 1), 65, (0,) * 6),
                           ((3, 1, 1, 1, 1, 1), 1, (0, 0, 0, -1, 0, 0))]:
        with pytest.raises(ValueError):
            H.find_peaks(t if 0 not in num else np.ones(0, np.float32), num, K, radius)


def test_find_peaks_under_asan_ubsan(tmp_path):
    exe = tmp_path / "find_peaks"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "find_peaks.cpp"),
                           os.path.join(ROOT, "orbslam2_nmi_amd", "host", "nmi_peaks_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "find peaks ok" in r.stdout
