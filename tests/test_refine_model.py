"""CPU tests of the refined-peaks rule (include/nmi_hip.h, "Refined peaks"): the numpy model (tests/helpers/refine_np.py) against
literal answers on hand-written tables; the host twin nmi_refine_peaks_host (include/nmi_host.h) == the float32 model on every
bit of every record of the case list; the accuracy of the rule on planted quadratics; the pose of a real-valued cell and the
covariance of a record; and the host functions under ASan / UBSan in a stand-alone program (tests/native/refine_peaks.cpp)."""
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from helpers import peaks_np as pk
from helpers import refine_np as rf
from orbslam2_nmi_amd import build as nmi_build
from orbslam2_nmi_amd import capi, hostapi as H

f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _built():
    nmi_build.build()


def key(table, index):
    return pk.keys_of(np.asarray(table, f32))[index]


def one(table, num, index, dtype=np.float64):
    """The model's record for the cell `index` of a hand-written table, and the host twin's == the float32 model's on the way."""
    table = np.asarray(table, f32)
    keys = [key(table, index)]
    want32 = rf.refine(table, num, keys, f32)
    assert rf.same_bytes(H.refine_peaks(table, num, keys), want32), rf.explain(H.refine_peaks(table, num, keys), want32)
    return rf.refine(table, num, keys, dtype)[0]


def test_the_models_record_is_the_librarys():
    assert capi.REFINED_PEAK == rf.record_dtype(f32) and capi.REFINED_PEAK.itemsize == 152
    assert (capi.REFINE_EMPTY, capi.REFINE_NONFINITE, capi.REFINE_COUPLED, capi.REFINE_CROSS_HOLE) == (rf.EMPTY, rf.NONFINITE, rf.COUPLED, rf.CROSS_HOLE)
    for a in range(6):
        assert (capi.refine_border(a), capi.refine_hole(a), capi.refine_flat(a)) == (rf.BORDER(a), rf.HOLE(a), rf.FLAT(a))


# ---- literal answers ---------------------------------------------------------------------------------------------------------
def test_a_parabola_in_one_dimension():
    """0.9 - 0.01 (x - 1.25)^2 on three cells: offset 0.25, score 0.9, g = 0.005, H = -0.02."""
    num = (3, 1, 1, 1, 1, 1)
    t = [0.9 - 0.01 * (x - 1.25) ** 2 for x in range(3)]
    r = one(t, num, 1)
    assert r["flags"] == rf.COUPLED
    assert abs(r["offset"][0] - 0.25) < 1e-5 and abs(r["score"] - 0.9) < 1e-7 and not r["offset"][1:].any()
    # (the table is fp32: each sample is within half an ulp of 0.9, 3e-8, of the parabola)
    assert abs(r["gradient"][0] - 0.005) < 6e-8 and abs(r["hessian"][0] + 0.02) < 2.4e-7 and not r["hessian"][1:].any()
    # the float64 table gives them to rounding
    exact = rf.refine(np.array(t), num, [key(t, 1)], np.float64)[0]
    assert abs(exact["offset"][0] - 0.25) < 1e-13 and abs(exact["score"] - 0.9) < 1e-15


def test_a_cross_term_moves_the_coupled_offset_away_from_the_separable_one():
    """f = 1 - (2 u^2 + 2 u v + 2 v^2) / 100 with u = x - 1.2, v = y - 1: H = [[-.04, -.02], [-.02, -.04]], g at the centre cell
    = (0.008, 0.004).  Coupled: -H^-1 g = (0.2, 0), the planted maximum.  Separable: (-g_x / H_xx, -g_y / H_yy) = (0.2, 0.1)."""
    num = (3, 3, 1, 1, 1, 1)
    t = np.array([[1 - (2 * (x - 1.2) ** 2 + 2 * (x - 1.2) * (y - 1) + 2 * (y - 1) ** 2) / 100 for x in range(3)] for y in range(3)])
    r = one(t, num, 4)
    assert r["flags"] == rf.COUPLED
    assert np.allclose(r["offset"][:2], [0.2, 0.0], atol=1e-5) and abs(r["score"] - 1.0) < 1e-6
    assert np.allclose(r["gradient"][:2], [0.008, 0.004], atol=1e-7)
    assert np.allclose(rf.hessian_matrix(r)[:2, :2], [[-0.04, -0.02], [-0.02, -0.04]], atol=1e-6)
    separable = -r["gradient"][:2] / np.diag(rf.hessian_matrix(r))[:2]
    assert np.allclose(separable, [0.2, 0.1], atol=1e-5) and abs(separable[1] - r["offset"][1]) > 0.09
    # a NaN corner: the cross term goes, the other terms stay, and the step is the separable one exactly
    hole = t.copy()
    hole[0, 0] = np.nan
    h = one(hole, num, 4)
    assert h["flags"] == rf.COUPLED | rf.CROSS_HOLE and h["hessian"][1] == 0
    assert (h["gradient"] == r["gradient"]).all() and h["hessian"][0] == r["hessian"][0] and h["hessian"][6] == r["hessian"][6]
    assert np.allclose(h["offset"][:2], [0.2, 0.1], atol=1e-5)
    # a saddle is not a maximum: -H has a negative pivot, and each axis goes on its own
    saddle = np.array([[0.5 + 0.1 * (x - 1) * (y - 1) - 0.01 * ((x - 1) ** 2 + (y - 1) ** 2) for x in range(3)] for y in range(3)])
    s = one(saddle, num, 4)
    assert s["flags"] == 0 and not s["offset"].any() and abs(s["hessian"][1] - 0.1) < 1e-6 and s["hessian"][0] < 0


def test_an_all_equal_table_is_flat():
    num = (3, 3, 3, 3, 3, 3)
    r = one(np.full(729, 0.5), num, rf.CENTRE_KEY_INDEX)
    assert r["flags"] == sum(rf.FLAT(a) for a in range(6)) and not r["offset"].any() and r["score"] == 0.5
    assert not r["gradient"].any() and not r["hessian"].any()
    num = (5, 1, 3, 1, 1, 2)     # axes of one cell carry no flag; axis 5 has two cells: every cell is on its border
    r = one(np.full(30, 0.5), num, pk.linear(num, (2, 0, 1, 0, 0, 1)))
    assert r["flags"] == rf.FLAT(0) | rf.FLAT(2) | rf.BORDER(5) and r["score"] == 0.5


def test_a_peak_on_a_corner_is_border_on_every_axis():
    num = (3, 3, 3, 1, 4, 2)
    t = pk.table(num, "corners")
    for cell in pk.corner_cells(num):
        r = one(t, num, cell)
        assert r["flags"] == sum(rf.BORDER(a) for a in range(6) if num[a] >= 2) and r["score"] == 1.5 and not r["offset"].any()


def test_holes_and_an_infinite_peak():
    num = (3, 3, 1, 1, 1, 1)
    t = np.array([0.10, 0.20, 0.12,
                  0.30, 0.90, 0.40,
                  0.14, 0.25, 0.16])
    whole = one(t, num, 4)
    assert int(whole["flags"]) & ~rf.COUPLED == 0
    for bad in (np.nan, -0.5, np.inf, -np.inf):
        hole = t.copy()
        hole[3] = bad       # the neighbour at -1 on axis 0
        r = one(hole, num, 4)
        assert int(r["flags"]) & ~rf.COUPLED == rf.HOLE(0) and r["offset"][0] == 0 and r["gradient"][0] == 0 and r["hessian"][0] == 0
        assert r["gradient"][1] == whole["gradient"][1] and r["hessian"][6] == whole["hessian"][6] and r["hessian"][1] == 0
    minus_zero = t.copy()
    minus_zero[3] = -0.0    # usable
    assert one(minus_zero, num, 4)["flags"] & rf.HOLE(0) == 0
    inf = t.copy()
    inf[4] = np.inf
    r = one(inf, num, 4)
    assert r["flags"] == rf.NONFINITE and r["score"] == np.inf and not r["offset"].any() and not r["hessian"].any() and not r["gradient"].any()
    assert r["key"] == key(inf, 4)


def test_samples_near_the_top_of_fp32_keep_the_offsets_in_range():
    """Usable samples near 3.4e38: sums of differences overflow to +-inf.  The offsets stay finite and within [-1, 1] (the header's
    "Overflow"), in the model and in the host twin alike, on the coupled and on the separable path; the score may be NaN."""
    big = 3.0e38
    tables = [((3, 1, 1, 1, 1, 1), 1, [big, 3.4e38, 0.0]),                      # H = -inf, coupled
              ((3, 1, 1, 1, 1, 1), 1, [big, 1.0, big]),                          # H = +inf: flat
              ((3, 3, 1, 1, 1, 1), 4, [big, 0, 0, 0, 1.0, 0, 0, 0, big]),        # the cross term overflows
              ((3, 3, 1, 1, 1, 1), 4, [0, big, 0, big, 3.4e38, 0, 0, 0, 0])]
    for num, cell, t in tables:
        t = np.asarray(t, f32)
        keys = [key(t, cell)]
        model, twin = rf.refine(t, num, keys, f32)[0], H.refine_peaks(t, num, keys)[0]
        for r in (model, twin):
            assert np.isfinite(r["offset"]).all() and (np.abs(r["offset"]) <= 1).all(), (t, r)
        assert (model["offset"] == twin["offset"]).all() and model["flags"] == twin["flags"]
        assert not np.isfinite(model["hessian"]).all()      # (the case does overflow)


def test_keys_that_name_no_cell_give_the_empty_record():
    num = (3, 1, 1, 1, 1, 1)
    t = np.array([0.1, 0.9, 0.2], f32)
    keys = np.array([0, capi.key_pack(0.9, 3), capi.key_pack(0.9, 2 ** 32 - 2), capi.key_pack(0.9, 1)], np.uint64)
    for got in (rf.refine(t, num, keys, f32), H.refine_peaks(t, num, keys)):
        empty = np.zeros(1, capi.REFINED_PEAK)
        empty["flags"] = rf.EMPTY
        for k in range(3):
            assert got[k].tobytes() == empty.tobytes()
        assert got[3]["key"] == keys[3] and got[3]["flags"] == rf.COUPLED


def test_a_row_end_is_not_crossed():
    """(4, 3): the peak at sx = 3 of row 0 (index 3).  sx = 0 of row 1 (index 4) is its linear neighbour and no neighbour of the
    rule's: a huge value planted there moves nothing.  The same for the peak at sx = 0 of row 1 and index 3."""
    num = (4, 3, 1, 1, 1, 1)
    t = np.linspace(0.1, 0.2, 12).astype(f32)
    for peak, beside in ((3, 4), (4, 3)):
        a = t.copy()
        a[peak] = 0.9
        b = a.copy()
        b[beside] = 1e30
        keys = [key(a, peak)]
        ra, rb = H.refine_peaks(a, num, keys), H.refine_peaks(b, num, keys)
        assert rf.same_bytes(ra, rb) and rf.same_bytes(ra, rf.refine(a, num, keys, f32)) and rf.same_bytes(rb, rf.refine(b, num, keys, f32))
        assert ra[0]["flags"] & rf.BORDER(0) and ra[0]["offset"][0] == 0


# ---- the host twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num", rf.SHAPES, ids=pk.shape_id)
def test_host_twin_equals_the_model(num):
    coupled = separable = 0
    for content in rf.CONTENTS:
        t = rf.table(num, content)
        for radius in rf.RADII:
            keys, want = rf.keys_of(num, content, radius), rf.refined(num, content, radius)
            for K in rf.KS:
                got = H.refine_peaks(t, num, keys[:K])
                assert rf.same_bytes(got, want[:K]), (content, radius, K, rf.explain(got, want[:K]))
            live = want[want["key"] != 0]
            assert np.isfinite(live["offset"]).all() and (np.abs(live["offset"]) <= 1).all(), (content, radius)
            coupled += int((live["flags"] & rf.COUPLED != 0).sum())
            separable += int((live["flags"] & (rf.COUPLED | rf.NONFINITE) == 0).sum())
    if all(n >= 3 for n in num):   # the case list takes both branches
        assert coupled > 0 and separable > 0


def test_host_twin_refuses():
    t = np.ones(3, f32)
    for num, keys in [((3, 1, 1, 1, 1, 0), [1]), ((3, 1, 1, 1, 1, 1), []), ((3, 1, 1, 1, 1, 1), [1] * 65)]:
        with pytest.raises(ValueError):
            H.refine_peaks(t if 0 not in num else np.ones(0, f32), num, keys)


# ---- accuracy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("magnitude", sorted(rf.MAGNITUDES))
def test_accuracy(magnitude):
    """Planted quadratics: float64 recovers the planted offset; the float32 model takes the coupled step on every kept case and
    stays within the recorded tolerance of the float64 model on the same float32 table."""
    cases = [c for seed in rf.CPU_SEEDS for c in rf.planted(seed, magnitude)]
    kept = worst_offset = worst_score = 0
    for t64, offset, A in cases:
        k = rf.kept(t64)
        if k is None:
            continue
        kept += 1
        t32, m64 = k
        keys = [rf.centre_key(t32)]
        exact = rf.refine(t64, rf.NUM3, keys, np.float64)[0]
        assert np.abs(exact["offset"] - offset).max() < 1e-12
        assert np.allclose(rf.hessian_matrix(exact), -2 * A, rtol=0, atol=1e-12)
        m32 = rf.refine(t32, rf.NUM3, keys, f32)[0]
        assert m32["flags"] == rf.COUPLED
        worst_offset = max(worst_offset, np.abs(m32["offset"].astype(np.float64) - m64["offset"]).max())
        worst_score = max(worst_score, abs(float(m32["score"]) - m64["score"]))
        # the covariance of the record is (-H)^-1 in the steps' units
        step = [0.2, 0.2, 0.5, 0.02, 0.02, 0.05]
        cov, mask = H.refined_covariance(m32, step)
        s = np.asarray(step, f32).astype(np.float64)     # the steps are fp32, the product is not
        want = np.linalg.inv(-rf.hessian_matrix(m32).astype(np.float64)) * np.outer(s, s)
        assert mask == 63 and np.allclose(cov, want, rtol=1e-9, atol=1e-10 * np.abs(want).max())
    print(f"{magnitude}: kept {kept} of {len(cases)}, float32 against float64: offset {worst_offset:.3g} cells, score {worst_score:.3g}")
    assert kept >= 0.9 * len(cases)
    assert worst_offset <= rf.OFFSET_TOLERANCE and worst_score <= rf.SCORE_TOLERANCE


# ---- pose and covariance ---------------------------------------------------------------------------------------------------------
def test_a_zero_offset_is_the_whole_cells_pose():
    from test_host_driver import model_relocalization, random_pose
    rng = np.random.default_rng(0)
    for _ in range(50):
        Twc = random_pose(rng)
        num = [int(rng.integers(1, 6)) for _ in range(6)]
        step = [rng.uniform(0.01, 0.5) for _ in range(3)] + [rng.uniform(0.001, 0.05) for _ in range(3)]
        best = [int(rng.integers(0, n)) for n in num]
        k = H.SearchKernel.make(num, step, best=best)
        whole = H.calculate_relocalization(Twc, k)
        for zero in (np.zeros(6), -np.zeros(6)):
            got = H.calculate_relocalization_offset(Twc, k, zero)
            assert (got.view(np.uint32) == whole.view(np.uint32)).all()
        # a real offset against the float64 model of the real-valued cell
        offset = rng.uniform(-1, 1, 6).astype(f32)
        real = types.SimpleNamespace(num=list(k.num), step=list(k.step), best=[b + float(o) for b, o in zip(best, offset)])
        got = H.calculate_relocalization_offset(Twc, k, offset)
        assert np.allclose(got, model_relocalization(Twc.astype(f32).astype(float), real), atol=5e-5)


def test_the_pose_is_linear_and_monotone_in_a_translation_offset():
    """The identity pose, offsets on axis 1 only (dir_y = the pose's second column): the pose moves by offset * step along y and
    by nothing else, in order."""
    k = H.SearchKernel.make([3] * 6, [0.2, 0.3, 0.5, 0.02, 0.03, 0.05], best=[1, 2, 0, 1, 1, 1])
    whole = H.calculate_relocalization(np.eye(4), k)
    before = None
    for o in np.linspace(-1, 1, 21):
        got = H.calculate_relocalization_offset(np.eye(4), k, [0, o, 0, 0, 0, 0])
        assert abs(got[1, 3] - whole[1, 3] - 0.3 * o) < 1e-6
        moved = got.copy()
        moved[1, 3] = whole[1, 3]
        assert np.allclose(moved, whole, atol=1e-7)
        assert before is None or got[1, 3] > before
        before = got[1, 3]
    # a rotation offset: half a cell on warp axis z turns the pose by half a step about z
    got = H.calculate_relocalization_offset(np.eye(4), k, [0, 0, 0, 0, 0, 0.5])
    assert abs(np.arctan2(got[1, 0], got[0, 0]) - 0.5 * 0.05) < 1e-6


def test_covariance_needs_a_coupled_record():
    num = (3, 3, 1, 1, 1, 1)
    saddle = np.array([[0.5 + 0.1 * (x - 1) * (y - 1) - 0.01 * ((x - 1) ** 2 + (y - 1) ** 2) for x in range(3)] for y in range(3)], f32)
    rec = H.refine_peaks(saddle, num, [key(saddle, 4)])[0]
    assert rec["flags"] & rf.COUPLED == 0 and H.refined_covariance(rec, [0.1] * 6) is None
    empty = H.refine_peaks(saddle, num, [0])[0]
    assert H.refined_covariance(empty, [0.1] * 6) is None
    # two active axes of six: zero rows and columns for the others, and the mask says which
    t = np.array([[1 - (2 * (x - 1.2) ** 2 + 2 * (x - 1.2) * (y - 1) + 2 * (y - 1) ** 2) / 100 for x in range(3)] for y in range(3)], f32)
    rec = H.refine_peaks(t, num, [key(t, 4)])[0]
    cov, mask = H.refined_covariance(rec, [0.5, 0.25, 1, 1, 1, 1])
    want = np.linalg.inv(-rf.hessian_matrix(rec)[:2, :2].astype(np.float64)) * np.outer([0.5, 0.25], [0.5, 0.25])
    assert mask == 3 and np.allclose(cov[:2, :2], want, rtol=1e-12) and not cov[2:].any() and not cov[:, 2:].any()


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------
def test_refine_peaks_under_asan_ubsan(tmp_path):
    exe = tmp_path / "refine_peaks"
    host = os.path.join(ROOT, "orbslam2_nmi_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + host,
                           os.path.join(ROOT, "tests", "native", "refine_peaks.cpp"),
                           os.path.join(host, "nmi_refine_host.cpp"), os.path.join(host, "nmi_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refine peaks ok" in r.stdout
