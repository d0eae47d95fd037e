"""GPU tests (-m gpu) of the data-dependent tone maps (PERCENTILE, EQUALIZE; csrc/nmi_tone.hip) on planted histograms
(tests/helpers/tone_cases.py; their premises: tests/test_tone_cases_plan.py): running sums that sit exactly on, one below and
one above the two ranks at lane, wave and segment edges, extents at the ends of the range and of the segments, plateaus at the
counts themselves, quotients that are exact halves or whose fp64 first guess is one short, and frames confined to single
quarters of the histogram kernel's range.  Every comparison is == with the numpy twin: all 65,536 entries of nmi_tone_lut's
table, its {lo, hi} pair, and nmi_gray_frame == table[pixels].  A group of cases shares one context, so every case runs on
what the case before it left behind (the histogram, its copy, the records), first dense and then again with pitched rows at
an offset.

What no frame can decide, so that these tests do not claim it: `e > k_lo` against `e >= k_lo` over the segments (the extra match
is a lower lane of the same wave storing to the same LDS word, and the higher lane's store stands on this hardware); `v < lo`
against `v <= lo` (c'[vmin] == c0 makes entry vmin 0 either way); the `seg_sum != 0` guard (an empty segment has b == e, which
neither conjunction admits); the first-level record test (an empty record loses every min and max); and floor_div's `--q` line
(the product is never above the floor for these denominators: tests/test_tone_cases_plan.py)."""
import numpy as np
import pytest

from helpers import reduce_np as rnp
from helpers import tone_cases as tc
from helpers import tone_np as tnp
from orbslam2_nmi_amd import capi
from test_color_level import scene
from test_color_stream import outcome, same
from test_masked_level import views, warps
from test_stream_masked import level, pin
from test_tone_pipeline import replay, same_replay

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H, S, WN = 64, 48, 3, 3     # the level's and the stream's frame


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_case(ctx, c, seed):
    w, h = ctx.width, ctx.height
    px = c.frame(w, h, seed)
    want_lut, want_pair = c.twin()
    want = want_lut[px]
    ctx.set_tone_map(tnp.capi_tone(capi, c.tm))
    for pitch, off in ((0, 0), (2 * w + 10, 2)):       # (the second round also shows the histogram was left clean)
        d = dev(tnp.pack16(px, pitch, off, seed=seed))
        lut, pair = ctx.tone_lut(d[off:], 1, pitch)
        assert pair == want_pair, (c, pitch, pair, want_pair)
        got = lut.cpu().numpy()
        assert (got == want_lut).all(), (c, pitch, np.flatnonzero(got != want_lut)[:5], got[got != want_lut][:5], want_lut[got != want_lut][:5])
        out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
        ctx.gray_frame(d[off:], capi.FRAME_GRAY16, pitch, out=out)
        assert (out.cpu().numpy() == want).all(), (c, pitch)


@pytest.mark.parametrize("group", list(tc.groups()))
def test_planted_histograms_equal_the_twin(nmi, group):
    (w, h), cases = tc.groups()[group]
    with nmi.NmiContext(w, h) as ctx:
        for k, c in enumerate(cases):
            check_case(ctx, c, k)
        check_case(ctx, cases[0], 0)                   # the first again, after all the others


@pytest.mark.parametrize("f", [2, 3])
def test_reduced_planted_frames_equal_the_twin(nmi, f):
    """nmi_reduce_frame takes its statistics from the f W x f H source: N = f^2 * 4,096 planted pixels."""
    w, h = tc.SMALL
    pitch, off = 2 * f * w + 6, 2
    with nmi.NmiContext(w, h) as ctx:
        for k, c in enumerate(x for pair in tc.one_per_family(f * f * w * h) for x in pair):
            px = c.frame(f * w, f * h, k)
            want_lut, want_pair = c.twin()
            d = dev(tnp.pack16(px, pitch, off, seed=k))
            ctx.set_tone_map(tnp.capi_tone(capi, c.tm))
            out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
            ctx.reduce_frame(d[off:], capi.FRAME_GRAY16, f, pitch, out=out)
            assert (out.cpu().numpy() == rnp.reduce_gray(want_lut[px], f)).all(), c
            lut, pair = ctx.tone_lut(d[off:], f, pitch)
            assert pair == want_pair and (lut.cpu().numpy() == want_lut).all(), c


def test_a_level_alternating_planted_frames(nmi):
    """A captured level fed, in place, two planted frames in turn whose lo / hi lie in other segments: the histogram, the
    records and the crossings are rebuilt at every replay.  The baseline is the same level on the twin's 8-bit frame."""
    with nmi.NmiContext(W, H) as ctx:
        sc = scene(nmi, ctx, W, H, False, "plain")
        d = dev(np.zeros(2 * W * H, np.uint8))
        twin_frame = dev(np.zeros((H, W), np.uint8))
        mvps, Ms = views(sc.rp, S), warps(W, H, WN)
        with nmi.NmiLevel(ctx, sc.dx, sc.da, d, S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, twin_frame, S, WN, 3.0) as base:
            lv.set_frame_format(capi.FRAME_GRAY16, 2 * W)
            for a, b in tc.one_per_family(W * H):
                assert (a.twin()[0] != b.twin()[0]).any(), (a, b)
                tm = None
                for k, c in enumerate((a, b, a, b)):
                    if c.tm != tm:                                 # (most pairs share one setting: no new capture between them)
                        tm = c.tm
                        lv.set_tone_map(tnp.capi_tone(capi, tm))
                    px = c.frame(W, H, k)
                    twin = c.twin()[0][px]
                    d.copy_(dev(tnp.pack16(px)))
                    twin_frame.copy_(dev(twin))
                    torch.cuda.synchronize()
                    got = replay(lv, mvps, Ms)
                    same_replay(got, replay(base, mvps, Ms))


def test_a_stream_alternating_planted_frames(nmi):
    frames = [level(W, H, (3, 1, 1), (3, 1, 1), seed=s) for s in (5, 9)]
    Ms = frames[0][2]
    pitch = 2 * W + 6
    with nmi.NmiContext(W, H) as ctx, nmi.NmiStream(ctx, S, WN, depth=4) as st, nmi.NmiStream(ctx, S, WN, depth=4) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        st.set_frame_format(capi.FRAME_GRAY16, pitch)
        for a, b in tc.one_per_family(W * H):
            tickets = []
            for k, c in enumerate((a, b, a)):
                st.set_tone_map(tnp.capi_tone(capi, c.tm))
                px = c.frame(W, H, k)
                rs = frames[k % 2][1]
                t = st.submit(pin(rs), pin(tnp.pack16(px, pitch, seed=k)), Ms)
                r = ref.submit(pin(rs), pin(c.twin()[0][px]), Ms)
                tickets.append((t, r))
            for t, r in tickets:
                same(outcome(st, t, WN, S, "plain"), outcome(ref, r, WN, S, "plain"))
