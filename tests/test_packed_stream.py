"""GPU tests (-m gpu) of keyframe streams fed the deep raw formats (NMI_FRAME_MONO12P, _RAW10, _BAYER16_GRBG through
nmi_stream_set_frame_format / _set_frame_reduction): host frames cross as their packed rows, and every ticket equals, bit for
bit, the ticket of a stream fed NMI_FRAME_GRAY16 with the model's container (tests/helpers/packed_np.py) -- at 64x48 and 52x38,
S = 3, Wn = 3, factor 1 and 2, with and without a lens, under SHIFT and EQUALIZE, two frames in flight; and a wider format after
a narrower one on the same stream (the frame slots grow)."""
import numpy as np
import pytest

from helpers import packed_np as pnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import capi
from orbslam2_nmi_amd import synthetic as sy
from test_color_stream import outcome, same
from test_packed_level import FORMATS, deep, tone_maps
from test_reduce_level import full_size
from test_stream_masked import level, pin

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

S, WN = 3, 3
LENS = unp.FAMILIES["barrel"]


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def host_frames(F, fmt, f, seed):
    """-> (the host frame in fmt with a pitch beyond the dense one, that pitch, the model's container as a dense GRAY16 host frame)."""
    h, w = F.shape
    px = deep(F if f == 1 else full_size(F, f, seed), fmt, seed)
    pitch = pnp.row_bytes(fmt, f * w) + (2 if pnp.GROUP[fmt][1] == 2 else 3)
    buf = pnp.frame(px, fmt, pitch, 0, seed)
    cont = pnp.container(buf, fmt, f * w, f * h, pitch)
    return buf, pitch, np.ascontiguousarray(cont, "<u2").view(np.uint8).reshape(-1)


@pytest.mark.parametrize("size", [(64, 48), (52, 38)], ids=["64x48", "52x38"])
@pytest.mark.parametrize("name", list(FORMATS))
def test_packed_tickets_equal_gray16_tickets(nmi, name, size):
    w, h = size
    fmt = FORMATS[name]
    frames = [level(w, h, (3, 1, 1), (3, 1, 1), seed=s) for s in (5, 9)]
    Ms = frames[0][2]
    K = sy.intrinsics(w, h)
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, S, WN, depth=4) as st, nmi.NmiStream(ctx, S, WN, depth=4) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        seen = []
        for f in (1, 2):
            for lens in (None, LENS):
                st.set_distortion(K, lens)
                ref.set_distortion(K, lens)
                for tm in tone_maps(fmt).values():
                    st.set_tone_map(tm)
                    ref.set_tone_map(tm)
                    pairs = []
                    for k, (F, rs, _) in enumerate(frames):             # two frames in flight on each stream
                        buf, pitch, cont = host_frames(F, fmt, f, seed=k + 1)
                        st.set_frame_reduction(f, fmt, pitch)
                        ref.set_frame_reduction(f, capi.FRAME_GRAY16, 0)
                        pairs.append((st.submit(pin(rs), pin(buf), Ms), ref.submit(pin(rs), pin(cont), Ms)))
                    for t, r in pairs:
                        got = outcome(st, t, WN, S, "plain")
                        same(got, outcome(ref, r, WN, S, "plain"))
                        seen.append(got[1].view(np.uint32).copy())
        assert (seen[0] != seen[2]).any()                                # SHIFT and EQUALIZE are different frames


def test_a_wider_format_after_a_narrower_one(nmi):
    """MONO12P at factor 1 (1.5 bytes per pixel), BAYER16 at factor 2 (8 per search pixel), RAW10 at factor 1 again, dense grey
    last: the frame slots grow once and every ticket, two in flight, is the GRAY16 stream's."""
    w, h = 64, 48
    frames = [level(w, h, (3, 1, 1), (3, 1, 1), seed=s) for s in (3, 7)]
    Ms = frames[0][2]
    tm = capi.ToneMap.equalize(0, 16)
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, S, WN, depth=2) as st, nmi.NmiStream(ctx, S, WN, depth=2) as ref:
        st.keep_ratings()
        ref.keep_ratings()
        st.set_tone_map(tm)
        ref.set_tone_map(tm)
        for fmt, f in ((pnp.MONO12P, 1), (pnp.BAYER16["grbg"], 2), (pnp.RAW10, 1)):
            pairs = []
            for k, (F, rs, _) in enumerate(frames):
                buf, pitch, cont = host_frames(F, fmt, f, seed=10 + k)
                assert buf.size == pnp.span(fmt, f * w, f * h, pitch)    # the packed rows are all that crosses
                st.set_frame_reduction(f, fmt, pitch)
                ref.set_frame_reduction(f, capi.FRAME_GRAY16, 0)
                pairs.append((st.submit(pin(rs), pin(buf), Ms), ref.submit(pin(rs), pin(cont), Ms)))
            for t, r in pairs:
                same(outcome(st, t, WN, S, "plain"), outcome(ref, r, WN, S, "plain"))
            for bad in ((f, fmt, pnp.row_bytes(fmt, f * w) - 1), (1, 51, 0), (5, fmt, 0)):   # refused: the stream stays as it was
                with pytest.raises(capi.NmiError):
                    st.set_frame_reduction(*bad)
            F, rs, _ = frames[0]
            buf, pitch, cont = host_frames(F, fmt, f, seed=20)
            same(outcome(st, st.submit(pin(rs), pin(buf), Ms), WN, S, "plain"), outcome(ref, ref.submit(pin(rs), pin(cont), Ms), WN, S, "plain"))
        st.set_frame_reduction(1, capi.FRAME_GRAY, 0)
        ref.set_frame_reduction(1, capi.FRAME_GRAY, 0)
        F, rs, _ = frames[1]
        same(outcome(st, st.submit(pin(rs), pin(F), Ms), WN, S, "plain"), outcome(ref, ref.submit(pin(rs), pin(F), Ms), WN, S, "plain"))
