"""GPU tests (-m gpu) of nmi_reduce_frame on deep grey frames (NMI_FRAME_GRAY16): the tone map's statistics from the full-size
frame, each source pixel mapped, then the rounded box average == the numpy twin (tests/helpers/tone_np.py through
helpers/reduce_np.py), at factors 2, 3 and 4, with and without a source mask (whose rule is the existing one)."""
import numpy as np
import pytest

from helpers import reduce_np as rnp
from helpers import tone_np as tnp
from orbslam2_nmi_amd import capi
from test_tone_frame import dev, tones

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# search size, factor, source pitch (0: dense), base offset.  620x188: the 1241x376 source's spare column is never read;
# 261x9 and 264x8: a second block column of the conversion at factors 3 (its last quad one pixel) and 4
CASES = [(5, 3, 2, 0, 0), (5, 3, 3, 2 * 15 + 2, 2), (5, 3, 4, 2 * 20 + 10, 6), (64, 48, 2, 0, 0), (64, 48, 3, 2 * 192 + 64, 0),
         (64, 48, 4, 2 * 256 + 6, 2), (620, 188, 2, 2 * 1241, 0), (261, 9, 3, 0, 0), (264, 8, 4, 2 * 1056 + 8, 0)]
CONTENTS = {"uniform": (lambda w, h: tnp.uniform(w, h, 5), 16), "thermal": (lambda w, h: tnp.thermal(w, h, 6), 14),
            "flat": (lambda w, h: tnp.flat(w, h), 16)}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("case", CASES, ids=[f"{w}x{h}-f{f}-p{p}-o{o}" for w, h, f, p, o in CASES])
def test_reduce_frame_equals_the_twin(nmi, case, content):
    w, h, f, pitch, off = case
    make, bits = CONTENTS[content]
    sw = pitch // 2 if pitch else f * w                              # the source's own width (a spare column under a pitch)
    px = make(max(sw, f * w), f * h)[:, :f * w]
    buf = tnp.pack16(px, pitch, off, seed=3)
    d = dev(buf)
    mask = (np.random.default_rng(7).random((f * h, f * w)) < 0.9).astype(np.uint8) * 3
    with nmi.NmiContext(w, h) as ctx:
        for name, tm in tones(bits, seed=2).items():
            d_lut = dev(tm["lut"]) if tm["mode"] == tnp.TABLE else None
            ctx.set_tone_map(tnp.capi_tone(capi, tm, d_lut))
            want = tnp.reduce_frame(buf, w, h, f, tm, pitch, off)
            out = torch.full((h, w), 0xAB, dtype=torch.uint8, device="cuda")
            ctx.reduce_frame(d[off:], capi.FRAME_GRAY16, f, pitch, out=out)
            got = out.cpu().numpy()
            assert (got == want).all(), (name, np.argwhere(got != want)[:5])
            g2, m2 = ctx.reduce_frame(d[off:], capi.FRAME_GRAY16, f, pitch, src_mask=dev(mask))
            assert (g2.cpu().numpy() == want).all(), name              # a mask does not change the statistics
            assert (m2.cpu().numpy() == rnp.reduce_mask(mask, f)).all(), name
            lut, pair = ctx.tone_lut(d[off:], f, pitch)
            want_lut, want_pair = tnp.lut_of(buf, f * w, f * h, tm, pitch, off)
            assert pair == want_pair and (lut.cpu().numpy() == want_lut).all(), name


def test_factor_one_is_gray_frame(nmi):
    w, h = 64, 48
    px = tnp.thermal(w, h, 1)
    d = dev(tnp.pack16(px, 2 * w + 10))
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_tone_map(capi.ToneMap.equalize(bits=14))
        a = ctx.reduce_frame(d, capi.FRAME_GRAY16, 1, 2 * w + 10).cpu().numpy()
        b = ctx.gray_frame(d, capi.FRAME_GRAY16, 2 * w + 10).cpu().numpy()
        assert (a == b).all() and (a == tnp.apply(px, tnp.tone(tnp.EQUALIZE, 14))).all()
