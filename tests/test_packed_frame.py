"""GPU tests (-m gpu) of the deep raw formats' standalone entries (include/nmi_hip.h "Deep frames"): nmi_unpack_frame against the
model of tests/helpers/packed_np.py, and nmi_gray_frame / nmi_reduce_frame / nmi_deep_frame on a packed, big-endian or 16-bit
mosaic source against THE SAME CALL on NMI_FRAME_GRAY16 given the model's container -- which is the definition.  Every comparison
is == on bytes.  Contexts of 4 x 1 (one group), 20 x 3, 52 x 38 and 68 x 5, factors 1 .. 4, dense and odd pitches, bases 0 .. 3
bytes off a 16-byte boundary."""
import numpy as np
import pytest

from helpers import packed_np as pnp
from orbslam2_nmi_amd import capi

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = [(4, 1), (20, 3), (52, 38), (68, 5)]
BAYER_SIZES = [(2, 2), (3, 2), (52, 38)]
FACTORS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def dev_at(buf, off):
    """The bytes of buf on the device, their first byte `off` bytes past a 16-byte boundary (a view: keep it to keep the memory)."""
    t = torch.empty(32 + buf.size, dtype=torch.uint8, device="cuda")
    start = (-t.data_ptr()) % 16 + off
    v = t[start:start + buf.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(buf)))
    assert v.data_ptr() % 16 == off
    return v


def dev16(cont):
    """A container [H,W] uint16 as the dense GRAY16 source the entries take: device uint8, little-endian."""
    return torch.from_numpy(np.ascontiguousarray(cont, "<u2").view(np.uint8).reshape(-1).copy()).cuda()


def layouts(fmt, ws):
    """(pitch, base offset) of every run: a dense pitch, then dense + 1 and dense + 3 (2-byte formats: dense + 2); a base 0 .. 3 bytes
    off a 16-byte boundary (2-byte formats: 0 and 2)."""
    dense = pnp.row_bytes(fmt, ws)
    words = pnp.GROUP[fmt][1] == 2
    return [(p, o) for p in ((0, dense + 2) if words else (0, dense + 1, dense + 3)) for o in ((0, 2) if words else (0, 1, 2, 3))]


def unpacked(ctx, d, fmt, f, pitch):
    return ctx.unpack_frame(d, fmt, f, pitch).cpu().numpy().view(np.uint16)


def tone_maps(ctx, bits, seed=0):
    """name -> ToneMap at `bits`, CLAHE's 3 x 2 tiles only where the context has room for them."""
    top = (1 << bits) - 1
    lut = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, capi.TONE_LEVELS).astype(np.uint8)).cuda()
    maps = {"shift": capi.ToneMap.shift(bits), "window": capi.ToneMap.window(top // 8, top - top // 4, bits),
            "pct": capi.ToneMap.percentile(300, 200, bits), "equalize": capi.ToneMap.equalize(0, bits),
            "table": capi.ToneMap.from_table(lut, bits), "clahe1": capi.ToneMap.clahe(1, 1, 0, bits)}
    if ctx.width >= 3 and ctx.height >= 2:
        maps["clahe32"] = capi.ToneMap.clahe(3, 2, 3, bits)
    return maps


def same_under_every_tone_map(ctx, d, fmt, f, pitch, cont, bits):
    """gray_frame (factor 1) and reduce_frame of the source == the same call on GRAY16 with the model's container."""
    d_cont = dev16(cont)
    seen = {}
    for name, tm in tone_maps(ctx, bits).items():
        ctx.set_tone_map(tm)
        want = ctx.reduce_frame(d_cont, capi.FRAME_GRAY16, f).cpu().numpy()
        got = ctx.reduce_frame(d, fmt, f, pitch).cpu().numpy()
        assert (got == want).all(), (name, fmt, f, pitch)
        if f == 1:
            assert (ctx.gray_frame(d, fmt, pitch).cpu().numpy() == ctx.gray_frame(d_cont, capi.FRAME_GRAY16).cpu().numpy()).all(), name
            assert (ctx.gray_frame(d, fmt, pitch).cpu().numpy() == want).all(), name
        seen[name] = got
    ctx.set_tone_map(None)
    return seen


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", pnp.LAYOUTS)
def test_unpack_equals_the_model(nmi, fmt, size):
    """(a): every factor, pitch, base and content."""
    w, h = size
    with nmi.NmiContext(w, h) as ctx:
        for f in FACTORS:
            ws, hs = f * w, f * h
            assert pnp.row_bytes(fmt, ws) > 0
            for name, px in pnp.contents(fmt, ws, hs, seed=f).items():
                for pitch, off in layouts(fmt, ws):
                    buf = pnp.frame(px, fmt, pitch, 0, seed=off)
                    d = dev_at(buf, off)
                    got = unpacked(ctx, d, fmt, f, pitch)
                    assert got.shape == (hs, ws) and (got == px).all(), (name, f, pitch, off)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", pnp.LAYOUTS)
def test_frames_equal_gray16_on_the_container(nmi, fmt, size):
    """(b): every tone mode, a different pitch and base at each factor."""
    w, h = size
    bits = pnp.BITS[fmt]
    with nmi.NmiContext(w, h) as ctx:
        for f in FACTORS:
            ws, hs = f * w, f * h
            runs = layouts(fmt, ws)
            pitch, off = runs[(3 * f + 1) % len(runs)]
            px = pnp.contents(fmt, ws, hs, seed=10 + f)["tail" if f % 2 else "random"]
            d = dev_at(pnp.frame(px, fmt, pitch, 0, seed=f), off)
            seen = same_under_every_tone_map(ctx, d, fmt, f, pitch, pnp.container(pnp.frame(px, fmt), fmt, ws, hs), bits)
            if w * h > 100:
                assert (seen["shift"] != seen["equalize"]).any()
        # a container pixel above the declared depth saturates like GRAY16's: 12-bit data declared as 10 bits
        if bits == 12:
            px = pnp.random_pixels(fmt, w, h, seed=5)
            ctx.set_tone_map(capi.ToneMap.equalize(0, 10))
            want = ctx.gray_frame(dev16(px), capi.FRAME_GRAY16).cpu().numpy()
            assert (ctx.gray_frame(dev_at(pnp.frame(px, fmt), 1), fmt).cpu().numpy() == want).all()


RANGES = {10: ((0, 1022), 1023), 12: ((1, 4095), 0)}   # bits -> (valid range, the planted invalid value)


@pytest.mark.parametrize("size,f", [((20, 3), 1), ((52, 38), 2), ((68, 5), 3)], ids=["20x3-f1", "52x38-f2", "68x5-f3"])
@pytest.mark.parametrize("fmt", pnp.PACKED)
def test_a_valid_range_is_taken_on_the_container(nmi, fmt, size, f):
    """(c): planted invalid pixels under the statistics modes, reduce_frame's mask pair, deep_frame on the unpacked container."""
    w, h = size
    ws, hs = f * w, f * h
    bits = pnp.BITS[fmt]
    (lo, hi), bad = RANGES[bits]
    rng = np.random.default_rng(fmt + f)
    px = rng.integers(lo + 1, hi, (hs, ws)).astype(np.uint16)      # (a band inside the range, then the plants)
    px = (px // 3 + (1 << bits) // 3).astype(np.uint16)
    plants = rng.random((hs, ws)) < 0.1
    plants[0, 0] = plants[-1, -1] = True
    px[plants] = bad
    pitch, off = pnp.row_bytes(fmt, ws) + 3, 3
    src_mask = (rng.random((hs, ws)) < 0.9).astype(np.uint8)
    frame_mask = (rng.random((h, w)) < 0.8).astype(np.uint8)
    with nmi.NmiContext(w, h) as ctx:
        d = dev_at(pnp.frame(px, fmt, pitch, 0, seed=1), off)
        d_cont, d_sm, d_fm = dev16(px), torch.from_numpy(src_mask).cuda(), torch.from_numpy(frame_mask).cuda()
        cont = ctx.unpack_frame(d, fmt, f, pitch)
        assert (cont.cpu().numpy().view(np.uint16) == px).all()
        for name, tm in tone_maps(ctx, bits).items():
            ctx.set_tone_map(tm)
            ctx.set_valid_range(0, 65535)
            off_frame = ctx.reduce_frame(d, fmt, f, pitch).cpu().numpy()
            ctx.set_valid_range(lo, hi)
            want, want_mask = ctx.reduce_frame(d_cont, capi.FRAME_GRAY16, f, 0, d_sm)
            got, got_mask = ctx.reduce_frame(d, fmt, f, pitch, d_sm)
            assert (got.cpu().numpy() == want.cpu().numpy()).all() and (got_mask.cpu().numpy() == want_mask.cpu().numpy()).all(), name
            assert (ctx.reduce_frame(d, fmt, f, pitch).cpu().numpy() == got.cpu().numpy()).all(), name
            # the mask: the pair's rule ANDed with validity of all f x f container pixels
            valid = ((px >= lo) & (px <= hi) & (src_mask != 0)).reshape(h, f, w, f).all(axis=(1, 3))
            assert (got_mask.cpu().numpy() == valid).all(), name
            if name in ("pct", "equalize", "clahe1"):
                assert (got.cpu().numpy() != off_frame).any(), name   # the plants were in the statistics, and are not now
            a, am = ctx.deep_frame(cont.view(torch.uint8).reshape(-1), f, 0, d_fm)
            b, bm = ctx.deep_frame(d_cont, f, 0, d_fm)
            assert (a.cpu().numpy() == b.cpu().numpy()).all() and (am.cpu().numpy() == bm.cpu().numpy()).all(), name
            assert (a.cpu().numpy() == got.cpu().numpy()).all(), name
        ctx.set_valid_range(0, 65535)


@pytest.mark.parametrize("size", BAYER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pattern", list(pnp.BAYER16))
def test_bayer16(nmi, pattern, size):
    """(d): the mosaic's container is the model's grey value of the raw 16-bit sites; every entry goes on from it."""
    w, h = size
    fmt = pnp.BAYER16[pattern]
    with nmi.NmiContext(w, h) as ctx:
        for f in FACTORS:
            ws, hs = f * w, f * h
            sites = {"random": pnp.random_pixels(fmt, ws, hs, seed=f), "ones": np.full((hs, ws), 65535, np.uint16)}
            sites["dark"] = (sites["random"] >> 8).astype(np.uint16)
            for name, m in sites.items():
                for pitch, off in layouts(fmt, ws):
                    d = dev_at(pnp.frame(m, fmt, pitch, 0, seed=off), off)
                    want = pnp.container(pnp.frame(m, fmt), fmt, ws, hs)
                    assert (unpacked(ctx, d, fmt, f, pitch) == want).all(), (name, f, pitch, off)
            assert (pnp.bayer16_gray(sites["ones"], fmt) == 65535).all()
            pitch, off = layouts(fmt, ws)[f % 4]
            d = dev_at(pnp.frame(sites["random"], fmt, pitch, 0, seed=7), off)
            same_under_every_tone_map(ctx, d, fmt, f, pitch, pnp.bayer16_gray(sites["random"], fmt), 16)
        # the four patterns are four different frames
        if w * h > 100:
            m = pnp.random_pixels(fmt, w, h, seed=1)
            others = [p for p in pnp.BAYER16 if p != pattern]
            mine = unpacked(ctx, dev_at(pnp.frame(m, fmt), 0), fmt, 1, 0)
            assert all((unpacked(ctx, dev_at(pnp.frame(m, pnp.BAYER16[p]), 0), pnp.BAYER16[p], 1, 0) != mine).any() for p in others)
