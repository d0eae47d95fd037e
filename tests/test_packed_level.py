"""GPU tests (-m gpu) of captured levels fed the deep raw formats (NMI_FRAME_MONO12P, _RAW10, _BAYER16_GRBG through
nmi_level_set_frame_format / _set_frame_reduction): the same warps, ratings and winner, bit for bit, as the same level fed
NMI_FRAME_GRAY16 with the model's container (tests/helpers/packed_np.py), at 64x48 and 52x38 with S = 3, Wn = 3 on a small point
cloud, at factor 1 and 2, with and without a lens, under SHIFT and EQUALIZE; and a walk through the setters."""
import numpy as np
import pytest

from helpers import packed_np as pnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import capi
from test_color_level import bits, lens_K, scene
from test_masked_level import dev, views, warps
from test_packed_frame import dev16, dev_at
from test_reduce_level import full_size

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

S, WN = 3, 3
RADTAN = unp.FAMILIES["barrel"]
FORMATS = {"mono12p": pnp.MONO12P, "raw10": pnp.RAW10, "bayer16-grbg": pnp.BAYER16["grbg"]}


@pytest.fixture(scope="module")
def nmi():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    import orbslam2_nmi_amd as m
    m.load_library()
    return m


def deep(gray, fmt, seed=0):
    """An 8-bit frame at the format's depth: the grey value in the top 8 bits, noise below."""
    extra = pnp.BITS[fmt] - 8
    noise = np.random.default_rng(seed).integers(0, 1 << extra, gray.shape)
    return ((np.asarray(gray, np.int64) << extra) | noise).astype(np.uint16)


def source(gray0, fmt, f, seed=0):
    """-> (flat buffer, pitch, base offset, the model's container) of the scene's frame at f times its size in fmt, with a pitch
    beyond the dense one and a base off a 16-byte boundary."""
    h, w = gray0.shape
    px = deep(gray0 if f == 1 else full_size(gray0, f, 1), fmt, seed)
    words = pnp.GROUP[fmt][1] == 2
    pitch, off = pnp.row_bytes(fmt, f * w) + (2 if words else 3), 2 if words else 1
    buf = pnp.frame(px, fmt, pitch, 0, seed)
    return buf, pitch, off, pnp.container(buf, fmt, f * w, f * h, pitch)


def tone_maps(fmt):
    return {"shift": capi.ToneMap.shift(pnp.BITS[fmt]), "equalize": capi.ToneMap.equalize(0, pnp.BITS[fmt])}


def replay(lv, mvps, Ms):
    win = lv.run(mvps, Ms)
    return win, [np.array(o, copy=True) for o in lv.outputs()]


def same_replay(a, b):
    assert a[0][0] == b[0][0], (a[0], b[0])
    assert bits(np.float32(a[0][1])) == bits(np.float32(b[0][1])), (a[0], b[0])
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):                    # renders, warps, ratings
        assert x.shape == y.shape and x.dtype == y.dtype
        assert (x.view(np.uint8) == y.view(np.uint8)).all()


@pytest.mark.parametrize("size", [(64, 48), (52, 38)], ids=["64x48", "52x38"])
@pytest.mark.parametrize("name", list(FORMATS))
def test_a_packed_level_equals_the_gray16_level_on_the_container(nmi, name, size):
    w, h = size
    fmt = FORMATS[name]
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, "plain")
        gray0 = sc.frame.cpu().numpy()
        mvps, Ms = views(sc.rp, S), warps(w, h, WN)
        K = lens_K(sc.rp)
        seen = []
        for f in (1, 2):
            buf, pitch, off, cont = source(gray0, fmt, f, seed=f)
            d, d_cont = dev_at(buf, off), dev16(cont)
            for lens in (False, True):
                with nmi.NmiLevel(ctx, sc.dx, sc.da, d, S, WN, 3.0) as lv, nmi.NmiLevel(ctx, sc.dx, sc.da, d_cont, S, WN, 3.0) as base:
                    for target in (lv, base):
                        if lens:
                            target.set_distortion(K, RADTAN)
                    lv.set_frame_reduction(f, fmt, pitch)
                    base.set_frame_reduction(f, capi.FRAME_GRAY16, 0)
                    for tm in tone_maps(fmt).values():
                        lv.set_tone_map(tm)
                        base.set_tone_map(tm)
                        got = replay(lv, mvps, Ms)
                        same_replay(got, replay(base, mvps, Ms))
                        same_replay(got, replay(lv, mvps, Ms))         # a second replay: the container and histograms start clean
                        seen.append(bits(got[1][2]).copy())
        assert (seen[0] != seen[1]).any()                              # SHIFT and EQUALIZE are different frames
        assert (seen[0] != seen[2]).any()                              # ... and so are the lens's


def test_a_level_walks_through_the_formats(nmi):
    """gray -> MONO12P -> GRAY16 -> RAW10 at factor 2 -> gray, in place in one frame buffer: each state replays as a fresh level in
    that state, and a refused setting leaves the level replaying as before."""
    w, h = 64, 48
    with nmi.NmiContext(w, h) as ctx:
        sc = scene(nmi, ctx, w, h, False, "plain")
        gray0 = sc.frame.cpu().numpy()
        mvps, Ms = views(sc.rp, S), warps(w, h, WN)
        tm = capi.ToneMap.equalize(0, 12)
        m12 = pnp.frame(deep(gray0, pnp.MONO12P, 1), pnp.MONO12P, 99)
        g16 = np.ascontiguousarray(deep(np.roll(gray0, 3, axis=1), pnp.MONO12P, 2), "<u2").view(np.uint8).reshape(-1)
        r10 = pnp.frame(deep(full_size(np.roll(gray0, 5, axis=0), 2, 3), pnp.RAW10, 3), pnp.RAW10, 163)
        # (setting, what the frame buffer holds then)
        states = [((1, capi.FRAME_GRAY, 0), gray0.reshape(-1)), ((1, pnp.MONO12P, 99), m12), ((1, capi.FRAME_GRAY16, 0), g16),
                  ((2, pnp.RAW10, 163), r10), ((1, capi.FRAME_GRAY, 0), gray0.reshape(-1))]
        refused = [(1, pnp.MONO12P, 95), (1, 51, 0), (1, pnp.BAYER16["rggb"], 2 * w + 1), (5, pnp.RAW10, 0), (2, pnp.MONO10P, 159)]
        room = max(b.size for _, b in states)
        frame = torch.zeros(room, dtype=torch.uint8, device="cuda")
        tables = []
        with nmi.NmiLevel(ctx, sc.dx, sc.da, frame, S, WN, 3.0) as lv:
            lv.set_tone_map(tm)
            for (f, fmt, pitch), content in states:
                frame[:content.size].copy_(dev(content))
                torch.cuda.synchronize()
                lv.set_frame_reduction(f, fmt, pitch)
                got = replay(lv, mvps, Ms)
                with nmi.NmiLevel(ctx, sc.dx, sc.da, dev(content), S, WN, 3.0) as fresh:
                    fresh.set_tone_map(tm)
                    fresh.set_frame_reduction(f, fmt, pitch)
                    same_replay(got, replay(fresh, mvps, Ms))
                for bad in refused:
                    with pytest.raises(capi.NmiError):
                        lv.set_frame_reduction(*bad)
                same_replay(got, replay(lv, mvps, Ms))
                tables.append(bits(got[1][2]).copy())
        assert (tables[0] == tables[4]).all() and (tables[0] != tables[1]).any() and (tables[1] != tables[3]).any()
