"""CPU twin of a frame intake state (csrc/nmi_intake.h: FrameIntake) -- TEST INFRASTRUCTURE ONLY.

grey_of() is the search-size grey frame and mask the warps must read when a level or a stream is in the state (lens, frame) on
one byte buffer.  It only composes the existing twins: color_np / sensor_np / tone_np (to_gray, reduce_frame) for the grey frame,
undistort_np / fisheye_np (undistort) for the lens.  No arithmetic of its own.

The buffer is 2H rows of `pitch` bytes starting `off` bytes in, wide enough for 2W RGB pixels a row.  A frame value is one
reading of those bytes: (factor, format, tone map), always with that pitch.  The nine named readings are the states of the
intake walks (tests/test_intake_level_walk.py, tests/test_intake_stream_walk.py); "gray16-f<f>-<tone>" names every other deep
reading, which a walk passes through when it sets the format and the tone map one call after the other.
"""
import numpy as np

from helpers import color_np as cnp
from helpers import fisheye_np as fnp
from helpers import reduce_np as rnp
from helpers import sensor_np as snp
from helpers import tone_np as tnp
from helpers import undistort_np as unp
from orbslam2_nmi_amd import synthetic as sy

LENSES = ("none", "barrel", "fisheye")
BARREL = unp.FAMILIES["barrel"]
FISHEYE = fnp.FAMILIES["euroc_eq"]

# Tone maps by name: "shift" is the default setting (a level or a stream that never had one).  The plateau and the percentiles
# are above 0, and WINDOW's pair lies inside the buffer's skewed values, so that no two of them give the same frame.
TONES = {"shift": tnp.tone(),
         "window": tnp.tone(tnp.WINDOW, 16, lo=1500, hi=42000),
         "eq": tnp.tone(tnp.EQUALIZE, 16, plateau=2),
         "pct": tnp.tone(tnp.PERCENTILE, 16, p_lo=300, p_hi=500)}

# name -> (factor, format, tone name or None: not a deep format)
FRAMES = {"gray": (1, cnp.GRAY, None), "rgb": (1, cnp.RGB, None), "rgb-f2": (2, cnp.RGB, None), "uyvy": (1, snp.UYVY, None),
          "grbg": (1, snp.GRBG, None), "bggr-f2": (2, snp.BGGR, None), "deep-window": (1, tnp.GRAY16, "window"),
          "deep-eq": (1, tnp.GRAY16, "eq"), "deep-pct-f2": (2, tnp.GRAY16, "pct")}
FRAME_NAMES = tuple(FRAMES)
STATES = [(lens, frame) for lens in LENSES for frame in FRAME_NAMES]


def deep_name(factor, tone):
    """The name of the deep reading (factor, GRAY16, tone): one of the nine where it is one, else "gray16-f<f>-<tone>"."""
    for name, spec in FRAMES.items():
        if spec == (factor, tnp.GRAY16, tone):
            return name
    return f"gray16-f{factor}-{tone}"


def frame_spec(frame):
    """A frame name -> (factor, format, tone name or None)."""
    if frame in FRAMES:
        return FRAMES[frame]
    if frame == "off":   # no setting: the buffer's first H * W bytes as a dense grey frame
        return 1, cnp.GRAY, None
    head, f, tone = frame.split("-", 2)
    assert head == "gray16" and f in ("f1", "f2") and tone in TONES, frame
    return int(f[1]), tnp.GRAY16, tone


def is_deep(frame):
    return frame_spec(frame)[1] == tnp.GRAY16


def call_order(i, origin=0):
    """The order of the two calls of move i into a deep value, for a walk that numbers its moves from `origin`: on even numbers
    the tone map first, while the format still ignores it; on odd numbers the format first, which passes through the deep format
    under the tone map set before."""
    return "tone-first" if (i + origin) % 2 == 0 else "frame-first"


class Layout:
    """One of the walks' two shapes: the search size, the buffer's pitch and base offset, and the map kind the levels draw."""

    def __init__(self, name, w, h, pad, off, mesh):
        self.name, self.w, self.h, self.pitch, self.off, self.mesh = name, w, h, 2 * w * 3 + pad, off, mesh
        self.rows = 2 * h

    @property
    def nbytes(self):
        return self.off + self.rows * self.pitch


# A: rows of whole 16-byte chunks (vector loads, fused front kernels, the grid kernel for the 9 candidates).  B: a pitch that is
# even but no multiple of 4, a width that is no multiple of 4 and >= 32, an even base offset (byte loads and stores, ragged
# quads, the warp on the forked branch, the pixel-range search kernel).
LAYOUTS = {"A": Layout("A", 64, 48, 16, 0, False), "B": Layout("B", 50, 38, 6, 2, True)}


def walk_buffer(lay, seed=0):
    """The bytes every reading reads: a smooth scene (orbslam2_nmi_amd.synthetic) over the 2H x pitch bytes with camera noise,
    through a gamma of 2.2 so that the values crowd towards the dark end: a deep reading's histogram is then far from flat, and
    EQUALIZE is far from SHIFT.  The `off` bytes in front are noise."""
    field = sy.camera_frame(sy.scene(lay.pitch, lay.rows, 77 + seed), 78 + seed).astype(np.float64)
    body = np.rint(255.0 * (field / 255.0) ** 2.2).astype(np.uint8)
    head = np.random.default_rng(seed).integers(0, 256, lay.off, dtype=np.uint8)
    return np.concatenate([head, body.reshape(-1)])


def rolled(buf, lay, k):
    """The buffer's content moved for ticket k: its rows rolled by (3k, 5k) bytes, the bytes in front of `off` kept."""
    body = buf[lay.off:].reshape(lay.rows, lay.pitch)
    return np.concatenate([buf[:lay.off], np.roll(body, shift=(3 * k, 5 * k), axis=(0, 1)).reshape(-1)])


def raw_K(K, w):
    """K_raw of the fisheye states, as tests/test_fisheye_level.py makes it: a longer focal length, the principal point moved."""
    Kr = fnp.pinhole_K(K, 1 / 0.6)
    Kr[0, 2] += 0.02 * w
    Kr[1, 2] -= 0.01 * w
    return Kr


def hood_mask(w, h):
    """A frame mask of the search size: a hood over the bottom sixth and a mount in the top-left corner."""
    m = np.ones((h, w), np.uint8)
    m[h - h // 6:] = 0
    m[:h // 8, :w // 10] = 0
    return m


def to_grey(buf, W, H, pitch, off, frame):
    """The grey frame [H][W] of one reading, before the lens."""
    factor, fmt, tone = frame_spec(frame)
    if frame == "off":
        pitch = 0
    if fmt == tnp.GRAY16:
        tm = TONES[tone]
        return tnp.to_gray(buf, W, H, tm, pitch, off) if factor == 1 else tnp.reduce_frame(buf, W, H, factor, tm, pitch, off)
    if fmt in snp.BPP:
        return snp.to_gray(buf, fmt, W, H, pitch, off) if factor == 1 else snp.reduce_frame(buf, fmt, W, H, factor, pitch, off)
    return cnp.to_gray(buf, fmt, W, H, pitch, off) if factor == 1 else rnp.reduce_frame(buf, fmt, W, H, factor, pitch, off)


def grey_of(buf, W, H, pitch, off, state, frame_mask=None, K=None):
    """state = (lens, frame) -> (grey [H][W] uint8, mask [H][W] uint8): the frame and the mask the warps read.  frame_mask: the raw
    frame's mask (dense [H][W]) or None.  Without a lens the mask is frame_mask itself (all ones for None); with one it is the
    undistorted mask: the border rule, and frame_mask under it.  K: the pinhole camera (default: synthetic.intrinsics(W, H))."""
    lens, frame = state
    grey = to_grey(np.asarray(buf, np.uint8), W, H, pitch, off, frame)
    assert grey.shape == (H, W) and grey.dtype == np.uint8
    K = sy.intrinsics(W, H) if K is None else np.asarray(K, np.float64)
    if lens == "none":
        return grey, (np.ones((H, W), np.uint8) if frame_mask is None else (np.asarray(frame_mask) != 0).astype(np.uint8))
    if lens == "barrel":
        return unp.undistort(grey, K, BARREL, frame_mask)
    assert lens == "fisheye", lens
    return fnp.undistort(grey, K, raw_K(K, W), FISHEYE, frame_mask)
