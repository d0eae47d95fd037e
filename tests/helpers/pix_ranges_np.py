"""Which candidates of a pixel-range launch must fail the count test, worked out from the stacks alone (numpy).

A candidate's pixels are DEALT to its P workgroups (csrc/nmi_pix_device.h: pix_dealing, make_deal, Pieces): the frame's 16-pixel
chunks (rows' last width % 16 pixels apart) in pieces of 64, the pieces in periods of own + (P - 1) * hlp -- the owner takes the
first `own` of a period, helper q the `hlp` from own + (q - 1) * hlp on -- and own : hlp is the ratio closest to the owner's
share, ((W*H + (P - 1) * bias) / P) / (W*H) with NMI_OPT_PIX_OWNER_BIAS = 49152 by default (nmi_capi.cpp: pix_owner_share).  The
row tails are the owner's.

Every workgroup counts into 16-bit fields of its own, the owner adds its helpers' packed words to each other as packed words
(pix_collect: acc += v) and only then to its own fields in 32 bits (decode_merged).  So a field loses weight, and the decoded total
falls short of the pixels added, exactly when a bin of the OWNER's share, or of the HELPERS' shares taken together, exceeds
65,535 -- not when a bin of the whole pair does: 76,800 hits spread over an owner and two helpers wrap nothing, and the merged
decode is then exact.  count_test_redos counts the candidates for which that holds."""
import numpy as np

PIECE_CHUNKS = 64
DEFAULT_OWNER_BIAS = 49152


def dealing(npix, P, bias=DEFAULT_OWNER_BIAS):
    """-> (own, hlp): pieces per period of the owner and of each helper (pix_owner_share + pix_dealing)."""
    owner_px = (npix + (P - 1) * bias) / P
    f = min(max(owner_px / npix if owner_px < npix else 1.0, 0.02), 0.98)
    own, hlp, best = 1, 1, 2.0
    for b in range(1, 13):
        o = max(int(f / (1.0 - f) * (P - 1) * b + 0.5), 1)
        if o + (P - 1) * b > 48:
            break
        err = abs(o / (o + (P - 1) * b) - f)
        if err < best - 0.03:
            best, own, hlp = err, o, b
    return own, hlp


def range_of_pixels(w, h, P, bias=DEFAULT_OWNER_BIAS):
    """-> uint8 [h, w]: the range (0 = owner, q = helper q) that adds the pair's pixel at frame position (y, x)."""
    own, hlp = dealing(w * h, P, bias)
    L = own + (P - 1) * hlp
    of_slot = np.array([0] * own + [1 + k // hlp for k in range((P - 1) * hlp)], np.uint8)
    cpr = w // 16
    yy, xx = np.mgrid[0:h, 0:w]
    piece = (yy * cpr + xx // 16) // PIECE_CHUNKS
    return np.where(xx < cpr * 16, of_slot[piece % L], 0).astype(np.uint8)


def count_test_redos(rs, ws, P, render_bottom_up, keep=None, bias=DEFAULT_OWNER_BIAS):
    """Candidates (render s, warp v) of rs x ws on P ranges whose merged decode must fail the count test.  keep(v, s) -> bool
    [h, w] in the frame's row order, the pixels of that candidate that are added at all (None: every pixel)."""
    h, w = rs.shape[1:]
    rng = range_of_pixels(w, h, P, bias).ravel()
    seen, redos = {}, 0
    for v in range(len(ws)):
        for s in range(len(rs)):
            r = rs[s, ::-1] if render_bottom_up else rs[s]
            k = np.ones((h, w), bool) if keep is None else keep(v, s)
            key = (r.tobytes(), ws[v].tobytes(), k.tobytes())
            if key not in seen:
                cell = (r.astype(np.int64) * 256 + ws[v]).ravel()
                kf = k.ravel()
                owner = np.bincount(cell[kf & (rng == 0)], minlength=65536)
                helpers = np.bincount(cell[kf & (rng != 0)], minlength=65536)
                seen[key] = bool(owner.max() > 65535 or helpers.max() > 65535)
            redos += seen[key]
    return redos
