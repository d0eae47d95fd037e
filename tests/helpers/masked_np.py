"""numpy restatement of the masked search and of the warp-mask producer -- TEST INFRASTRUCTURE ONLY.

warp_masks: the validity rule of nmi_warp_stack_masked (include/nmi_hip.h) with the fp32 source coordinates computed as
oracle/warp_oracle_np.py computes them (the twin of the warp kernels' arithmetic, same operation order).

masked_hist / masked_search: the joint histogram counted with exact integers (render flip, background rule on the raw
values, then the shift) and scored by the oracle's score_from_hist with length = len_w, under oracle.binding.rounded() --
the product's bits.
"""
import numpy as np

from oracle import binding as oc
from oracle.warp_oracle_np import device_coeffs

f32 = np.float32


def warp_masks(shape, homographies, frame_mask=None):
    """-> uint8 [Wn, H, W]: 1 where the pixel of warp w interpolates from inside the frame (and from nonzero frame_mask
    taps), else 0."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    fx, fy = xx.astype(f32), yy.astype(f32)
    fm = None if frame_mask is None else (np.asarray(frame_mask) != 0)
    out = np.zeros((len(homographies), h, w), np.uint8)
    for i, M in enumerate(homographies):
        c = device_coeffs(M)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            coeff = f32(1.0) / ((c[6] * fx + c[7] * fy) + c[8])
            xs = coeff * ((c[0] * fx + c[1] * fy) + c[2])
            ys = coeff * ((c[3] * fx + c[4] * fy) + c[5])
            inside = (xs > f32(-2)) & (xs < f32(w + 1)) & (ys > f32(-2)) & (ys < f32(h + 1))
            xs = np.where(inside, xs, f32(0))
            ys = np.where(inside, ys, f32(0))
        x1 = np.floor(xs).astype(np.int64)
        y1 = np.floor(ys).astype(np.int64)
        x2 = x1 + (xs != x1.astype(f32))  # the second tap only where its weight is nonzero
        y2 = y1 + (ys != y1.astype(f32))
        ok = inside & (x1 >= 0) & (y1 >= 0) & (x2 <= w - 1) & (y2 <= h - 1)
        if fm is not None:
            cx1, cx2 = np.clip(x1, 0, w - 1), np.clip(x2, 0, w - 1)
            cy1, cy2 = np.clip(y1, 0, h - 1), np.clip(y2, 0, h - 1)
            ok &= fm[cy1, cx1] & fm[cy1, cx2] & fm[cy2, cx1] & fm[cy2, cx2]
        out[i] = ok
    return out


def masked_hist(render, warped, mask, shift=0, use_bg=True, render_bottom_up=True):
    """-> (joint [256, 256], h1 [256], h2 [256]) uint32 of the pixels that take part."""
    r = (render[::-1] if render_bottom_up else render).reshape(-1).astype(np.int64)
    wv = warped.reshape(-1).astype(np.int64)
    take = mask.reshape(-1) != 0
    if not use_bg:
        take &= (r != 0) & (wv != 0)
    d1, d2 = r[take] >> shift, wv[take] >> shift
    joint = np.bincount(d1 * 256 + d2, minlength=65536).astype(np.uint32).reshape(256, 256)
    return joint, joint.sum(axis=1, dtype=np.uint32), joint.sum(axis=0, dtype=np.uint32)


def masked_search(render_stack, warp_stack, warp_masks_, shift=0, use_bg=True, render_bottom_up=True, mode=oc.MODE_SUC,
                  rounded=True):
    """-> (ratings [Wn, S] float32, best linear index, best score) with len_w = popcount(mask[w])."""
    S, Wn = render_stack.shape[0], warp_stack.shape[0]
    ratings = np.zeros((Wn, S), np.float32)
    ctx = oc.rounded() if rounded else oc.term_mode(oc.TERM_LIBM)
    with ctx:
        for w in range(Wn):
            length = int(np.count_nonzero(warp_masks_[w]))
            for s in range(S):
                j, h1, h2 = masked_hist(render_stack[s], warp_stack[w], warp_masks_[w], shift, use_bg, render_bottom_up)
                ratings[w, s] = oc.score_from_hist(j, h1, h2, length, mode)[0]
    idx, best = oc.find_max(ratings)
    return ratings, idx, best
