"""numpy restatement of the covered search (masks on both sides) and of the renderers' coverage -- TEST INFRASTRUCTURE ONLY.

covered_search: the joint histogram of masked_np.masked_hist with mask = (wm[w] != 0) & (flip(rm[s]) != 0) and length =
len[w][s], the number of pixels where both masks are nonzero, scored by the oracle's score_from_hist under
oracle.binding.rounded() -- the product's bits.  len = 0 scores 0.0.

coverage_twin_points / coverage_twin_mesh: what the renderers cover, from the unmodified numpy twins in oracle/: the same
views rendered with every red 0 / an all-black texture, covered = != 255 (the clear colour).
"""
import numpy as np

from helpers import masked_np as mnp
from oracle import binding as oc
from oracle import mesh_oracle_np as mo
from oracle import render_oracle_np as ro


def pair_mask(wm_w, rm_s, render_bottom_up=True):
    """-> bool [H, W] in frame (warp) coordinates: both masks nonzero."""
    r = rm_s[::-1] if render_bottom_up else rm_s
    return (np.asarray(wm_w) != 0) & (np.asarray(r) != 0)


def cover_counts(wm, rm, render_bottom_up=True):
    """-> int32 [Wn, S]: len[w][s]."""
    out = np.zeros((wm.shape[0], rm.shape[0]), np.int32)
    for w in range(wm.shape[0]):
        for s in range(rm.shape[0]):
            out[w, s] = np.count_nonzero(pair_mask(wm[w], rm[s], render_bottom_up))
    return out


def covered_search(rs, ws, wm, rm, shift=0, use_bg=True, render_bottom_up=True, mode=oc.MODE_SUC, rounded=True):
    """-> (ratings [Wn, S] float32, best linear index, best score, counts [Wn, S])."""
    S, Wn = rs.shape[0], ws.shape[0]
    ratings = np.zeros((Wn, S), np.float32)
    counts = np.zeros((Wn, S), np.int32)
    ctx = oc.rounded() if rounded else oc.term_mode(oc.TERM_LIBM)
    with ctx:
        for w in range(Wn):
            for s in range(S):
                mask = pair_mask(wm[w], rm[s], render_bottom_up)
                length = int(np.count_nonzero(mask))
                counts[w, s] = length
                if length == 0:
                    continue  # nothing counts: 0.0
                j, h1, h2 = mnp.masked_hist(rs[s], ws[w], mask.astype(np.uint8), shift, use_bg, render_bottom_up)
                ratings[w, s] = oc.score_from_hist(j, h1, h2, length, mode)[0]
    idx, best = oc.find_max(ratings)
    return ratings, idx, best, counts


def coverage_twin_points(xyz, mvps, width, height, point_size):
    """-> uint8 [S, H, W] (render layout): 1 where the point-cloud twin draws a point."""
    red = np.zeros(len(xyz), np.float32)
    return (ro.render_stack(xyz, red, mvps, width, height, point_size) != 255).astype(np.uint8)


def coverage_twin_mesh(xyz, uv, mvps, width, height):
    """-> uint8 [S, H, W] (render layout): 1 where the mesh twin draws a triangle."""
    levels = mo.mip_luma(np.zeros((4, 4, 3), np.uint8))
    return (mo.render_stack(xyz, uv, levels, mvps, width, height) != 255).astype(np.uint8)
