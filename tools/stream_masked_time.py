"""Keyframes/s of the streaming form (nmi_stream_*) with plain, masked and covered tickets at BASELINE configs[4]'s shape:
848 x 480, 3 levels x 27 renders x 27 warps per keyframe, depth 2, pinned host buffers, a frame (and, masked / covered, a
frame mask) with every level as bench.py --config stream submits them.  Covered tickets also carry the render masks as bits
(nmi_pack_mask_bits' layout, packed once on the device here the way a GPU producer would).

Prints one JSON line per mode -- keyframes/s (median of --reps timed runs) and H2D bytes per keyframe -- and, with --out, writes
them to that file.  For the unpack kernel's time, run it under rocprofv3 --kernel-trace --stats with --modes covered.

    python tools/stream_masked_time.py [--keyframes 200] [--reps 5] [--modes plain,masked,covered] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", default="plain,masked,covered")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import orbslam2_nmi_amd as nmi
    from orbslam2_nmi_amd import capi, synthetic as sy

    w, h, counts, levels, pool = 848, 480, (3, 3, 3), 3, 4
    npix, S, Wn = w * h, 27, 27
    K = sy.intrinsics(w, h)
    ctx = nmi.NmiContext(w, h, render_bottom_up=False)
    fmask = np.ones((h, w), np.uint8)
    fmask[h - h // 6:] = 0  # a bonnet in the bottom sixth of the frame
    hmask = torch.from_numpy(fmask).pin_memory()
    frames, stacks, bits, homs = [], [], [], []
    rng = np.random.default_rng(5)
    for kf in range(pool):
        B = sy.scene(w, h, 9000 + kf)
        frames.append(torch.from_numpy(sy.camera_frame(B, 9500 + kf)).pin_memory())
        for lvl in range(levels):
            rs = sy.render_stack(B, counts, shift_px=max(1, 4 >> lvl), zoom_step=0.02 / 2 ** lvl)
            cover = np.ones((S, h, w), np.uint8)
            for s in range(S):  # a hole in the map, somewhere different in every view
                y0, x0 = rng.integers(0, h // 2), rng.integers(0, w // 2)
                cover[s, y0:y0 + h // 4, x0:x0 + w // 5] = 0
            rs[cover == 0] = 255
            stacks.append(torch.from_numpy(rs).pin_memory())
            bits.append(ctx.pack_mask_bits(torch.from_numpy(cover).cuda()).cpu().pin_memory())
            homs.append(capi.warp_homographies(K, counts, tuple(s / 2 ** lvl for s in (0.02, 0.02, 0.05))))
    st = nmi.NmiStream(ctx, S, Wn, depth=2)

    def submit(mode, i):
        p = (i // levels) % pool
        j = p * levels + i % levels
        if mode == "plain":
            return st.submit(stacks[j], frames[p], homs[j])
        if mode == "masked":
            return st.submit_masked(stacks[j], frames[p], hmask, homs[j])
        return st.submit_covered(stacks[j], bits[j], frames[p], hmask, homs[j])

    def run(mode, n_kf):
        pending, winners = [], []
        for i in range(n_kf * levels):
            pending.append(submit(mode, i))
            if len(pending) == 2:
                winners.append(st.wait(pending.pop(0))[0])
        winners += [st.wait(t)[0] for t in pending]
        return winners

    h2d = {"plain": levels * (S * npix + npix)}
    h2d["masked"] = h2d["plain"] + levels * npix
    h2d["covered"] = h2d["masked"] + levels * S * ((npix + 7) // 8)
    lines = []
    for mode in args.modes.split(","):
        run(mode, 4)  # warm-up: allocations on the first masked / covered submission, code objects
        rates = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            winners = run(mode, args.keyframes)
            dt = time.perf_counter() - t0
            rates.append(args.keyframes / dt)
        line = {"mode": mode, "keyframes_per_s": round(float(np.median(rates)), 1), "runs": [round(r, 1) for r in rates],
                "h2d_bytes_per_keyframe": h2d[mode], "keyframes": args.keyframes,
                "shape": "848x480, 3 levels x 27 renders x 27 warps, depth 2", "distinct_winners": len(set(winners))}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if "plain" in args.modes:
        base = next(l["keyframes_per_s"] for l in lines if l["mode"] == "plain")
        ratio = {l["mode"]: round(l["keyframes_per_s"] / base, 3) for l in lines}
        lines.append({"ratio_to_plain": ratio})
        print(json.dumps(lines[-1]), flush=True)
    st.close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
