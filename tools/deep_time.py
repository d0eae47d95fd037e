"""Deep grey frames timing (NMI_FRAME_GRAY16 with a tone map through nmi_level_set_frame_format / _set_frame_reduction), after
tools/sensor_time.py.  Prints one JSON line.

A captured point-cloud level with 27 x 27 candidates on tools/color_time.py's cloud, host wall time of each nmi_level_run, in
phases that run one after the other (tools/summarize_deep_trace.py splits a kernel trace by them):
  grey        the level fed a pitched 8-bit grey frame (rows of W + 64 bytes): the bar.  --grey-only stops after it, so that a
              library built from an earlier commit runs it too (NMI_HIP_LIBRARY points the loader at it).
  <content>/<mode>   the same level fed a pitched GRAY16 frame (rows of 2 W + 64 bytes), content uniform (noise over 16 bits),
              thermal (a 14-bit band 7000 .. 7400 around the scene, twenty pixels at 16383) or flat (one value), tone map SHIFT,
              PERCENTILE(100, 100) or EQUALIZE
  grey        once more at the end: how far the bar moved within the run
at 640x480, and with --reduced a 960x540 level fed 1920x1080 frames through set_frame_reduction(2, ...).

Kernel times: rocprofv3 --kernel-trace --output-format csv -- python tools/deep_time.py --iters 100, then
python tools/summarize_deep_trace.py TRACE.csv REPLAYS_PER_PHASE
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbslam2_nmi_amd as nmi  # noqa: E402
from color_time import level_scene, med  # noqa: E402
from orbslam2_nmi_amd import capi, hostapi as H  # noqa: E402

GRAY16 = 48


def pitched(img, pitch):
    """[H,W] uint8 or uint16 -> flat uint8 rows of `pitch` bytes (little-endian), zero padding."""
    raw = np.ascontiguousarray(img).view(np.uint8).reshape(img.shape[0], -1)
    buf = np.zeros((img.shape[0], pitch), np.uint8)
    buf[:, :raw.shape[1]] = raw
    return buf.reshape(-1)


def deep_contents(gray, f, seed=0):
    """The scene's 8-bit frame (at f times its size) as 16-bit contents."""
    rng = np.random.default_rng(seed)
    big = np.kron(gray, np.ones((f, f), np.uint8)).astype(np.int64)
    thermal = (7000 + big * 400 // 255).astype(np.uint16)
    thermal.reshape(-1)[rng.choice(thermal.size, 20, replace=False)] = 16383
    return {"uniform": rng.integers(0, 65536, big.shape).astype(np.uint16), "thermal": thermal, "flat": np.full(big.shape, 7123, np.uint16)}


def tone_modes(bits):
    T = getattr(capi, "ToneMap", None)
    return {"shift": T.shift(bits), "percentile": T.percentile(100, 100, bits), "equalize": T.equalize(0, bits)}


def run_level(w, h, f, iters, warmup, grey_only):
    K, rp, xyz, red = level_scene(w, h)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
    out = {"shape": [w, h], "factor": f, "grid": [27, 27], "points": int(xyz.shape[0]), "replays_per_phase": iters + warmup, "phases": []}
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_stream(st.cuda_stream)
        Twc = np.eye(4, dtype=np.float32)
        Twc[:3, 1] = [0, -1, 0]
        pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
        g = H.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
        cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
        mvps = np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
        homs = capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
        frame = torch.flip(ctx.render_points(dx, torch.sqrt(dr), capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None], 3.0)[0], dims=[0]).contiguous()
        torch.cuda.synchronize()
        gray = frame.cpu().numpy()

        def phase(name, src, setup):
            lv = nmi.NmiLevel(ctx, dx, dr, src, 27, 27, 3.0)
            setup(lv)
            run = lv.bind(mvps, homs)
            for _ in range(warmup):
                run()
            ts = []
            for _ in range(iters):
                t0 = time.perf_counter()
                run()
                ts.append((time.perf_counter() - t0) * 1e6)
            lv.close()
            out["phases"].append({"name": name, "level_us": med(ts)})

        big8 = np.kron(gray, np.ones((f, f), np.uint8))
        p8, p16 = f * w + 64, 2 * f * w + 64
        grey_src = torch.from_numpy(pitched(big8, p8)).cuda()
        phase("grey", grey_src, lambda lv: lv.set_frame_reduction(f, 0, p8))
        if not grey_only:
            for cname, px in deep_contents(gray, f).items():
                src = torch.from_numpy(pitched(px, p16)).cuda()
                for mname, tm in tone_modes(14 if cname == "thermal" else 16).items():
                    def setup(lv, tm=tm):
                        lv.set_frame_reduction(f, GRAY16, p16)
                        lv.set_tone_map(tm)
                    phase(f"{cname}/{mname}", src, setup)
            phase("grey", grey_src, lambda lv: lv.set_frame_reduction(f, 0, p8))
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--grey-only", action="store_true")
    ap.add_argument("--reduced", action="store_true")
    a = ap.parse_args()
    nmi.load_library()
    res = {"level_640x480": run_level(640, 480, 1, a.iters, a.warmup, a.grey_only)}
    if a.reduced:
        res["level_960x540_from_1920x1080"] = run_level(960, 540, 2, a.iters, a.warmup, a.grey_only)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
