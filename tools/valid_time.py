"""Valid-range timing (nmi_set_valid_range on GRAY16 frames), after tools/clahe_time.py.  Prints one JSON line.

Phases, one after the other, host wall time of each call (the call ending in a synchronise):
  off/<size>/<content>/<mode>    nmi_gray_frame of a 640x480 frame, nmi_reduce_frame of a 2560x1920 source at factor 4, range off:
                                 content thermal (a 14-bit band 7000 .. 7400, twenty pixels at 16383; bits 14) or uniform (noise
                                 over 16 bits; bits 16); mode equalize or clahe (8 x 8 tiles).  These run on any library with
                                 CLAHE, so an earlier commit's (through NMI_HIP_LIBRARY) can be timed beside this one's.
  on/<size>/<content>/<mode>     the same calls with a range on (thermal: (0, 16382), the hot pixels out; uniform: (4096, 61439))
  deep/<size>/<content>/<mode>   nmi_deep_frame under that range: the masked conversion, with a frame mask
The on and deep phases need a library with nmi_set_valid_range and are skipped on one without.

--pipeline: the range inside a captured level and a keyframe stream (nmi_level_set_valid_range, nmi_stream_set_valid_range)
instead.  A masked point-cloud level with 27 x 27 candidates on tools/color_time.py's cloud, fed a 640x480 GRAY16 depth frame
(a 14-bit band with 30 % of its pixels 0, range (1, 65535)) under EQUALIZE and CLAHE 8 x 8, host wall time of nmi_level_run:
  level/off/<mode>      masks on, d_frame_mask NULL, range off: the parent's level
  level/on/<mode>       the range on: the conversion writes the validity mask the warp masks are made from
  level/caller/<mode>   range off and the same validity mask handed in as d_frame_mask: what a caller had to do before
and a masked keyframe (render stack, frame, 27 x 27) through a stream of depth 2, submit to wait:
  stream/off/<mode>, stream/on/<mode>, stream/caller/<mode>   the same three; caller uploads the H x W mask as h_frame_mask
The on phases are skipped on a library without the two calls.
--trace off|on: one replay of that masked level (EQUALIZE) and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --output-format csv -- python tools/valid_time.py --trace off); --names TRACE.csv then prints the
kernel names of that replay in launch order (from the last dispatch of the level's prep kernel onwards).

Kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/valid_time.py --iters 100 (every phase, so the
unranged kernels stand beside the ranged ones; --range-only leaves the off phases out), then python
tools/summarize_clahe_trace.py TRACE.csv CALLS_PER_PHASE PHASES (both printed in the JSON line).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbslam2_nmi_amd as nmi  # noqa: E402
from clahe_time import contents, med  # noqa: E402
from orbslam2_nmi_amd import capi  # noqa: E402

W, H = 640, 480
GRAY16 = capi.FRAME_GRAY16
RANGES = {"thermal": (0, 16382), "uniform": (4096, 61439)}


def modes(bits):
    return {"equalize": capi.ToneMap.equalize(0, bits), "clahe": capi.ToneMap.clahe(8, 8, 0, bits)}


def timed(call, iters, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"call_us": med(ts), "p10_us": round(float(np.percentile(ts, 10)), 2), "p90_us": round(float(np.percentile(ts, 90)), 2)}


def frame_phases(ctx, res, a, ranged):
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    out_mask = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    fm = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    fm[H - H // 6:] = 0
    for f in (1, 4):
        for cname, (px, bits) in contents(f * W, f * H).items():
            src = torch.from_numpy(np.ascontiguousarray(px).view(np.uint8).reshape(-1)).cuda()
            for mname, tm in modes(bits).items():
                ctx.set_tone_map(tm)

                def call():
                    if f == 1:
                        ctx.gray_frame(src, GRAY16, 0, out=out)
                    else:
                        ctx.reduce_frame(src, GRAY16, f, 0, out=out)

                def deep():
                    ctx.deep_frame(src, f, 0, frame_mask=fm, out=out, out_mask=out_mask)

                todo = [("off", call, None)] if not a.range_only else []
                if ranged:
                    todo += [("on", call, RANGES[cname]), ("deep", deep, RANGES[cname])]
                for kind, fn, rng in todo:
                    if ranged:
                        ctx.set_valid_range(*(rng or (0, 65535)))
                    ph = timed(fn, a.iters, a.warmup)
                    ph["name"] = f"{kind}/{f * W}x{f * H}/{cname}/{mname}"
                    ph["checksum"] = int(out.sum().item())
                    res["phases"].append(ph)


def depth_frame(gray, seed=0):
    """The scene's 8-bit frame as a 14-bit depth frame with 30 % holes (0): (pixels uint16, range, validity mask uint8)."""
    rng = np.random.default_rng(seed)
    px = (7000 + gray.astype(np.int64) * 12).astype(np.uint16)
    px[rng.random(px.shape) < 0.3] = 0
    return px, (1, 65535), (px != 0).astype(np.uint8)


def pipeline_scene(ctx):
    """color_time.py's cloud, 27 views, 27 warps and the frame the centre view sees."""
    from color_time import level_scene
    from orbslam2_nmi_amd import hostapi as Hh
    K, rp, xyz, red = level_scene(W, H)
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, 1] = [0, -1, 0]
    pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
    g = Hh.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
    cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
    mvps = np.stack([capi.render_mvp(rp, pos, look, up, Hh.calculate_translation(Twc, g, *c)) for c in cells])
    homs = capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
    frame = torch.flip(ctx.render_points(dx, torch.sqrt(dr), capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None], 3.0)[0], dims=[0]).contiguous()
    renders = ctx.render_points(dx, dr, mvps, 3.0)
    torch.cuda.synchronize()
    return dx, dr, mvps, homs, frame.cpu().numpy(), renders.cpu()


def pipeline_modes():
    return {"equalize": capi.ToneMap.equalize(0, 14), "clahe": capi.ToneMap.clahe(8, 8, 0, 14)}


def masked_level(ctx, dx, dr, src, tm, rng, d_mask):
    lv = nmi.NmiLevel(ctx, dx, dr, src, 27, 27, 3.0)
    lv.set_frame_format(GRAY16, 0)
    lv.set_tone_map(tm)
    lv.set_masks(True, d_mask)
    if rng is not None:
        lv.set_valid_range(*rng)
    return lv


def pipeline_phases(ctx, res, a, ranged):
    dx, dr, mvps, homs, gray, renders = pipeline_scene(ctx)
    px, rng, valid = depth_frame(gray)
    src = torch.from_numpy(np.ascontiguousarray(px).view(np.uint8).reshape(-1)).cuda()
    d_valid = torch.from_numpy(valid).cuda()
    ways = [("off", None, None), ("on", rng, None), ("caller", None, d_valid)]
    for mname, tm in pipeline_modes().items():
        for way, r, d_mask in ways:
            if way == "on" and not ranged:
                continue
            with masked_level(ctx, dx, dr, src, tm, r, d_mask) as lv:
                run = lv.bind(mvps, homs)
                ph = timed(run, a.iters, a.warmup)
                ph["name"] = f"level/{way}/{mname}"
                ph["winner"] = list(run())
                res["phases"].append(ph)
    host_src, host_valid, host_rs = src.cpu().pin_memory(), torch.from_numpy(valid).pin_memory(), renders.pin_memory()
    for mname, tm in pipeline_modes().items():
        for way, r, mask in [("off", None, None), ("on", rng, None), ("caller", None, host_valid)]:
            if way == "on" and not ranged:
                continue
            with nmi.NmiStream(ctx, 27, 27, depth=2) as st:
                st.set_frame_format(GRAY16, 0)
                st.set_tone_map(tm)
                if r is not None:
                    st.set_valid_range(*r)
                win = []

                def keyframe():
                    win[:] = st.wait(st.submit_masked(host_rs, host_src, mask, homs))

                ph = timed(keyframe, a.iters, a.warmup)
                ph["name"] = f"stream/{way}/{mname}"
                ph["winner"] = [int(win[0]), float(win[1])]
                res["phases"].append(ph)


def trace_one(ctx, way):
    """One replay of the masked GRAY16 level and nothing else on the device after its set-up."""
    dx, dr, mvps, homs, gray, _ = pipeline_scene(ctx)
    px, rng, _ = depth_frame(gray)
    src = torch.from_numpy(np.ascontiguousarray(px).view(np.uint8).reshape(-1)).cuda()
    with masked_level(ctx, dx, dr, src, pipeline_modes()["equalize"], rng if way == "on" else None, None) as lv:
        torch.cuda.synchronize()
        print(json.dumps({"trace": way, "winner": [float(v) for v in lv.run(mvps, homs)]}))
        torch.cuda.synchronize()


def replay_names(path):
    """Kernel names, in launch order, of the last level replay in a rocprofv3 kernel trace: from the last dispatch of the level's
    prep kernel to the end."""
    import csv
    with open(path) as f:
        rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    names = [n for _, n in rows]
    last = max(i for i, n in enumerate(names) if "level_prep" in n)
    for n in names[last:]:
        print(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--range-only", action="store_true", help="the on and deep phases alone (kernel traces)")
    ap.add_argument("--pipeline", action="store_true", help="a masked level's replay and a stream keyframe, three ways each")
    ap.add_argument("--trace", choices=["off", "on"], help="one replay of the masked level, for a kernel trace")
    ap.add_argument("--names", metavar="TRACE.csv", help="print the kernel names of the last replay in a kernel trace")
    a = ap.parse_args()
    if a.names:
        return replay_names(a.names)
    lib = capi.load_library()
    ranged = hasattr(lib, "nmi_set_valid_range")
    if a.trace or a.pipeline:
        ranged = hasattr(lib, "nmi_level_set_valid_range")
    res = {"shape": [W, H], "calls_per_phase": a.iters + a.warmup, "valid_range": ranged, "phases": []}
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    with nmi.NmiContext(W, H) as ctx:
        ctx.set_stream(st.cuda_stream)
        if a.trace:
            trace_one(ctx, a.trace)
            return
        if a.pipeline:
            pipeline_phases(ctx, res, a, ranged)
        else:
            frame_phases(ctx, res, a, ranged)
    torch.cuda.set_stream(torch.cuda.default_stream())
    res["phase_names"] = ",".join(p["name"] for p in res["phases"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
