#!/usr/bin/env python3
"""Where nmi_grid_kernel's time goes on a grid of S x Wn candidates (one workgroup per candidate): wall_clock64 stamps
(100 MHz) at the phase boundaries of one candidate of every workgroup -- its k-th, the first by default (NMI_OPT_STAMPS,
NMI_OPT_STAMP_CANDIDATE -> nmi_grid_kernel<GridStamped, ..>, csrc/nmi_kernels_stamped.hip) -- and the moment each of the 16 wavefronts added its last pixel.
python tools/grid_stamps.py [S Wn] [--noise] [--k K] [--shares FILE] [--calibrate N] [--out FILE]
  --k K          stamp every workgroup's K-th candidate (0 or 1 on a 27 x 27 grid: wavefront 0 scores the previous candidate
                 before it starts on the K-th's pixels when K > 0)
  --shares FILE  JSON {"first": [16 shares], "later": [16 shares]}: the wavefronts' pixel shares the stamped kernel runs with
                 (NMI_OPT_WAVE_SHARES) in place of the built-in ones (slab_cum, csrc/nmi_grid_device.h)
  --calibrate N  N rounds of: stamp, new share = old share x (mean end time / the wavefront's end time), for the row of
                 shares that the K-th candidate uses; needs --shares for the starting point; prints every round's table
  --out FILE     write the last round's shares (JSON as above, plus both rows as the cumulative Q16 table of slab_cum)"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import orbslam2_nmi_amd as nmi
from orbslam2_nmi_amd import synthetic as sy


def flag(name, default=None):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


def cumulative_q16(shares):
    """16 shares -> the 17 cumulative Q16 values of one row of slab_cum."""
    s = np.asarray(shares, np.float64)
    c = np.rint(np.cumsum(s / s.sum()) * 65536).astype(np.int64)
    c[-1] = 65536
    return [0] + [int(x) for x in c]


NOISE = "--noise" in sys.argv   # uniform noise instead of the benchmark's frames: no flat regions, no two lanes on one bin
sys.argv = [x for x in sys.argv if x != "--noise"]
K = int(flag("--k", 0))
SHARES = flag("--shares")
ROUNDS = int(flag("--calibrate", 0))
OUT = flag("--out")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 9
Wn = int(sys.argv[2]) if len(sys.argv) > 2 else 9
w, h = 640, 480
wl = sy.workload(w, h, 27, 27, seed=1234)
rs, ws = torch.from_numpy(wl["render_stack"]).cuda()[:S].contiguous(), torch.from_numpy(wl["warp_stack"]).cuda()[:Wn].contiguous()
if NOISE:
    g = torch.Generator(device="cuda").manual_seed(1)
    rs = torch.randint(0, 256, rs.shape, dtype=torch.uint8, device="cuda", generator=g)
    ws = torch.randint(0, 256, ws.shape, dtype=torch.uint8, device="cuda", generator=g)
names = ["start", "cleared", "hist(wave0)", "B1", "decoded(B2)", "scored", "end", "hist start"]
shares = json.load(open(SHARES)) if SHARES else None
if ROUNDS and not shares:
    sys.exit("--calibrate needs --shares")
row = "later" if K > 0 else "first"


def send_shares(ctx):
    table = np.array([cumulative_q16(shares["first"]), cumulative_q16(shares["later"])], np.uint32)
    ctx.set_option(ctx.OPT_WAVE_SHARES, table.ctypes.data)
    return table


def stamped_launch(ctx, st, n_wg, rep):
    """One stamped search -> the 16 wavefronts' mean pixel-loop end times (us after the stamped candidate's start)."""
    st.zero_()
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    ctx.search_grid(rs, ws)
    ctx.synchronize()
    ms = ctx.last_kernel_ms()
    ctx.set_profiling(False)
    raw = st.cpu().numpy().astype(np.float64)
    a = raw[: n_wg * 8].reshape(n_wg, 8)
    wv = raw[n_wg * 8:].reshape(n_wg, 16)
    live = (a[:, 1] > 0) & (a[:, 3] > 0)
    t0 = a[live, 0].min()
    print(f"launch {rep}: {live.sum()} workgroups, candidate k={K}, stamped kernel {ms * 1e3:.1f} us by HIP events; times from the first workgroup's start")
    for k in (0, 1, 7, 2, 3, 4, 5, 6):
        col = a[live, k]
        col = col[col > 0]
        if col.size:
            print(f"  {names[k]:>12}: mean {np.mean(col - t0) / 100:6.2f} us  min {np.min(col - t0) / 100:6.2f}  max {np.max(col - t0) / 100:6.2f}  (n={col.size})")
    # the stamped candidate's pixels start at "hist start" (wavefront 1's stamp); a library without it stamps the first candidate: "cleared"
    begin = a[live, 7:8] if (a[live, 7] > 0).all() else a[live, 1:2]
    rel = (wv[live] - begin) / 100
    ends = rel.mean(axis=0)
    print("  wavefronts' pixel loops end (us after the candidate's start), mean over workgroups: " + " ".join(f"{x:.1f}" for x in ends))
    srt = np.sort(rel, axis=1)
    print("  ... sorted within each workgroup (1st ... 16th to finish):                       " + " ".join(f"{x:.1f}" for x in srt.mean(axis=0)))
    print(f"  first-to-last spread of the means {ends.max() - ends.min():.2f} us; within a workgroup (mean) {(srt[:, -1] - srt[:, 0]).mean():.2f} us; "
          f"B1 {((a[live, 3:4] - begin) / 100).mean():.2f} us after the candidate's start")
    per = (a[live, 1:7] - a[live, 0:6]) / 100
    print("  per-workgroup phase lengths (mean): " + "  ".join(f"{names[k + 1]} {per[:, k].mean():.2f}" for k in range(6)))
    return ends


with nmi.NmiContext(w, h) as ctx:
    ctx.set_option(ctx.OPT_SPLIT, 0)
    n_wg = min(S * Wn, 256)
    st = torch.zeros((n_wg * 24,), dtype=torch.int64, device="cuda")   # [n_wg][8] phase stamps, then [n_wg][16]: every wavefront's last pixel
    for rep in range(20):
        ctx.search_grid(rs, ws)
    ctx.set_profiling(True)
    d = []
    for rep in range(20):
        ctx.search_grid(rs, ws)
        d.append(ctx.last_kernel_ms())
    ctx.set_profiling(False)
    print(f"{S}x{Wn}: nmi_grid_kernel {np.median(d) * 1e3:.1f} us (HIP events, unstamped, built-in shares)")
    if K:
        ctx.set_option(ctx.OPT_STAMP_CANDIDATE, K)
    ctx.set_option(ctx.OPT_STAMPS, st.data_ptr())
    for rnd in range(ROUNDS + 1):
        if shares:
            table = send_shares(ctx)
            print(f"round {rnd}: shares ({row} row in use for the stamps) first " + " ".join(f"{x:.4f}" for x in shares["first"]) + " | later " + " ".join(f"{x:.4f}" for x in shares["later"]))
        ends = np.mean([stamped_launch(ctx, st, n_wg, rep) for rep in range(3)][1:], axis=0)
        if rnd < ROUNDS:
            new = np.asarray(shares[row], np.float64) * ends.mean() / ends
            shares[row] = [float(x) for x in new / new.sum()]
    ctx.set_option(ctx.OPT_STAMPS, 0)
    if K:
        ctx.set_option(ctx.OPT_STAMP_CANDIDATE, 0)
if OUT and shares:
    shares["slab_cum"] = [cumulative_q16(shares["first"]), cumulative_q16(shares["later"])]
    json.dump(shares, open(OUT, "w"), indent=1)
