"""Refined peaks (nmi_refine_peaks, nmi_level_set_refine; csrc/nmi_refine.hip) timed, and the figures written to
profiles/refine/README.md.

Run:      python tools/refine_time.py [--out profiles/refine/README.md] [--json FILE]
Kernel times from the profiler, in a run of its own, then merged into the same file:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/refine_time.py --kernels-only
    python tools/refine_time.py --trace DIR --json FILE --out profiles/refine/README.md      (FILE: the first run's --json)
The latency to the winner of another build of the library (the parent commit's), one process per run, merged the same way:
    NMI_HIP_LIBRARY=/path/to/parent/libnmi_hip.so python tools/refine_time.py --latency-only --json PARENT_1.json
    python tools/refine_time.py --parent PARENT_1.json --parent PARENT_2.json --json FILE --out profiles/refine/README.md
(--like LIKE_1.json adds --latency-only runs of THIS commit's library: the same process shape as the parent's runs, which the main
run's latency rows -- three levels, after the other measurements -- are not.)

What is measured:
  launch    the enqueue-only nmi_refine_peaks (device keys, device records) at K = 1, 4 and 64 on tables of 729 (3^6) and 65,536
            (16x16x16 x 4x2x2) cells, the keys the K best of a top-K, a pair of HIP events around each call (launch included); with
            --trace the profiler's own kernel durations beside it
  level     the replay period, first kernel to last node, of a 729-candidate point-cloud level (848x480): three levels on one
            context -- peaks off, peaks on (K 8, radius 1), peaks and refine on -- replayed in alternating blocks, each block
            between two synchronisations
  latency   nmi_level_run's latency to the winner of the same levels: a host clock around each call, the stream drained before
            each, the levels alternating call by call.  --latency-only measures the peaks-off and peaks-on levels alone, so that it
            runs on a library without refined peaks: the parent's figures, and the spread between its runs, come from there
Warm-up calls come first and are dropped; the timed calls are cut into --reps repetitions: per repetition the median, over the
repetitions their median and their spread (min .. max).  The compiler's resource report of the kernel is taken from hipcc.
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

TABLES = [("729 cells", (3, 3, 3, 3, 3, 3)), ("65,536 cells", (16, 16, 16, 4, 2, 2))]
KS = (1, 4, 64)
RADIUS = (1,) * 6


def stat(us, reps):
    per_rep = [float(np.median(c)) for c in np.array_split(np.asarray(us, float), reps) if len(c)]
    return {"median_of_reps": round(float(np.median(per_rep)), 2), "min_rep": round(min(per_rep), 2), "max_rep": round(max(per_rep), 2),
            "calls": int(len(us))}


def resource_report():
    """{VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy} of nmi_refine_kernel from hipcc's remarks on csrc/nmi_refine.hip."""
    from orbslam2_nmi_amd import build as nmi_build
    src = os.path.join(nmi_build.PKG, "csrc", "nmi_refine.hip")
    r = subprocess.run(["hipcc", *nmi_build.flags(), "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    fields = {"TotalSGPRs": "SGPRs", "VGPRs": "VGPRs", "AGPRs": "AGPRs", "ScratchSize [bytes/lane]": "scratch bytes/lane",
              "Occupancy [waves/SIMD]": "waves/SIMD", "LDS Size [bytes/block]": "LDS bytes", "VGPRs Spill": "VGPR spills",
              "SGPRs Spill": "SGPR spills"}
    out, inside = {}, False
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            inside = "nmi_refine_kernel" in m.group(1)
            continue
        m = re.search(r"remark:\s+(.+?): (\d+)", line)
        if inside and m and m.group(1).strip() in fields:
            out[fields[m.group(1).strip()]] = int(m.group(2))
    return out


def measure_launch(nmi, torch, iters, warmup, reps):
    out = {}
    with nmi.NmiContext(64, 48) as ctx:
        st = torch.cuda.Stream()
        torch.cuda.set_stream(st)
        ctx.set_stream(st.cuda_stream)
        for name, num in TABLES:
            rng = np.random.default_rng(5)
            table = torch.from_numpy(rng.uniform(0, 2, int(np.prod(num))).astype(np.float32)).cuda()
            for K in KS:
                keys = torch.zeros(K, dtype=torch.int64, device="cuda")
                ctx.rank_peaks(table, num, K, (0,) * 6, keys_out=keys)
                records = torch.zeros(K * 152, dtype=torch.uint8, device="cuda")
                call = lambda: ctx.refine_peaks(table, num, keys, records_out=records, blocking=False)
                for _ in range(warmup):
                    call()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
                for e0, e1 in ev:
                    e0.record(st)
                    call()
                    e1.record(st)
                torch.cuda.synchronize()
                out[f"{name}, K {K}"] = stat([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev], reps)
        torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def level_scene(nmi, torch, ctx, w, h):
    from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=3.0)
    B = sy.scene(2 * w, 2 * h, 77)
    nu, nv = int(3 * w * 0.9), int(3 * h * 0.9)
    uu, vv = np.meshgrid(np.linspace(-w, 2 * w, nu), np.linspace(-h, 2 * h, nv))
    xyz = np.stack([(uu - rp.cx) / rp.fx * 10.0, (vv - rp.cy) / rp.fy * 10.0, np.full_like(uu, 10.0)], -1).reshape(-1, 3).astype(np.float32)
    red = (B[np.clip(((vv + h) / 3 * 2).astype(int), 0, 2 * h - 1), np.clip(((uu + w) / 3 * 2).astype(int), 0, 2 * w - 1)].astype(np.float32)
           / np.float32(256)).reshape(-1)
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, 1] = [0, -1, 0]
    pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
    g = H.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
    cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
    mvps = np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
    homs = capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
    frame = torch.flip(ctx.render_points(dx, torch.sqrt(dr), capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None], 3.0)[0], dims=[0]).contiguous()
    return dx, dr, frame, mvps, homs


def measure_level(nmi, torch, iters, warmup, reps, with_refine, block=50):
    """-> (replay periods, latencies to the winner) of the levels peaks_off, peaks_on and, with_refine, refine_on."""
    w, h = 848, 480
    with nmi.NmiContext(w, h) as ctx:
        dx, dr, frame, mvps, homs = level_scene(nmi, torch, ctx, w, h)
        names = ["peaks_off", "peaks_on"] + (["refine_on"] if with_refine else [])
        levels = [nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0) for _ in names]
        try:
            for name, lv in zip(names, levels):
                if name != "peaks_off":
                    lv.set_peaks(8, (3,) * 6, RADIUS)
                if name == "refine_on":
                    lv.set_refine(True)
            replay = {name: lv.bind(mvps, homs) for name, lv in zip(names, levels)}
            period = {k: [] for k in replay}
            for i in range((warmup + iters) // block):
                for name, fn in replay.items():
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(block):
                        fn()
                    ctx.synchronize()
                    if i * block >= warmup:
                        period[name].append((time.perf_counter() - t0) * 1e6 / block)
            latency = {k: [] for k in replay}
            for i in range(warmup + iters):
                for name, fn in replay.items():
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e6
                    if i >= warmup:
                        latency[name].append(dt)
            winners = {name: fn() for name, fn in replay.items()}
            assert len(set(winners.values())) == 1, winners
        finally:
            for lv in levels:
                lv.close()
        p = {k: stat(v, reps) for k, v in period.items()}
        p["replays_per_timed_block"] = block
        return p, {k: stat(v, reps) for k, v in latency.items()}


def read_trace(directory, reps, warm_share):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if "nmi_refine_kernel" in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3,
                                 int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // 64))
    rows.sort()
    out = {}
    # the launches come in measure_launch's order: per table, per K, warm-up then timed calls; K is the grid's workgroup count
    order = [f"{name}, K {K}" for name, _ in TABLES for K in KS]
    runs, last = [], None
    for _, us, K in rows:
        if K != last:
            runs.append([])
            last = K
        runs[-1].append(us)
    if len(runs) != len(order):
        raise SystemExit(f"the trace holds {len(runs)} runs of nmi_refine_kernel, not the {len(order)} of measure_launch")
    for name, us in zip(order, runs):
        out[name] = stat(us[int(round(len(us) * warm_share)):], reps)   # (the first warmup / (warmup + iters) of a run: warm-up)
    return out


def fmt(s):
    return f"{s['median_of_reps']} ({s['min_rep']} .. {s['max_rep']})"


def write_readme(path, res):
    L = ["# Refined peaks: timings", "",
         "Written by `tools/refine_time.py` (its docstring says what each figure is and how it is taken).  Microseconds; median over",
         f"the repetitions of the per-repetition medians, with the spread of the repetitions (min .. max).  Device: {res.get('device', 'not recorded')}.", ""]
    L += ["## The launch alone", "", "| table, K | events around the enqueue-only call | profiler: kernel duration |", "|---|---|---|"]
    for name, s in res.get("launch", {}).items():
        tr = res.get("trace", {}).get(name)
        L.append(f"| {name} | {fmt(s)} | {fmt(tr) if tr else 'not measured'} |")
    if "level" in res:
        lv = res["level"]
        d = lambda a, b: round(lv[a]["median_of_reps"] - lv[b]["median_of_reps"], 2)
        L += ["", "## A level's replay: peaks off, peaks on, peaks and refine on", "",
              "Replay period of a 729-candidate point-cloud level at 848x480 (`nmi_level_run` back to back, blocks of "
              f"{lv['replays_per_timed_block']} replays between two synchronisations, the levels alternating).", "",
              "| peaks off | peaks on (K 8, radius 1) | peaks and refine on | refine's share |", "|---|---|---|---|",
              f"| {fmt(lv['peaks_off'])} | {fmt(lv['peaks_on'])} | {fmt(lv['refine_on'])} | {d('refine_on', 'peaks_on')} |"]
    if "latency" in res:
        la = res["latency"]
        L += ["", "## nmi_level_run: latency to the winner", "",
              "Host clock around each call, the stream drained before it, the levels alternating call by call.  The first row is the main",
              "run's (three levels on the context, after the other measurements).  The others are runs of this tool with",
              "`--latency-only` (two levels, nothing before them), one process each, on this commit's library and on the parent",
              "commit's: the parent's runs differ by their run-to-run spread, which a change has to stay within.", "",
              "| library | peaks off | peaks on | peaks and refine on |", "|---|---|---|---|",
              f"| this commit | {fmt(la['peaks_off'])} | {fmt(la['peaks_on'])} | {fmt(la['refine_on']) if 'refine_on' in la else 'not measured'} |"]
        for i, p in enumerate(res.get("like_latency", [])):
            L.append(f"| this commit, `--latency-only` run {i + 1} | {fmt(p['peaks_off'])} | {fmt(p['peaks_on'])} | -- |")
        for i, p in enumerate(res.get("parent_latency", [])):
            L.append(f"| parent, run {i + 1} | {fmt(p['peaks_off'])} | {fmt(p['peaks_on'])} | -- |")
    if res.get("resources"):
        r = res["resources"]
        L += ["", "## Compiler resource report (gfx950)", "",
              "| kernel | VGPRs | AGPRs | SGPRs | scratch bytes/lane | VGPR spills | SGPR spills | LDS bytes | waves/SIMD |", "|---|---|---|---|---|---|---|---|---|",
              f"| nmi_refine_kernel | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('SGPRs')} | {r.get('scratch bytes/lane')} | {r.get('VGPR spills')} | "
              f"{r.get('SGPR spills')} | {r.get('LDS bytes')} | {r.get('waves/SIMD')} |"]
    for note in res.get("notes", []):
        L += ["", note]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000, help="timed calls of each form")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine", "README.md"))
    ap.add_argument("--json", help="keep the figures here (and, with --trace or --parent, read them from here)")
    ap.add_argument("--kernels-only", action="store_true", help="only the enqueue-only calls (the run under the profiler)")
    ap.add_argument("--latency-only", action="store_true", help="only the latency to the winner, without refined peaks (another build of the library)")
    ap.add_argument("--trace", help="read a rocprofv3 --kernel-trace directory and merge its kernel durations into --json's figures")
    ap.add_argument("--parent", action="append", default=[], help="a --latency-only run's --json of the parent commit's library; merged into --json's figures")
    ap.add_argument("--like", action="append", default=[], help="a --latency-only run's --json of THIS commit's library: the like-for-like rows beside the parent's")
    ap.add_argument("--note", action="append", default=[], help="a paragraph for the end of the file (what the figures were found to mean)")
    a = ap.parse_args()
    if a.trace or a.parent or a.like:
        res = json.load(open(a.json)) if a.json and os.path.exists(a.json) else {}
        if a.trace:
            warmup, iters = res.get("warmup", a.warmup), res.get("iters", a.iters)   # (those of the run that --json kept)
            res["trace"] = read_trace(a.trace, a.reps, warmup / float(warmup + iters))
        if a.like:
            res["like_latency"] = [json.load(open(p))["latency"] for p in a.like]
        if a.parent:
            res["parent_latency"] = [json.load(open(p))["latency"] for p in a.parent]
    else:
        import torch
        import orbslam2_nmi_amd as nmi
        if not torch.cuda.is_available():
            raise SystemExit("refine_time.py needs a HIP device: nothing here can be measured without one")
        nmi.load_library()
        res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "reps": a.reps}
        if a.latency_only:
            res["latency"] = measure_level(nmi, torch, a.iters, a.warmup, a.reps, with_refine=False)[1]
        else:
            res["launch"] = measure_launch(nmi, torch, a.iters, a.warmup, a.reps)
            if not a.kernels_only:
                res["level"], res["latency"] = measure_level(nmi, torch, a.iters, a.warmup, a.reps, with_refine=True)
                res["resources"] = resource_report()
    if a.note:
        res["notes"] = a.note
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not (a.kernels_only or a.latency_only):
        write_readme(a.out, res)


if __name__ == "__main__":
    main()
