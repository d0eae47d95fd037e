"""Ranked peaks (nmi_rank_peaks, nmi_level_set_peaks; csrc/nmi_peaks.hip) timed, and the figures written to
profiles/peaks/README.md.

Run:      python tools/peaks_time.py [--out profiles/peaks/README.md] [--json FILE]
Kernel times from the profiler, in a run of its own, then merged into the same file:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/peaks_time.py --kernels-only
    python tools/peaks_time.py --trace DIR --json FILE --out profiles/peaks/README.md      (FILE: the first run's --json)

What is measured, at (729 cells = 3^6, K 8, radius 1) and (32,768 cells = 8x8x8 x 4x4x4, K 16, radius 1):
  kernel    the enqueue-only nmi_rank_peaks on the table of a real search, a pair of HIP events around each call (launch included);
            with --trace the profiler's own kernel durations beside it
  blocking  in one process, alternating call by call, a host clock around each, every call's arguments converted beforehand:
              device route   nmi_search_grid with d_ratings, nmi_rank_peaks with h_keys (the K keys read back)
              host route     the same search, hipMemcpy of the table to the host, nmi_find_peaks there
  level     the replay period of a 729-candidate point-cloud level (848x480) with peaks on and off: two levels on one context,
            replayed in alternating blocks
Warm-up calls come first and are dropped; the timed calls are cut into --reps repetitions: per repetition the median, over the
repetitions their median and their spread (min .. max).  The compiler's resource report of the kernel is taken from hipcc.
"""
import argparse
import csv
import ctypes as C
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

SHAPES = [{"name": "729 cells, K 8, radius 1", "num": (3, 3, 3, 3, 3, 3), "K": 8, "frame": (640, 480)},
          {"name": "32,768 cells, K 16, radius 1", "num": (8, 8, 8, 4, 4, 4), "K": 16, "frame": (160, 120)}]
RADIUS = (1,) * 6


def stat(us, reps):
    per_rep = [float(np.median(c)) for c in np.array_split(np.asarray(us, float), reps) if len(c)]
    return {"median_of_reps": round(float(np.median(per_rep)), 2), "min_rep": round(min(per_rep), 2), "max_rep": round(max(per_rep), 2),
            "calls": int(len(us))}


def resource_report():
    """{kernel instance: {VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy}} from hipcc's remarks on csrc/nmi_peaks.hip."""
    from orbslam2_nmi_amd import build as nmi_build
    src = os.path.join(nmi_build.PKG, "csrc", "nmi_peaks.hip")
    r = subprocess.run(["hipcc", *nmi_build.flags(), "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    out, cur = {}, None
    fields = {"TotalSGPRs": "SGPRs", "VGPRs": "VGPRs", "AGPRs": "AGPRs", "ScratchSize [bytes/lane]": "scratch bytes/lane",
              "Occupancy [waves/SIMD]": "waves/SIMD", "LDS Size [bytes/block]": "LDS bytes"}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            inst = re.search(r"nmi_peaks_kernelILi(\d+)E", m.group(1))
            cur = f"nmi_peaks_kernel<{inst.group(1)}>" if inst else None
            if cur:
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+)", line)
        if cur and m and m.group(1).strip() in fields:
            out[cur][fields[m.group(1).strip()]] = int(m.group(2))
    return out


def search_setup(nmi, torch, shape):
    from orbslam2_nmi_amd import synthetic as sy
    w, h = shape["frame"]
    num = shape["num"]
    S, Wn = int(np.prod(num[:3])), int(np.prod(num[3:]))
    wl = sy.workload(w, h, S, Wn, seed=41)
    ctx = nmi.NmiContext(w, h, render_bottom_up=wl["bottom_up"])
    rs, ws = torch.from_numpy(wl["render_stack"]).cuda(), torch.from_numpy(wl["warp_stack"]).cuda()
    ratings = torch.zeros((Wn, S), dtype=torch.float32, device="cuda")
    return ctx, rs, ws, ratings


def measure_kernel(nmi, torch, shape, iters, warmup, reps):
    ctx, rs, ws, ratings = search_setup(nmi, torch, shape)
    with ctx:
        st = torch.cuda.Stream()
        torch.cuda.set_stream(st)
        ctx.set_stream(st.cuda_stream)
        ctx.search_grid(rs, ws, ratings)
        keys = torch.zeros(shape["K"], dtype=torch.int64, device="cuda")
        call = lambda: ctx.rank_peaks(ratings, shape["num"], shape["K"], RADIUS, keys_out=keys, blocking=False)
        for _ in range(warmup):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            e0.record(st)
            call()
            e1.record(st)
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream())
        return stat([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev], reps)


def measure_blocking(nmi, torch, shape, iters, warmup, reps):
    from orbslam2_nmi_amd import hostapi
    ctx, rs, ws, ratings = search_setup(nmi, torch, shape)
    num, K = shape["num"], shape["K"]
    with ctx:
        # every call bound once (bind_search's reason): the interpreter converts no argument inside the timed region
        search = ctx.bind_search(rs, ws, ratings)
        rank, dev_keys = ctx.bind_rank_peaks(ratings, num, K, RADIUS)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        host_table, host_keys = np.empty(ratings.numel(), np.float32), np.zeros(K, np.uint64)
        dst, src, nbytes = C.c_void_p(host_table.ctypes.data), C.c_void_p(ratings.data_ptr()), C.c_size_t(host_table.nbytes)
        find = hostapi._lib().nmi_find_peaks
        pt, pk = host_table.ctypes.data_as(C.POINTER(C.c_float)), host_keys.ctypes.data_as(C.POINTER(C.c_uint64))
        num6, rad6, cK = (C.c_int32 * 6)(*num), (C.c_int32 * 6)(*RADIUS), C.c_int32(K)

        def device_route():
            search()
            return rank()

        def host_route():
            search()
            if hip.hipMemcpy(dst, src, nbytes, 2) != 0:    # hipMemcpyDeviceToHost of the whole table, blocking
                raise RuntimeError("hipMemcpy failed")
            return find(pt, num6, cK, rad6, pk)

        a, b = device_route(), host_route()
        assert a == b and dev_keys.tolist() == host_keys.tolist(), "the two routes disagree"
        times = {"device": [], "host": [], "search_alone": []}
        for i in range(warmup + iters):
            for name, fn in (("device", device_route), ("host", host_route), ("search_alone", search)):
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e6
                if i >= warmup:
                    times[name].append(dt)
        return {k: stat(v, reps) for k, v in times.items()}


def measure_level(nmi, torch, iters, warmup, reps, block=50):
    from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy
    w, h = 848, 480
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
    with nmi.NmiContext(w, h) as ctx:
        dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
        frame = torch.flip(ctx.render_points(dx, torch.sqrt(dr), capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None], 3.0)[0], dims=[0]).contiguous()
        with nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0) as on, nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0) as off:
            on.set_peaks(8, (3,) * 6, RADIUS)
            replay = {"peaks_on": on.bind(mvps, homs), "peaks_off": off.bind(mvps, homs)}
            times = {k: [] for k in replay}
            for i in range((warmup + iters) // block):
                for name, fn in replay.items():
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(block):
                        fn()
                    ctx.synchronize()
                    if i * block >= warmup:
                        times[name].append((time.perf_counter() - t0) * 1e6 / block)
            assert replay["peaks_on"]() == replay["peaks_off"]()
            keys, count = on.copy_peaks()
        out = {k: stat(v, reps) for k, v in times.items()}
        out["replays_per_timed_block"] = block
        out["peaks_found"] = count
        return out


def read_trace(directory, reps):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    per_kernel = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"nmi_peaks_kernel<(\d+)>", row["Kernel_Name"])
                if m:
                    per_kernel.setdefault(f"nmi_peaks_kernel<{m.group(1)}>", []).append(
                        (int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    out = {}
    for name, rows in per_kernel.items():
        rows.sort()
        us = [d for _, d in rows]
        out[name] = stat(us[len(us) // 5:], reps)   # (the first fifth: warm-up)
    return out


def fmt(s):
    return f"{s['median_of_reps']} ({s['min_rep']} .. {s['max_rep']})"


def write_readme(path, res):
    L = ["# Ranked peaks: timings", "",
         "Written by `tools/peaks_time.py` (its docstring says what each figure is and how it is taken).  Microseconds; median over",
         f"the repetitions of the per-repetition medians, with the spread of the repetitions (min .. max).  Device: {res.get('device', 'not recorded')}.", ""]
    L += ["## The kernel", "",
          "| shape | events around the enqueue-only call | profiler: kernel duration |", "|---|---|---|"]
    inst = {"729 cells, K 8, radius 1": "nmi_peaks_kernel<1>", "32,768 cells, K 16, radius 1": "nmi_peaks_kernel<64>"}
    for name, s in res.get("kernel", {}).items():
        tr = res.get("trace", {}).get(inst.get(name, ""))
        L.append(f"| {name} | {fmt(s)} | {fmt(tr) + ' (' + inst[name] + ')' if tr else 'not measured'} |")
    L += ["", "## Blocking: device route against the host route", "",
          "Device route: `nmi_search_grid` with `d_ratings`, then `nmi_rank_peaks` with the keys read back.  Host route: the same",
          "search, a copy of the table to the host, `nmi_find_peaks` there.  Host clock around each, the routes alternating.", "",
          "| shape (frame) | device route | host route | the search alone | faster |", "|---|---|---|---|---|"]
    for name, b in res.get("blocking", {}).items():
        faster = "device" if b["device"]["median_of_reps"] < b["host"]["median_of_reps"] else "host"
        L.append(f"| {name} ({b['frame'][0]}x{b['frame'][1]}) | {fmt(b['device'])} | {fmt(b['host'])} | {fmt(b['search_alone'])} | {faster} |")
    if "level" in res:
        lv = res["level"]
        d = round(lv["peaks_on"]["median_of_reps"] - lv["peaks_off"]["median_of_reps"], 2)
        L += ["", "## A level with peaks on and off", "",
              "Replay period of a 729-candidate point-cloud level at 848x480 (`nmi_level_run` back to back, blocks of "
              f"{lv['replays_per_timed_block']} replays, the two levels alternating).", "",
              "| peaks off | peaks on (K 8, radius 1) | difference |", "|---|---|---|",
              f"| {fmt(lv['peaks_off'])} | {fmt(lv['peaks_on'])} | {d} |"]
    if res.get("resources"):
        L += ["", "## Compiler resource report (gfx950)", "",
              "| kernel instance (cells per lane) | VGPRs | AGPRs | SGPRs | scratch bytes/lane | LDS bytes | waves/SIMD |", "|---|---|---|---|---|---|---|"]
        for k, r in sorted(res["resources"].items(), key=lambda kv: int(re.search(r"<(\d+)>", kv[0]).group(1))):
            L.append(f"| {k} | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('SGPRs')} | {r.get('scratch bytes/lane')} | {r.get('LDS bytes')} | {r.get('waves/SIMD')} |")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "peaks", "README.md"))
    ap.add_argument("--json", help="keep the figures here (and, with --trace, read them from here)")
    ap.add_argument("--kernels-only", action="store_true", help="only the enqueue-only calls (the run under the profiler)")
    ap.add_argument("--trace", help="read a rocprofv3 --kernel-trace directory and merge its kernel durations into --json's figures")
    ap.add_argument("--note", action="append", default=[], help="a paragraph for the end of the file (what the figures were found to mean)")
    a = ap.parse_args()
    if a.trace:
        res = json.load(open(a.json)) if a.json and os.path.exists(a.json) else {}
        res["trace"] = read_trace(a.trace, a.reps)
    else:
        import torch
        import orbslam2_nmi_amd as nmi
        if not torch.cuda.is_available():
            raise SystemExit("peaks_time.py needs a HIP device: nothing here can be measured without one")
        nmi.load_library()
        res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "reps": a.reps, "kernel": {}, "blocking": {}}
        for shape in SHAPES:
            res["kernel"][shape["name"]] = measure_kernel(nmi, torch, shape, a.iters, a.warmup, a.reps)
        if not a.kernels_only:
            for shape in SHAPES:
                big = shape["num"] != (3,) * 6
                b = measure_blocking(nmi, torch, shape, a.iters // 10 if big else a.iters, a.warmup // 10 if big else a.warmup, a.reps)
                b["frame"] = list(shape["frame"])
                res["blocking"][shape["name"]] = b
            res["level"] = measure_level(nmi, torch, a.iters, a.warmup, a.reps)
            res["resources"] = resource_report()
    if a.note:
        res["notes"] = a.note
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not a.kernels_only:
        write_readme(a.out, res)


if __name__ == "__main__":
    main()
