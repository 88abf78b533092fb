"""R2 / R3 measurement: the raw DN <-> [0, 1] kernels (csrc/rawio.hip) next to K4 in the same process, and what device ingest and
--save cost or gain the full-frame driver end to end.
    timeout 900 python tools/rawio_bench.py [--iters 100] [--driver 16] [--rounds 3] [--out profiles/rawio_bench.json] [--note "..."]
Prints (and writes) one JSON document:
  - kernels, per frame size (3472 x 4624, 4000 x 6000): median of event-timed launches after warm-up of yond_raw_ingest_u16 (2 + 4 B
    per pixel), yond_raw_ingest_f32 (4 + 4), yond_raw_emit_u16 (4 + 2, with the saturation counter) and, interleaved with them,
    yond_denorm_ivst_unpack_f32 (K4, exact inverse, 4 + 4) on a frame of the same size; GB/s each and the ratio to K4's rate;
  - driver (--driver N frames): a temporary tree of N uint16 frames of 3472 x 4624 with gt/, YOND_any (the ANY runfile, one ratio) with
    --host-ingest, with device ingest and with device ingest + --save dn16, ALTERNATED, `rounds` rounds each after one warm-up round;
    frames/s per run, median and spread (max - min) per configuration, speed-up over --host-ingest;
  - notes: what the numbers above need said (a kernel under half of K4's rate, a requirement missed) plus --note."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as G
from yond_public_amd import _lib, rawio

DEV = "cuda:0"


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def kernel_times(H, W, iters):
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(H + W)
    bl, wp, ratio = 64, 1023, 2
    x = torch.rand((H, W), device=DEV, generator=g) * 1.3 - 0.1
    raw_f = (torch.rand((H, W), device=DEV, generator=g) * 1100.0).round()
    raw_u = torch.from_numpy(np.random.default_rng(0).integers(0, 1100, (H, W)).astype(np.uint16)).to(DEV)
    out_f = torch.empty((H, W), device=DEV)
    out_u = torch.empty((H, W), dtype=torch.uint16, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    y4 = torch.rand((H // 2, W // 2, 4), device=DEV, generator=g)
    k4_out = torch.empty((H, W), device=DEV)
    runs = {
        "ingest_u16": (lambda: rawio.ingest(raw_u, bl, wp, ratio, out=out_f), 6),
        "ingest_f32": (lambda: rawio.ingest(raw_f, bl, wp, ratio, out=out_f), 8),
        "emit_u16": (lambda: rawio.emit(x, bl, wp, ratio, out=out_u, count=count), 6),
        "k4_denorm_ivst_unpack": (lambda: _lib.check(lib.yond_denorm_ivst_unpack_f32(
            _lib.ptr(y4), H // 2, W // 2, 0, 0, H // 2, W // 2, _lib.ptr(k4_out), 2, 959.0, 2.0, 8.0, 0.0, 120.0, 1, _lib.stream()), "k4"), 8),
    }
    names = list(runs)
    for _ in range(10):
        for n in names:
            runs[n][0]()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)] for _ in range(iters)]
    for row in ev:
        row[0].record()
        for i, n in enumerate(names):
            runs[n][0]()
            row[i + 1].record()
    torch.cuda.synchronize()
    res = {}
    for i, n in enumerate(names):
        us = float(np.median([row[i].elapsed_time(row[i + 1]) * 1e3 for row in ev]))
        nbytes = H * W * runs[n][1]
        res[n] = {"us": round(us, 2), "bytes": nbytes, "GBs": round(nbytes / us * 1e-3, 1)}
    k4 = res["k4_denorm_ivst_unpack"]["GBs"]
    for n in names[:-1]:
        res[n]["vs_k4"] = round(res[n]["GBs"] / k4, 3)
    return res


def write_tree(root, n, H, W, bl=64, wp=1023):
    """n uint16 frames (+ gt/) of low-light Poisson-Gaussian content; four distinct syntheses, repeated (a 16 MP draw takes ~1 s of NumPy)."""
    from yond_public_amd import synthetic as S
    os.makedirs(os.path.join(root, "gt"))
    made = []
    for j in range(min(4, n)):
        noisy, clean = S.synth_noisy(H, W, 2.0, 8.0, 900 + j)
        made.append((np.clip(np.round(noisy * (wp - bl) + bl), 0, 65535).astype(np.uint16),
                     np.clip(np.round(clean * (wp - bl) + bl), 0, 65535).astype(np.uint16)))
    for k in range(n):
        lr, hr = made[k % len(made)]
        np.save(os.path.join(root, f"f{k:02d}.npy"), lr)
        np.save(os.path.join(root, "gt", f"f{k:02d}.npy"), hr)


def driver_times(n, rounds, H=3472, W=4624):
    import yaml
    from yond_public_amd import YOND_full as Y
    tmp = tempfile.mkdtemp(prefix="rawio_bench_")
    cwd = os.getcwd()
    try:
        frames = os.path.join(tmp, "frames")
        write_tree(frames, n, H, W)
        cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
        for k in ("dst", "dst_eval", "dst_test"):
            cfg[k].update(root_dir=frames, H=H, W=W, ratio_list=[1], bl=64, wp=1023)
        cfg["result_dir"] = os.path.join(tmp, "images")
        rf = os.path.join(tmp, "any.yml")
        with open(rf, "w") as f:
            f.write(yaml.dump(cfg))
        os.chdir(tmp)
        configs = {"host_ingest": ["--host-ingest"], "device_ingest": [], "device_ingest_save_dn16": ["--save", "dn16"]}
        drivers = {k: Y.YOND_Full(["-f", rf, "-m", "eval"] + extra) for k, extra in configs.items()}
        fps = {k: [] for k in configs}
        psnr = {}
        for rnd in range(rounds + 1):                       # round 0: warm-up (plans, buffers, the page cache), not kept
            for k, drv in drivers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                red = drv.eval(-1)["x1"]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert red["count"] == n
                psnr[k] = round(red["psnr_last"], 3)
                if rnd:
                    fps[k].append(n / dt)
        saved = sorted(os.listdir(drivers["device_ingest_save_dn16"].save_dir))
        out = {"frames": n, "H": H, "W": W, "rounds": rounds, "psnr_last": psnr, "saved_files": len(saved)}
        for k, v in fps.items():
            out[k] = {"fps": [round(q, 2) for q in v], "median": round(float(np.median(v)), 2), "spread": round(max(v) - min(v), 2)}
        host = out["host_ingest"]["median"]
        for k in ("device_ingest", "device_ingest_save_dn16"):
            out[k]["vs_host"] = round(out[k]["median"] / host, 3)
        return out
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--driver", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rawio_bench.json"))
    ap.add_argument("--note", action="append", default=[])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rawio_bench needs an MI355X"
    G.build()
    res = {"clock_mhz_before": round(clock_mhz()), "kernels": {}}
    for H, W in ((3472, 4624), (4000, 6000)):
        res["kernels"][f"{H}x{W}"] = kernel_times(H, W, a.iters)
    res["clock_mhz_after"] = round(clock_mhz())
    notes = list(a.note)
    for size, ks in res["kernels"].items():
        for n, r in ks.items():
            if r.get("vs_k4", 1.0) < 0.5:
                notes.append(f"{n} at {size} runs at {r['vs_k4']} of K4's rate")
    if a.driver:
        d = res["driver"] = driver_times(a.driver, a.rounds)
        spread = max(d[k]["spread"] for k in ("host_ingest", "device_ingest"))
        if d["device_ingest"]["median"] < d["host_ingest"]["median"] - spread:
            notes.append("MISSED: device ingest is slower than host ingest beyond the spread of the runs")
        if d["device_ingest_save_dn16"]["median"] < d["host_ingest"]["median"]:
            notes.append("MISSED: --save dn16 drops below the host-ingest rate")
    res["notes"] = notes
    line = json.dumps(res, indent=1)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
