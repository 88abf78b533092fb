"""M4 measurement: the defective-pixel kernels (csrc/bpc.hip) on whole frames, against a plain device copy of the same frame.
    python tools/bpc_bench.py [--iters 50] [--no-host] [--no-driver] [--out profiles/bpc_bench.json]
Two Bayer frames, 3000 x 4000 and 4000 x 6000: synthetic.synth_clean * 0.6 with Poisson-Gaussian noise (K = 4, sigma = 6 DN of 959)
and 200 isolated defects at the white level.  Per frame, one JSON object:
  - detect_us, copy_us: medians of event-timed calls after a warm-up of 20, the two ALTERNATED call by call in one loop (the same
    clock, the same neighbours on the machine), with p10 / p90.  detect: yond_bpc_detect_repair_f32 with a coordinate buffer of 4096
    (the launch alone: the counts are zeroed outside the timed region and not read); copy: torch.Tensor.copy_ device to device of the same
    frame, the yardstick -- both move 4 B in and 4 B out per pixel.  Every call works on the next of `copies` frames -- more than
    600 MB in all, so that a call finds nothing of its input in the 256 MiB Infinity Cache.  detect_vs_copy = detect_us / copy_us (the
    expectation written down before the first run: at most 2); *_GBs = 8 B per pixel over the time;
  - detect_warm_us, copy_warm_us: the same on ONE frame over and over (the driver's case: the frame has just been written);
  - detect_counts_us: the launch without a coordinate buffer; wrapper_ms: bpc.detect_and_repair as the drivers call it, host clock
    around a call that ends in the host read of the counts;
  - list_1k_us, list_100k_us: yond_bpc_repair_list_f32 for 1,000 and 100,000 listed points (the launch alone; the wrapper adds the
    one device copy, copy_us);
  - hot, cold: the counts of the frame at t = 6 with the true noise model; model_host_s: tests/bpc_model.py detect_and_repair on one
    host thread (once, on the 3000 x 4000 frame), and that the kernel's output and counts equal it;
  - clock_mhz: the shader clock before and after (yond_clock_probe).
driver (3000 x 4000, --synth-noise 4,6, the streamed path): ms per frame of YOND_any with and without --bad-pixels auto, the two runs
alternated twice after one warm-up run each, from the host clock around eval(); auto_step_ms: the added step alone (SimpleNLF, its host
read, the launch, the read of the counts) on a resident frame."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import __graft_entry__ as G
from yond_public_amd import _lib
from yond_public_amd import bpc as BP
from yond_public_amd import synthetic as S

DEV = "cuda:0"
SCALE, K, SIGMA = 959.0, 4.0, 6.0
BETA1, BETA2 = K / SCALE, (SIGMA / SCALE) ** 2


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def stats(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 2), [round(float(np.percentile(t, 10)), 2), round(float(np.percentile(t, 90)), 2)]


def timed_alternated(fns, iters, warmup=20):
    """Event times (us) of every function of `fns`, called in turn, round after round; fn.prep, if set, runs before the first event."""
    prep = [getattr(fn, 'prep', lambda: None) for fn in fns]
    for _ in range(warmup):
        for fn, pre in zip(fns, prep):
            pre()
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(max(20, iters))]
    for row in ev:
        for fn, pre, (a, b) in zip(fns, prep, row):
            pre()
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) * 1e3 for a, b in (row[i] for row in ev)] for i in range(len(fns))]


def frame(H, W):
    rng = np.random.default_rng(7)
    clean = S.synth_clean(H, W) * 0.6
    noisy = ((rng.poisson(clean * SCALE / K) * K + rng.normal(0.0, SIGMA, clean.shape)) / SCALE).astype(np.float32)
    out, truth = BP.inject_defects(torch.from_numpy(noisy), 200, 1, level=1.0)
    return out.numpy(), truth


def measure(H, W, iters, host):
    lib = _lib.load()
    host_frame, truth = frame(H, W)
    n = H * W
    copies = int(np.ceil(600e6 / (4 * n))) + 1
    frames = [torch.from_numpy(host_frame).to(DEV) for _ in range(copies)]
    out = torch.empty_like(frames[0])
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    coords = torch.empty((BP.MAX_SAVED_POINTS, 2), dtype=torch.int32, device=DEV)
    st = _lib.stream()
    turn = [0]

    def nxt(rotate):
        turn[0] = (turn[0] + 1) % copies if rotate else 0
        return frames[turn[0]]

    def f_detect(rotate=True, buf=coords):
        _lib.check(lib.yond_bpc_detect_repair_f32(_lib.ptr(nxt(rotate)), _lib.ptr(out), H, W, BETA1, BETA2, 6.0, _lib.ptr(counts), _lib.ptr(buf),
                                                  BP.MAX_SAVED_POINTS if buf is not None else 0, st), "detect")

    def f_copy(rotate=True):
        out.copy_(nxt(rotate))
    f_detect.prep = counts.zero_                             # the caller zeroes the counts: outside the timed region

    res = {"shape": [H, W], "bytes": 8 * n, "copies": copies, "defects": int(len(truth))}
    td, tc = timed_alternated([f_detect, f_copy], iters)
    res["detect_us"], res["detect_us_p10_p90"] = stats(td)
    res["copy_us"], res["copy_us_p10_p90"] = stats(tc)
    res["detect_vs_copy"] = round(res["detect_us"] / res["copy_us"], 3)
    res["detect_GBs"], res["copy_GBs"] = round(8 * n / res["detect_us"] * 1e-3, 1), round(8 * n / res["copy_us"] * 1e-3, 1)
    td, tc = timed_alternated([lambda: f_detect(False), lambda: f_copy(False)], iters)
    res["detect_warm_us"], res["copy_warm_us"] = stats(td)[0], stats(tc)[0]
    res["detect_counts_us"] = stats(timed_alternated([lambda: f_detect(True, None)], iters)[0])[0]
    for label, npts in (("list_1k_us", 1000), ("list_100k_us", 100000)):
        rng = np.random.default_rng(npts)
        pts = torch.from_numpy(np.stack([rng.integers(0, H, npts), rng.integers(0, W, npts)], axis=1).astype(np.int32)).to(DEV)
        f_copy(False)
        res[label] = stats(timed_alternated([lambda: _lib.check(lib.yond_bpc_repair_list_f32(_lib.ptr(nxt(True)), _lib.ptr(out), H, W, _lib.ptr(pts), npts, st),
                                                                "list")], iters)[0])[0]
    t = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fixed, info = BP.detect_and_repair(frames[0], BETA1, BETA2, 6.0, coords=BP.MAX_SAVED_POINTS)
        t.append((time.perf_counter() - t0) * 1e3)
    res["wrapper_ms"] = round(float(np.median(t)), 3)
    res["hot"], res["cold"] = info["hot"], info["cold"]
    res["found"] = len({tuple(p) for p in truth} & {tuple(p) for p in info["points"]})
    if host:
        import bpc_model as M
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        want, winfo = M.detect_and_repair(host_frame, BETA1, BETA2, 6.0)
        res["model_host_s"] = round(time.perf_counter() - t0, 2)
        res["equals_model"] = bool(np.array_equal(fixed.cpu().numpy(), want) and np.array_equal(info["points"], winfo["points"])
                                   and (info["hot"], info["cold"]) == (winfo["hot"], winfo["cold"]))
        res["model_host_vs"] = round(res["model_host_s"] * 1e6 / res["detect_us"])
    return res


def driver(frames_n=6):
    import yaml
    from yond_public_amd import YOND_full as Y
    from yond_public_amd import pipeline as P
    cfg = yaml.load(open(os.path.join(ROOT, "runfiles", "YOND", "ANY_simple+full_pre_grumix.yml")).read(), Loader=yaml.FullLoader)
    res = {"shape": [3000, 4000], "frames": frames_n}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        for sec in ('dst', 'dst_eval', 'dst_test'):
            cfg[sec].update(root_dir=os.path.join(tmp, "nowhere"), H=3000, W=4000, ratio_list=[1])
        rf = os.path.join(tmp, "any.yml")
        with open(rf, "w") as f:
            f.write(yaml.dump(cfg))
        os.chdir(tmp)
        try:
            base = ['-f', rf, '-m', 'eval', '--synthetic', str(frames_n), '--synth-noise', '4,6']
            runs = {"off": base, "auto": base + ['--bad-pixels', 'auto']}
            ms = {k: [] for k in runs}
            for rnd in range(3):                             # round 0 warms up
                for k, args in runs.items():
                    drv = Y.YOND_Full(args)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    drv.eval(-1)
                    torch.cuda.synchronize()
                    if rnd:
                        ms[k].append((time.perf_counter() - t0) * 1e3 / frames_n)
            res["ms_per_frame_off"], res["ms_per_frame_auto"] = [round(v, 1) for v in ms["off"]], [round(v, 1) for v in ms["auto"]]
            res["added_ms_per_frame"] = round(float(np.mean(ms["auto"]) - np.mean(ms["off"])), 1)
        finally:
            os.chdir(cwd)
    lr = torch.from_numpy(frame(3000, 4000)[0]).to(DEV)
    t = []
    for _ in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        beta1, beta2 = (float(v) for v in P.SimpleNLF(lr, k=29, setting={'mode': 'self'}))
        BP.detect_and_repair(lr, beta1, max(beta2, 0.0), 6.0, coords=BP.MAX_SAVED_POINTS)
        t.append((time.perf_counter() - t0) * 1e3)
    res["auto_step_ms"] = round(float(np.median(t[2:])), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-host", dest="host", action="store_false", default=True)
    ap.add_argument("--no-driver", dest="driver", action="store_false", default=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpc_bench.json"))
    a = ap.parse_args()
    G.build()
    res = {"clock_mhz_before": round(clock_mhz())}
    res["frame_12mp"] = measure(3000, 4000, a.iters, a.host)
    res["frame_24mp"] = measure(4000, 6000, a.iters, False)             # (the host model once, on the smaller frame)
    res["clock_mhz_after"] = round(clock_mhz())
    if a.driver:
        res["driver"] = driver()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
