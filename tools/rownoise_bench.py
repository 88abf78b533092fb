"""M5 measurement: the row-noise kernels (csrc/rownoise.hip) on whole frames, against a plain device copy of the same frame.
    python tools/rownoise_bench.py [--iters 50] [--no-host] [--out profiles/rownoise_bench.json]

THE EXPECTATION, written down before the first run: the pair of launches moves 12 B per pixel (sums: 4 B in; apply: 4 B in, 4 B out)
against the copy's 8, so it should take at most 1.5 times the copy plus one dependent launch boundary: call it 2 times the copy at most.
(The recorded run, profiles/rownoise_bench.json: 1.61 times the copy at 3000 x 4000 and 1.52 at 4000 x 6000, cold; 1.37 / 1.40 for the pair
launched back to back.  The one-element-per-lane path of misaligned frames is not timed by this tool.)

Two Bayer frames, 3000 x 4000 and 4000 x 6000: synthetic.synth_clean * 0.6 with Poisson-Gaussian noise (K = 4, sigma = 6 DN of 959)
and one offset per sensor row (sigR = 3 DN).  Per frame, one JSON object:
  - sums_us, apply_us, copy_us: medians of event-timed calls after a warm-up of 20, the three ALTERNATED call by call in one loop (the
    same clock, the same neighbours on the machine), with p10 / p90.  sums: yond_rownoise_sums_f32; apply: yond_rownoise_apply_f32 with an
    offsets buffer (per = row, d = 25); copy: torch.Tensor.copy_ device to device of the same frame, the yardstick.  COLD: every call works
    on the next of `copies` frames, more than 600 MB in all, so that a call finds nothing of its input in the 256 MiB Infinity Cache --
    apply therefore reads a frame that its sums launch did not just read.  pair_vs_copy = (sums_us + apply_us) / copy_us;
  - pair_us: both launches back to back on the next frame, one event pair around the two (the dependent launch boundary included);
  - *_warm_us: the same on ONE frame over and over -- the driver's case: a 48 MB frame that the first launch read sits in the Infinity
    Cache for the second;
  - apply_plane_us, apply_inplace_us: per = plane, and out == in;
  - wrapper_ms: rownoise.row_denoise(return_offsets=True) + offsets_report as the drivers call it, host clock around a call that ends in
    the host read of the two numbers;
  - model_host_s: tests/rownoise_model.py row_denoise on one host thread (once, on the 3000 x 4000 frame), and whether the kernel's output
    is within the end-to-end bound of it;
  - sigma_dn, max_dn: the removed offsets' RMS and largest magnitude; clock_mhz: the shader clock before and after (yond_clock_probe)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import __graft_entry__ as G
from yond_public_amd import _lib
from yond_public_amd import rownoise as RN
from yond_public_amd import synthetic as S

DEV = "cuda:0"
SCALE, K, SIGMA, SIG_R = 959.0, 4.0, 6.0, 3.0
SC, SS, D = 10.0 / SCALE, 9.0, 25


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def stats(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 2), [round(float(np.percentile(t, 10)), 2), round(float(np.percentile(t, 90)), 2)]


def timed_alternated(fns, iters, warmup=20):
    """Event times (us) of every function of `fns`, called in turn, round after round."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(max(20, iters))]
    for row in ev:
        for fn, (a, b) in zip(fns, row):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) * 1e3 for a, b in (row[i] for row in ev)] for i in range(len(fns))]


def frame(H, W):
    rng = np.random.default_rng(7)
    clean = S.synth_clean(H, W) * 0.6
    noisy = (rng.poisson(clean * SCALE / K) * K + rng.normal(0.0, SIGMA, clean.shape) + rng.normal(0.0, SIG_R, (H, 1))) / SCALE
    return noisy.astype(np.float32)


def measure(H, W, iters, host):
    lib = _lib.load()
    host_frame = frame(H, W)
    n = H * W
    copies = int(np.ceil(600e6 / (4 * n))) + 1
    frames = [torch.from_numpy(host_frame).to(DEV) for _ in range(copies)]
    out = torch.empty_like(frames[0])
    sums = torch.empty((H, 2), dtype=torch.float64, device=DEV)
    offsets = torch.empty((H, 2), dtype=torch.float64, device=DEV)
    st = _lib.stream()
    turn = [0]

    def nxt(rotate):
        turn[0] = (turn[0] + 1) % copies if rotate else 0
        return frames[turn[0]]

    def f_sums(rotate=True):
        _lib.check(lib.yond_rownoise_sums_f32(_lib.ptr(nxt(rotate)), H, W, _lib.ptr(sums), st), "sums")

    def f_apply(rotate=True, per=0, inplace=False):
        src = nxt(rotate)
        _lib.check(lib.yond_rownoise_apply_f32(_lib.ptr(src), _lib.ptr(src if inplace else out), H, W, _lib.ptr(sums), per, D, SC, SS, _lib.ptr(offsets), st),
                   "apply")

    def f_copy(rotate=True):
        out.copy_(nxt(rotate))

    def f_pair(rotate=True):
        src = nxt(rotate)
        _lib.check(lib.yond_rownoise_sums_f32(_lib.ptr(src), H, W, _lib.ptr(sums), st), "sums")
        _lib.check(lib.yond_rownoise_apply_f32(_lib.ptr(src), _lib.ptr(out), H, W, _lib.ptr(sums), 0, D, SC, SS, _lib.ptr(offsets), st), "apply")

    res = {"shape": [H, W], "pixels": n, "copies": copies}
    f_sums(False)                                            # (apply reads sums of the same values whichever copy it is given)
    ts, ta, tc, tp = timed_alternated([f_sums, f_apply, f_copy, f_pair], iters)
    for key, t in (("sums_us", ts), ("apply_us", ta), ("copy_us", tc), ("pair_us", tp)):
        res[key], res[key + "_p10_p90"] = stats(t)
    res["pair_vs_copy"] = round((res["sums_us"] + res["apply_us"]) / res["copy_us"], 3)
    res["pair_launched_together_vs_copy"] = round(res["pair_us"] / res["copy_us"], 3)
    res["sums_GBs"], res["apply_GBs"], res["copy_GBs"] = (round(b * n / res[k] * 1e-3, 1) for b, k in ((4, "sums_us"), (8, "apply_us"), (8, "copy_us")))
    ts, ta, tc, tp = timed_alternated([lambda: f_sums(False), lambda: f_apply(False), lambda: f_copy(False), lambda: f_pair(False)], iters)
    for key, t in (("sums_warm_us", ts), ("apply_warm_us", ta), ("copy_warm_us", tc), ("pair_warm_us", tp)):
        res[key], res[key + "_p10_p90"] = stats(t)
    res["pair_warm_vs_copy_warm"] = round(res["pair_warm_us"] / res["copy_warm_us"], 3)
    res["apply_plane_us"] = stats(timed_alternated([lambda: f_apply(True, 1)], iters)[0])[0]
    t = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fixed, off = RN.row_denoise(frames[0], sigma_color=SC, sigma_space=SS, d=D, return_offsets=True)
        rep = RN.offsets_report(off, SCALE)
        t.append((time.perf_counter() - t0) * 1e3)
    res["wrapper_ms"] = round(float(np.median(t)), 3)
    res["sigma_dn"], res["max_dn"] = round(rep["sigma"], 4), round(rep["max"], 4)
    if host:
        import rownoise_model as M
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        _, _, z = M.row_denoise(host_frame, M.ROW, D, SC, SS)
        res["model_host_s"] = round(time.perf_counter() - t0, 2)
        got = fixed.cpu().numpy()
        lim = 0.5 * np.spacing(np.abs(got)).astype(np.float64) + M.per_pixel(M.e2e_band(host_frame, M.ROW, D, SC, SS), W)
        res["within_model_bound"] = bool((np.abs(got.astype(np.float64) - z) <= lim).all())
        res["model_host_vs_pair"] = round(res["model_host_s"] * 1e6 / res["pair_us"])
    res["apply_inplace_us"] = stats(timed_alternated([lambda: f_apply(True, 0, True)], iters)[0])[0]      # (last: it changes the frames)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-host", dest="host", action="store_false", default=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rownoise_bench.json"))
    a = ap.parse_args()
    G.build()
    res = {"clock_mhz_before": round(clock_mhz())}
    res["frame_12mp"] = measure(3000, 4000, a.iters, a.host)
    res["frame_24mp"] = measure(4000, 6000, a.iters, False)             # (the host model once, on the smaller frame)
    res["clock_mhz_after"] = round(clock_mhz())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
