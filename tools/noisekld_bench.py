"""M3 measurement: the residual-histogram kernels of the noise-model KLD (yond_noise_hist_f32, yond_pg_noise_hist_f32,
csrc/noisehist.hip) on whole frames, next to the two-step pair the fused kernel replaces and to the reference's expression in NumPy.
    python tools/noisekld_bench.py [--iters 50] [--out profiles/noisekld_bench.json]
Two Bayer frames, 3000 x 4000 and 4000 x 6000: a synthetic scene at 0.6 of full scale and its Poisson-Gaussian realisation (K = 4,
sigma = 6 DN of 959).  Every time is an object {us, p10_p90, clock_mhz}: the median of event-timed launches after a warm-up of 20, and
the shader clock (yond_clock_probe) read right after them.  Per frame:
  - hist_nb1, hist_nb8: yond_noise_hist_f32 with one band and with eight (the entry point's zero-fill of the counts included), each
    launch on the next of `copies` copies of the frame pair -- more than 600 MB in all, so that nothing a launch reads is left in the
    256 MiB Infinity Cache by the launch before; bytes = 8 per pixel, GBs = bytes / time, of_hbm = that rate over HBM_ACHIEVABLE;
  - hist_nb1_warm: the same launch on ONE pair over and over (the driver's case: the frames have just been written);
  - hist_zero_residual: noisy = clean, every pixel of a CFA position in one bin -- the contention case of the LDS histogram;
  - fused: yond_pg_noise_hist_f32 on the rotating clean frames; two_step: yond_pg_noise_f32 into a scratch frame and then
    yond_noise_hist_f32 on it, timed as one pair; fused_vs_two_step = two_step / fused (>= 1: the fused launch is no slower);
    counts_equal: the two give the same integers;
  - numpy_host_ms: the reference's cal_kld expression (two np.histogram calls on the float32 residuals and the finish) on one host
    thread; kld_device / kld_host: the two values."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import __graft_entry__ as G
from yond_public_amd import _lib
from yond_public_amd import noisekld as NK
from yond_public_amd import pgnoise as PG
from yond_public_amd import synthetic as S

DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12          # bytes / s
K, SIGMA, SCALE = 4.0, 6.0, 959.0


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(20, iters))]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return {"us": round(float(np.median(t)), 2), "p10_p90": [round(float(np.percentile(t, 10)), 2), round(float(np.percentile(t, 90)), 2)],
            "clock_mhz": round(clock_mhz())}


def host_kld(p, q):
    """utils/sidd_utils.py:290-304 in NumPy."""
    e = NK.kld_edges()
    hp, hq = np.histogram(p, e)[0] / p.size, np.histogram(q, e)[0] / q.size
    idx = (hp > 0) & (hq > 0)
    hp, hq = hp[idx], hq[idx]
    return float(np.sum(hp * (np.log(hp) - np.log(hq))))


def measure(H, W, iters, host):
    lib = _lib.load()
    st = _lib.stream()
    n = H * W
    clean = torch.from_numpy((S.synth_clean(H, W) * 0.6).astype(np.float32)).to(DEV)
    noisy = PG.add_pg_noise(clean, K, SIGMA, SCALE, 1, [0])
    copies = int(np.ceil(600e6 / (8 * n))) + 1
    cleans, noisys = [clean] + [clean.clone() for _ in range(copies - 1)], [noisy] + [noisy.clone() for _ in range(copies - 1)]
    scratch = torch.empty_like(clean)
    e = NK.kld_edges()
    d_e = torch.from_numpy(e).to(DEV)
    d_t = torch.from_numpy(NK.band_thresholds(8)).to(DEV)
    lo, inv = NK._hint(e)
    counts = torch.empty((8, 4, e.size - 1), dtype=torch.int64, device=DEV)
    items = {k: torch.from_numpy(np.ascontiguousarray(PG.plan(1, K, SIGMA, SCALE, k, [0])).view(np.uint8)).to(DEV) for k in (1, 2)}
    turn = [0]

    def rot(rotate):
        turn[0] = (turn[0] + 1) % copies if rotate else 0
        return turn[0]

    def f_hist(nb=1, rotate=True, zero=False, src=None):
        i = rot(rotate)
        a = src if src is not None else (cleans[i] if zero else noisys[i])
        _lib.check(lib.yond_noise_hist_f32(_lib.ptr(a), _lib.ptr(cleans[i]), 1, H, W, _lib.ptr(d_e), e.size, _lib.ptr(d_t) if nb > 1 else None, nb,
                                           lo, inv, _lib.ptr(counts), st), "hist")

    def f_fused(key=2, rotate=True):
        i = rot(rotate)
        _lib.check(lib.yond_pg_noise_hist_f32(_lib.ptr(cleans[i]), 1, H, W, _lib.ptr(items[key]), 0, _lib.ptr(d_e), e.size, None, 1, lo, inv,
                                              _lib.ptr(counts), st), "fused")

    def f_two(key=2, rotate=True):
        i = rot(rotate)
        _lib.check(lib.yond_pg_noise_f32(_lib.ptr(cleans[i]), _lib.ptr(scratch), n, 1, _lib.ptr(items[key]), 0, st), "pg")
        _lib.check(lib.yond_noise_hist_f32(_lib.ptr(scratch), _lib.ptr(cleans[i]), 1, H, W, _lib.ptr(d_e), e.size, None, 1, lo, inv,
                                           _lib.ptr(counts), st), "hist")

    res = {"shape": [H, W], "hist_bytes": 8 * n, "copies": copies}
    res["hist_nb1"] = timed(f_hist, iters)
    res["hist_nb8"] = timed(lambda: f_hist(8), iters)
    res["hist_nb1_warm"] = timed(lambda: f_hist(rotate=False), iters)
    res["hist_zero_residual"] = timed(lambda: f_hist(zero=True), iters)
    for k in ("hist_nb1", "hist_nb8", "hist_zero_residual"):
        res[k]["GBs"] = round(8 * n / res[k]["us"] * 1e-3, 1)
        res[k]["of_hbm"] = round(8 * n / (res[k]["us"] * 1e-6) / HBM_ACHIEVABLE, 3)
    res["fused"] = timed(f_fused, iters)
    res["two_step"] = timed(f_two, iters)
    res["pg_noise_alone"] = timed(lambda: _lib.check(lib.yond_pg_noise_f32(_lib.ptr(cleans[rot(True)]), _lib.ptr(scratch), n, 1, _lib.ptr(items[2]), 0, st),
                                                     "pg"), iters)
    res["fused_vs_two_step"] = round(res["two_step"]["us"] / res["fused"]["us"], 3)
    f_two(rotate=False)
    two = counts[0].cpu().numpy().copy()
    f_fused(rotate=False)
    q = counts[0].cpu().numpy().copy()
    res["counts_equal"] = bool((two == q).all())
    f_hist(rotate=False)
    p = counts[0].cpu().numpy().copy()
    res["kld_device"] = NK.kld_from_counts(p.sum(0), q.sum(0), n, n)[0]
    if host:
        rp = (noisy - clean).cpu().numpy()
        rq = (PG.add_pg_noise(clean, K, SIGMA, SCALE, 2, [0]) - clean).cpu().numpy()
        t = []
        for _ in range(2):
            t0 = time.perf_counter()
            v = host_kld(rp, rq)
            t.append((time.perf_counter() - t0) * 1e3)
        res["numpy_host_ms"], res["kld_host"] = round(float(np.median(t)), 1), v
        res["numpy_host_vs"] = round(res["numpy_host_ms"] * 1e3 / (res["hist_nb1"]["us"] + res["fused"]["us"]), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-host", dest="host", action="store_false", default=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noisekld_bench.json"))
    a = ap.parse_args()
    G.build()
    torch.set_num_threads(1)
    res = {"hbm_achievable_TBs": HBM_ACHIEVABLE * 1e-12, "clock_mhz_before": round(clock_mhz())}
    res["frame_12mp"] = measure(3000, 4000, a.iters, a.host)
    res["frame_24mp"] = measure(4000, 6000, a.iters, a.host)
    res["clock_mhz_after"] = round(clock_mhz())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
