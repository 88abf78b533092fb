"""K7r measurement: the robust noise-level fit (polyfit(ransac=True), csrc/ransac.hip) on one 3000 x 4000 synthetic frame.
    python tools/ransac_bench.py [--iters 5] [--out profiles/ransac_bench.json] [--no-sklearn]
Prints one JSON line:
  - n_selected / n / m: the points below the estimator's threshold (self estimate, k = 29), those kept by the non-saturation rule, and
    min_samples = int(sqrt(n));
  - fit_ms: wall time of the fit on the device maps (compaction -> n -> two exact medians -> per batch of 2, 4, 8, ... trials: subsets
    drawn on the host and uploaded, trial fits, scoring pass, finish, rows back, sklearn's loop on the rows so far -> refit), median of
    --iters runs after one warm-up, every host sync included; rows: the trials it computed; draws_100_ms: the host draw of all 100
    subsets (sklearn.utils.random.sample_without_replacement), of which the fit makes `rows`; compact_us / threshold_us / trials_us:
    the compaction, the two medians and the trial-fit + scoring + finish launches of all 100 trials alone, event-timed;
  - sklearn_ms: RANSACRegressor(min_samples=int(sqrt(n))).fit on [x, 1], y after np.random.seed(2024) -- the call of
    utils/isp_algos.py:354-355 -- on the same points on ONE host thread of the same box (one run), with its inlier count and trials
    next to the device's;
  - round_ms: SimpleNLF (self) per frame with fit 'lsq' and with fit 'ransac', wall time with the final sync, median of --iters: the
    time the robust fit adds to an estimation round;
  - clock_mhz: the shader clock the chip held before and after (yond_clock_probe)."""
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
from yond_public_amd import pipeline as P
from yond_public_amd import synthetic as S

DEV = "cuda:0"


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_bench.json"))
    a = ap.parse_args()
    G.build()
    torch.set_num_threads(1)
    lib = _lib.load()
    res = {"frame": [3000, 4000], "k": 29, "clock_mhz_before": round(clock_mhz())}
    lr = torch.from_numpy(S.synth_noisy(3000, 4000, 4.0, 6.0, 0)[0]).to(DEV)

    # the estimation round with either fit
    lsq_ms, (reg_lsq, info) = wall(lambda: P.SimpleNLF(lr, k=29, setting={'mode': 'self'}, full=True), a.iters)
    rns_ms, (reg_rns, rinfo) = wall(lambda: P.SimpleNLF(lr, k=29, setting={'mode': 'self', 'fit': 'ransac'}, full=True), a.iters)
    ri = rinfo['ransac']
    res.update(n_selected=ri['n_selected'], n=ri['n'], m=ri['m'], thr=float(ri['thr']),
               round_ms={"lsq": round(lsq_ms, 3), "ransac": round(rns_ms, 3), "added": round(rns_ms - lsq_ms, 3)},
               reg_lsq=[float(v) for v in reg_lsq], reg_ransac=[float(v) for v in reg_rns],
               device={"winner": ri['winner'], "n_inliers": ri['n_inliers'], "n_trials": ri['n_trials'], "rows": len(ri['table'])})

    # the fit alone, on the maps of that frame
    lap, mean, var, _ = P.SimpleNLF(lr, k=29, setting={'mode': 'self'}, _maps_only=True)
    lap, mean, var = lap.reshape(-1), mean.reshape(-1), var.reshape(-1)
    th = torch.full((1,), float(info['th']), dtype=torch.float64, device=DEV)
    fit_ms, _ = wall(lambda: P._ransac_fit(lap, mean, var, th, 4), a.iters)
    t0 = time.perf_counter()
    idx = P.ransac_subsets(ri['n'], ri['m'])
    res["fit_ms"] = round(fit_ms, 3)
    res["draws_100_ms"] = round((time.perf_counter() - t0) * 1e3, 3)

    # the launches over all points and trials alone: the compacted points once, then the trials call event-timed
    n, m, T = ri['n'], ri['m'], idx.shape[0]
    x = torch.empty(lap.numel(), dtype=torch.float32, device=DEV)
    y = torch.empty_like(x)
    cnt = torch.empty(3, dtype=torch.int64, device=DEV)
    cws = torch.empty(int(lib.yond_ransac_compact_ws_bytes(lap.numel() // 4)), dtype=torch.uint8, device=DEV)
    st = _lib.stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    _lib.check(lib.yond_ransac_compact_f32(_lib.ptr(lap), _lib.ptr(mean), _lib.ptr(var), lap.numel() // 4, 4, 0, _lib.ptr(th), _lib.ptr(x),
                                           _lib.ptr(y), _lib.ptr(cnt), _lib.ptr(cws), st), "yond_ransac_compact_f32")
    ev[1].record()
    med2 = P._ransac_median2(y, n, lib, st)
    d = torch.empty(n, dtype=torch.float32, device=DEV)
    _lib.check(lib.yond_ransac_absdev_f32(_lib.ptr(y), n, _lib.ptr(med2), _lib.ptr(d), st), "yond_ransac_absdev_f32")
    thr2 = P._ransac_median2(d, n, lib, st)
    ev[2].record()
    idx_dev = torch.from_numpy(idx).to(DEV)
    tab = torch.empty((T, 10), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.yond_ransac_ws_bytes(n, T)), dtype=torch.uint8, device=DEV)
    args = (_lib.ptr(x), _lib.ptr(y), n, _lib.ptr(idx_dev), T, m, _lib.ptr(thr2), _lib.ptr(tab), _lib.ptr(ws), st)
    _lib.check(lib.yond_ransac_trials_f32(*args), "yond_ransac_trials_f32")
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(5, a.iters))]
    for e0, e1 in pairs:
        e0.record()
        lib.yond_ransac_trials_f32(*args)
        e1.record()
    torch.cuda.synchronize()
    assert int(cnt[0]) == n
    res["compact_us"] = round(ev[0].elapsed_time(ev[1]) * 1e3, 1)
    res["threshold_us"] = round(ev[1].elapsed_time(ev[2]) * 1e3, 1)
    res["trials_us"] = round(float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs])), 1)

    if not a.no_sklearn:
        import sklearn.linear_model as lm
        from threadpoolctl import threadpool_limits
        xs, ys = x[:n].cpu().numpy(), y[:n].cpu().numpy()
        X = np.vstack([xs, np.ones(len(xs))]).T
        with threadpool_limits(limits=1):
            np.random.seed(2024)
            t0 = time.perf_counter()
            r = lm.RANSACRegressor(min_samples=int(np.sqrt(len(xs))))
            r.fit(X, ys)
            res["sklearn_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["sklearn"] = {"n_inliers": int(r.inlier_mask_.sum()), "n_trials": int(r.n_trials_),
                          "reg": [float(r.estimator_.coef_[0]), float(r.estimator_.intercept_)]}
        res["speedup_fit"] = round(res["sklearn_ms"] / fit_ms, 1)
    res["clock_mhz_after"] = round(clock_mhz())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
