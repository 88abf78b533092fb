"""I3 measurement: camera-noise synthesis (yond_camera_noise_f32, csrc/camnoise.hip) per noise code, next to the Poisson-Gaussian kernel
(yond_pg_noise_f32, the yardstick) on the same data and to the same model in NumPy / SciPy on one host thread.
    python tools/camnoise_bench.py [--iters 50] [--out profiles/camnoise_bench.json]
Two shapes: one 3472 x 4624 Bayer frame (layout 1) and a training batch 64 x 4 x 128 x 128 (layout 0), both at ratio 100 with
K = 0.22, sigTL = 0.76, sigGs = 1.26, sigR = 0.23, lam = -0.026 DN of a 15871-DN range (a low-ISO full-frame sensor).  Per shape, one
JSON object:
  - pg_us: yond_pg_noise_f32 with (K, sigGs, 1 / ratio); codes.<code>.us: yond_camera_noise_f32 for p, pg, pgr, pgrq -- medians of
    event-timed launches after a warm-up of 20; GBs: the 8 bytes per element (4 in, 4 out) over that time; vs_pg = us / pg_us;
  - codes.<code>.host_ms: the model in NumPy / SciPy (rng.poisson, scipy.stats.tukeylambda.rvs or rng.normal, a normal per row,
    rng.uniform) on one host thread, one run; speedup = host_ms / us;
  - p_equals_pg: code p's output equals the Poisson-Gaussian kernel's bit for bit (the degenerate case);
  - residual_std: standard deviation of noisy - clean per code, device and host, beside the effective Poisson-Gaussian prediction;
  - lambda_max: the largest Poisson mean of the shape; clock_mhz: the shader clock before and after (yond_clock_probe)."""
import argparse
import ctypes as C
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
from yond_public_amd import camnoise as CN
from yond_public_amd import pgnoise as PG
from yond_public_amd import synthetic as S

DEV = "cuda:0"
PARAMS = dict(K=0.22, sigTL=0.76, sigGs=1.26, sigR=0.23, lam=-0.026, wp=16383, bl=512)
SCALE, RATIO = 16383 - 512, 100.0
CODES = ("p", "pg", "pgr", "pgrq")


def clock_mhz():
    out = torch.zeros(2, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def timed(fn, args, iters):
    for _ in range(20):
        _lib.check(fn(*args), "launch")
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(max(20, iters))]
    for a, b in ev:
        a.record()
        fn(*args)
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def host_model(clean, code, rng, row_shape):
    """The model on the host, float64 NumPy / SciPy, in DN at capture and back."""
    from scipy import stats
    p = PARAMS
    y = clean * (SCALE / RATIO)
    z = rng.poisson(y / p['K']) * p['K']
    if 'g' in code:
        z = z + stats.tukeylambda.rvs(p['lam'], scale=p['sigTL'], size=y.shape, random_state=rng)
    else:
        z = z + rng.normal(0.0, p['sigGs'], y.shape)
    if 'r' in code:
        z = z + rng.normal(0.0, p['sigR'], row_shape)
    if 'q' in code:
        z = z + rng.uniform(-0.5, 0.5, y.shape)
    return (z * (RATIO / SCALE)).astype(np.float32)


def measure(clean, layout, iters, host):
    """clean: host float32 [B][...]."""
    B = clean.shape[0]
    n = clean.size // B
    x = torch.from_numpy(clean).to(DEV)
    y = torch.empty_like(x)
    lib = _lib.load()
    slots = np.arange(B)
    pg_items = torch.from_numpy(PG.plan(B, PARAMS['K'], PARAMS['sigGs'], SCALE, 1997, slots, exposure=1 / RATIO).view(np.uint8)).to(DEV)
    pg_us, pg_lo, pg_hi = timed(lib.yond_pg_noise_f32, (_lib.ptr(x), _lib.ptr(y), n, B, C.c_void_p(pg_items.data_ptr()), 0, _lib.stream()), iters)
    y_pg = y.clone()
    res = {"shape": list(clean.shape), "layout": layout, "bytes": 8 * clean.size, "pg_us": round(pg_us, 2), "pg_us_p10_p90": [round(pg_lo, 2), round(pg_hi, 2)],
           "pg_GBs": round(8 * clean.size / pg_us * 1e-3, 1), "lambda_max": float(clean.max() * SCALE / RATIO / PARAMS['K']), "codes": {}}
    row_shape = clean.shape[:-1] + (1,)
    rng = np.random.default_rng(0)
    for code in CODES:
        items = CN.items_for(PARAMS, code, SCALE, 1997, slots, ratio=RATIO)
        d_items = torch.from_numpy(items.view(np.uint8)).to(DEV)
        row_len = clean.shape[-1] if CN.needs_geometry(items) else 0
        us, lo, hi = timed(lib.yond_camera_noise_f32, (_lib.ptr(x), _lib.ptr(y), n, B, C.c_void_p(d_items.data_ptr()), layout, row_len, _lib.stream()),
                           iters)
        K, sig = CN.effective_pg(PARAMS, code)
        r = {"us": round(us, 2), "us_p10_p90": [round(lo, 2), round(hi, 2)], "GBs": round(8 * clean.size / us * 1e-3, 1), "vs_pg": round(us / pg_us, 3),
             "residual_std_device": float((y.double().cpu().numpy() - clean).std()),
             "residual_std_effective_pg": float(np.sqrt((K * clean.astype(np.float64) * SCALE / RATIO + sig * sig).mean()) * RATIO / SCALE)}
        if code == "p":
            res["p_equals_pg"] = bool(torch.equal(y, y_pg))
        if host:
            t0 = time.perf_counter()
            noisy = host_model(clean.astype(np.float64), code, rng, row_shape)
            r["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            r["speedup"] = round(r["host_ms"] * 1e3 / us, 1)
            r["residual_std_host"] = float((noisy.astype(np.float64) - clean).std())
        res["codes"][code] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-host", dest="host", action="store_false", default=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camnoise_bench.json"))
    a = ap.parse_args()
    G.build()
    torch.set_num_threads(1)
    res = {"params": {k: v for k, v in PARAMS.items()}, "ratio": RATIO, "clock_mhz_before": round(clock_mhz())}
    frame = (S.synth_clean(3472, 4624) * 0.6).astype(np.float32)[None]
    res["frame_16mp"] = measure(frame, CN.LAYOUT_BAYER, a.iters, a.host)
    big = S.synth_clean(1024, 2048).astype(np.float32)
    batch = np.stack([np.stack([big[(37 * i) % 768:, (101 * i) % 1792:][c // 2:256 + c // 2:2, c % 2:256 + c % 2:2] for c in range(4)])
                      for i in range(64)])
    assert batch.shape == (64, 4, 128, 128)
    res["train_batch"] = measure(batch, CN.LAYOUT_PLANAR, a.iters, a.host)
    res["clock_mhz_after"] = round(clock_mhz())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
