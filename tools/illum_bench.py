"""M2 measurement: the illuminance correction (yond_illum_sums_f32 + yond_illum_apply_f32, csrc/illum.hip) on whole frames, next to the
same expression in torch on the same GPU and in torch on one host thread.
    python tools/illum_bench.py [--iters 50] [--out profiles/illum_bench.json]
Two Bayer frames, 3000 x 4000 and 4000 x 6000: a synthetic scene with 5 % of the targets saturated and a prediction that is the scene
at 1 / 1.1 of its brightness plus an offset.  Per frame, one JSON object:
  - sums_us, apply_us: medians of event-timed launches after a warm-up of 20 (sums: the partials' launch and the one-workgroup finish
    together, as the entry point issues them), with p10 / p90, each launch on the next of `copies` copies of the frame pair -- more than
    600 MB in all, so that nothing a launch reads is left in the 256 MiB Infinity Cache by the launch before; *_bytes: what the launch
    must move (8 B per pixel read; 4 B read and 4 B written); *_GBs = bytes / time; *_of_hbm = that rate over HBM_ACHIEVABLE, the
    6.3 TB/s DESIGN.md uses;
  - sums_warm_us, apply_warm_us: the same launches on ONE pair, over and over (what fits the Infinity Cache is served from it: the
    driver's case, whose frame the denoiser has just written);
  - layouts: sums_us of the FLAT and PACKED4 layouts on the same data, apply_us of mode cfa and of the in-place call;
  - torch_gpu_us: p = clamp(pred, 0, 1); m = source != 1; gain = dot(p[m], source[m]) / dot(p[m], p[m]); out = gain.item() * p -- the
    reference's expression with the host read of the gain, event-timed the same way; torch_gpu_vs = torch_gpu_us / (sums_us + apply_us);
  - torch_host_ms: the same on one host thread (median of 3); gain_device / gain_torch_gpu / gain_host: the three gains;
  - clock_mhz: the shader clock before and after (yond_clock_probe)."""
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
from yond_public_amd import illum as I
from yond_public_amd import synthetic as S

DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12          # bytes / s


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
    return round(float(np.median(t)), 2), [round(float(np.percentile(t, 10)), 2), round(float(np.percentile(t, 90)), 2)]


def torch_expression(pred, source):
    p = torch.clamp(pred, 0, 1)
    m = source != 1
    pc, sc = p[m], source[m]
    gain = (torch.dot(pc, sc) / torch.dot(pc, pc)).item()          # the host read
    return gain * p, gain


def frame_pair(H, W):
    scene = S.synth_clean(H, W).astype(np.float32)
    source = np.clip(scene * np.float32(1.0 / np.quantile(scene, 0.95)), 0, 1).astype(np.float32)      # 5 % saturated
    rng = np.random.default_rng(7)
    pred = (source / np.float32(1.1) + np.float32(0.004) + rng.normal(0, 0.01, source.shape)).astype(np.float32)
    return pred, source


def measure(H, W, iters, host):
    lib = _lib.load()
    pred_h, source_h = frame_pair(H, W)
    pred, source = torch.from_numpy(pred_h).to(DEV), torch.from_numpy(source_h).to(DEV)
    n = pred.numel()
    copies = int(np.ceil(600e6 / (8 * n))) + 1
    preds, sources = [pred] + [pred.clone() for _ in range(copies - 1)], [source] + [source.clone() for _ in range(copies - 1)]
    turn = [0]
    sums = torch.empty((5, 3), dtype=torch.float64, device=DEV)
    ws = torch.empty(lib.yond_illum_ws_bytes() // 8, dtype=torch.float64, device=DEV)
    st = _lib.stream()

    def f_sums(layout=0, width=W, rotate=True):
        turn[0] = (turn[0] + 1) % copies if rotate else 0
        _lib.check(lib.yond_illum_sums_f32(_lib.ptr(preds[turn[0]]), _lib.ptr(sources[turn[0]]), n, width, layout, _lib.ptr(sums), _lib.ptr(ws), st), "sums")

    def f_apply(mode=0, rotate=True):
        turn[0] = (turn[0] + 1) % copies if rotate else 0               # (the output is the next turn's source: every byte written is evicted too)
        _lib.check(lib.yond_illum_apply_f32(_lib.ptr(preds[turn[0]]), n, W, 0, _lib.ptr(sums), mode, 1, _lib.ptr(sources[(turn[0] + 1) % copies]), st), "apply")

    res = {"shape": [H, W], "saturated_fraction": round(float((source_h == 1).mean()), 4), "sums_bytes": 8 * n, "apply_bytes": 8 * n, "copies": copies}
    res["sums_us"], res["sums_us_p10_p90"] = timed(f_sums, iters)
    res["sums_warm_us"] = timed(lambda: f_sums(rotate=False), iters)[0]
    res["layouts"] = {"sums_flat_us": timed(lambda: f_sums(2, 0), iters)[0], "sums_packed4_us": timed(lambda: f_sums(1, 0), iters)[0]}
    f_sums(rotate=False)
    res["gain_device"] = I.gains(sums)[0]
    res["torch_gpu_us"], res["torch_gpu_us_p10_p90"] = timed(lambda: torch_expression(pred, source), iters, warmup=5)
    res["gain_torch_gpu"] = torch_expression(pred, source)[1]
    # the apply launches last: they overwrite the copies of the target
    res["apply_us"], res["apply_us_p10_p90"] = timed(f_apply, iters)
    res["apply_warm_us"] = timed(lambda: f_apply(rotate=False), iters)[0]
    res["layouts"]["apply_cfa_us"] = timed(lambda: f_apply(1), iters)[0]
    for k in ("sums", "apply"):
        res[f"{k}_GBs"] = round(8 * n / res[f"{k}_us"] * 1e-3, 1)
        res[f"{k}_of_hbm"] = round(8 * n / (res[f"{k}_us"] * 1e-6) / HBM_ACHIEVABLE, 3)
    scratch = pred.clone()
    res["layouts"]["apply_in_place_us"] = timed(lambda: _lib.check(lib.yond_illum_apply_f32(_lib.ptr(scratch), n, W, 0, _lib.ptr(sums), 0, 1, _lib.ptr(scratch),
                                                                                             st), "apply"), iters)[0]
    res["torch_gpu_vs"] = round(res["torch_gpu_us"] / (res["sums_us"] + res["apply_us"]), 1)
    del preds, sources
    if host:
        tp, ts = torch.from_numpy(pred_h), torch.from_numpy(source_h)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            _, g = torch_expression(tp, ts)
            t.append((time.perf_counter() - t0) * 1e3)
        res["torch_host_ms"], res["gain_host"] = round(float(np.median(t)), 1), g
        res["torch_host_vs"] = round(res["torch_host_ms"] * 1e3 / (res["sums_us"] + res["apply_us"]), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-host", dest="host", action="store_false", default=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "illum_bench.json"))
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
