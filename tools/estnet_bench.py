"""Measure the estimation network EstUnet (default settings: depth 3, nf 64, 'add', 'std', pge; out_nc 2) on the HIP kernels.

    python tools/estnet_bench.py [--out profiles/estnet_bench.json] [--iters 30] [--shapes 1x3000x4000,1x256x8192,32x256x256]

Per shape: ms per estimate (HIP events around plan.forward, after warm-up, median of --iters), the algorithmic TFLOP of one forward
(EstimatorPlan.flops: real channels), TF/s, the clock the chip held inside the split-operand convolutions (in-kernel counters) and,
from one extra forward with an event pair around every launch, the time and rate per layer kind -- for the memory-bound edge
launches (yond_est_conv_in_f32, yond_est_head_f32, the pooling) also their algorithmic HBM bytes and TB/s.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import estnet_common as E  # noqa: E402


def bench_shape(N, H, W, iters):
    net = E.build(E.MEAN_ARGS, E.weights(E.MEAN_ARGS, 7), "cuda")
    x = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, (N, H, W)).astype(np.float32)).cuda()
    plan = net.plan(x.device)
    for _ in range(3):
        plan.forward(x)
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.forward(x)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    # in-kernel clock of the split-operand launches over a few forwards
    plan.clk = torch.zeros(2, dtype=torch.int64, device=x.device)
    for _ in range(5):
        plan.forward(x)
    torch.cuda.synchronize()
    c = plan.clk.cpu().numpy()
    plan.clk = None
    mhz = float(c[0]) / float(c[1]) * 100.0 if c[1] else None
    # one forward with an event pair around every convolution launch
    plan.prof, plan.prof_bytes = [], {}
    plan.forward(x)
    torch.cuda.synchronize()
    layers = {}
    for tag, flops, a, b in plan.prof:
        d = layers.setdefault(tag, {'launches': 0, 'ms': 0.0, 'tflop': 0.0})
        d['launches'] += 1
        d['ms'] += a.elapsed_time(b)
        d['tflop'] += flops / 1e12
    plan.prof = None
    for tag, d in layers.items():
        d['tflops_per_s'] = d['tflop'] / (d['ms'] / 1e3) if d['ms'] else None
        if tag in plan.prof_bytes:                          # the memory-bound edge launches: algorithmic HBM bytes and their rate
            d['gb'] = plan.prof_bytes[tag] / 1e9
            d['tb_per_s'] = d['gb'] / 1e3 / (d['ms'] / 1e3) if d['ms'] else None
    timed_ms = sum(d['ms'] for d in layers.values())
    tflop = plan.flops(N, H, W) / 1e12
    med = float(np.median(ms))
    out = {'shape': [N, H, W], 'ms_median': med, 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)), 'iters': iters,
           'tflop': tflop, 'tflops_per_s': tflop / (med / 1e3), 'in_kernel_mhz': mhz,
           'launches_ms': timed_ms, 'untimed_ms': med - timed_ms, 'layers': layers}
    del plan, net, x
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'estnet_bench.json'))
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--shapes', default='1x3000x4000,1x256x8192,32x256x256')
    a = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'settings': {k: v for k, v in E.MEAN_ARGS.items()}, 'results': []}
    for s in a.shapes.split(','):
        N, H, W = (int(v) for v in s.split('x'))
        r = bench_shape(N, H, W, a.iters)
        res['results'].append(r)
        print(f"{N}x{H}x{W}: {r['ms_median']:.2f} ms ({r['tflop']:.3f} TFLOP, {r['tflops_per_s']:.0f} TF/s, "
              f"in-kernel {r['in_kernel_mhz'] or 0:.0f} MHz)", flush=True)
        for tag, d in sorted(r['layers'].items(), key=lambda kv: -kv[1]['ms']):
            bw = f" {d['tb_per_s']:5.2f} TB/s ({d['gb']:.2f} GB)" if 'tb_per_s' in d else ""
            print(f"    {tag:48s} {d['launches']:3d} launches {d['ms']:8.2f} ms {d['tflops_per_s'] or 0:7.0f} TF/s{bw}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
