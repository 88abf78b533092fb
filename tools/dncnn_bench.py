"""Measure the DnCNN plug-in (runfile settings: depth 17, nf 64, BatchNorm, residual) on the HIP kernels.

    python tools/dncnn_bench.py [--out profiles/dncnn_bench.json] [--iters 30] [--shapes 1x3000x4000,32x256x256]

A shape is N Bayer frames of H x W: the network sees [N][H/2 -> multiple of 32][W/2 -> multiple of 32][4], as the VST hands it over.
Per shape, after warm-up:
  * the whole forward (HIP events around plan.forward_nhwc4, median of --iters) and, from one extra forward with an event pair around
    every launch, the time per layer kind;
  * the last layer A/B, interleaved in one loop on the same tensors: yond_conv3x3_out4_f32 against the route the other kernels allow --
    the weights zero-padded to 32 output channels on the split-operand 3x3 kernel with the fused output projection (out4) picking the
    four real channels; both medians, the largest difference of the two results, the layer's algorithmic HBM bytes
    (4 Cin + 32 per pixel) over the new kernel's time, and that rate as a fraction of what a device-to-device copy of the same
    number of bytes reaches in the same run;
  * Bayer megapixels per second of pipeline.IterDenoise with iter 'once' (host clock around calls that end in a synchronise).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dncnn_common as D  # noqa: E402

ARGS = D.dn_args()                    # depth 17, nf 64, use_bn, res


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def last_layer_ab(plan, N, H, W, iters):
    from yond_public_amd import _lib as L
    from yond_public_amd.engine import _PackedConv
    nf, dev = plan.nf, plan.dev
    g = torch.Generator(device=dev).manual_seed(3)
    feat = torch.rand((N, H, W, nf), device=dev, generator=g)
    x4 = torch.rand((N, H, W, 4), device=dev, generator=g)
    w = torch.randn((4, nf, 3, 3), generator=torch.Generator().manual_seed(4)) / np.sqrt(9.0 * nf)
    packed = np.empty(36 * nf, np.float32)
    wn = np.ascontiguousarray(w.numpy())
    L.check(plan.lib.yond_pack_conv3x3_out4_weight_f32(wn.ctypes.data, nf, packed.ctypes.data), "yond_pack_conv3x3_out4_weight_f32")
    wd = torch.from_numpy(packed).to(dev)
    out_new, out_pad = torch.empty_like(x4), torch.empty_like(x4)

    def new():
        L.check(plan.lib.yond_conv3x3_out4_f32(L.ptr(feat), nf, L.ptr(wd), None, L.ptr(x4), -1.0, N, H, W, L.ptr(out_new), L.stream()),
                "yond_conv3x3_out4_f32")

    # the padded route: x + conv(feat, -w) through 32 output channels (28 of them zero) and the fused projection [4][32] = identity on the first four
    pc = _PackedConv(dev, -w, None, 3, 1, [nf])
    pick = torch.zeros((4, 32), dtype=torch.float32, device=dev)
    pick[torch.arange(4), torch.arange(4)] = 1.0

    def padded():
        plan._conv(pc, feat, None, N, H, W, None, out4=(pick, None, x4, None, out_pad))

    nbytes = N * H * W * (4 * nf + 32)
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)      # a copy moves its size twice: the same number of bytes in all
    dst = torch.empty_like(src)
    for _ in range(3):
        new(), padded(), dst.copy_(src)
    torch.cuda.synchronize()
    t_new, t_pad, t_copy = [], [], []
    for _ in range(iters):
        t_new.append(timed(new))
        t_pad.append(timed(padded))
        t_copy.append(timed(lambda: dst.copy_(src)))
    torch.cuda.synchronize()
    diff = float((out_new - out_pad).abs().max())
    m_new, m_pad, m_copy = (float(np.median(t)) for t in (t_new, t_pad, t_copy))
    rate, copy_rate = nbytes / (m_new / 1e3) / 1e12, nbytes / (m_copy / 1e3) / 1e12
    return {'new_ms': m_new, 'new_ms_min': float(np.min(t_new)), 'padded_ms': m_pad, 'padded_ms_min': float(np.min(t_pad)),
            'max_abs_diff': diff, 'bytes': nbytes, 'new_tb_per_s': rate, 'copy_ms': m_copy, 'copy_tb_per_s': copy_rate,
            'fraction_of_copy_rate': rate / copy_rate, 'tflops_per_s': 2.0 * 36 * nf * N * H * W / (m_new / 1e3) / 1e12}


def pipeline_once(net, N, Hf, Wf, reps=5):
    """Bayer MP/s of IterDenoise (iter 'once'): one full frame (full_dn), or the N frames as a stack of blocks."""
    from yond_public_amd import pipeline as P
    from yond_public_amd import synthetic as S
    pipe = {'k': 29, 'vst_type': 'exact', 'bias_corr': 'pre', 'iter': 'once', 'max_iter': 1, 'full_dn': N == 1}
    if N == 1:
        lr = torch.from_numpy(S.synth_noisy(Hf, Wf, 4.0, 6.0, 5)[0]).cuda()
    else:
        lr = torch.from_numpy(np.ascontiguousarray(np.stack(np.split(S.synth_noisy(Hf, Wf * N, 4.0, 6.0, 5)[0], N, axis=-1)))).cuda()
    for _ in range(2):
        P.IterDenoise(lr, net, ARGS, pipe)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        P.IterDenoise(lr, net, ARGS, pipe)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return {'ms_median': med * 1e3, 'bayer_mp_per_s': N * Hf * Wf / 1e6 / med}


def bench_shape(N, Hf, Wf, iters):
    net = D.build(ARGS, D.weights(ARGS, 7), "cuda")
    H, W = (Hf // 2 + 31) // 32 * 32, (Wf // 2 + 31) // 32 * 32
    x4 = torch.rand((N, H, W, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 0.9
    plan = net._get_plan(x4.device)
    for _ in range(3):
        plan.forward_nhwc4(x4)
    torch.cuda.synchronize()
    ms = [timed(lambda: plan.forward_nhwc4(x4)) for _ in range(iters)]
    plan.prof = []
    plan.forward_nhwc4(x4)
    torch.cuda.synchronize()
    layers = {}
    for tag, flops, a, b in plan.prof:
        d = layers.setdefault(tag, {'launches': 0, 'ms': 0.0, 'tflop': 0.0})
        d['launches'] += 1
        d['ms'] += a.elapsed_time(b)
        d['tflop'] += flops / 1e12
    plan.prof = None
    for d in layers.values():
        d['ms_per_launch'] = d['ms'] / d['launches']
        d['tflops_per_s'] = d['tflop'] / (d['ms'] / 1e3) if d['ms'] else None
    med = float(np.median(ms))
    tflop = plan.flops(N, H, W) / 1e12
    out = {'shape': [N, Hf, Wf], 'network_input': [N, H, W, 4], 'forward_ms_median': med, 'forward_ms_min': float(np.min(ms)),
           'forward_ms_max': float(np.max(ms)), 'iters': iters, 'tflop': tflop, 'tflops_per_s': tflop / (med / 1e3), 'layers': layers,
           'last_layer_ab': last_layer_ab(plan, N, H, W, iters)}
    try:
        out['pipeline_once'] = pipeline_once(net, N, Hf, Wf)
    except Exception as e:                                      # (recorded, not hidden: the A/B and the forward stand on their own)
        out['pipeline_once'] = {'error': f"{type(e).__name__}: {e}"}
    del plan, net, x4
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dncnn_bench.json'))
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--shapes', default='1x3000x4000,32x256x256')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dncnn_bench.py needs an MI355X: there is nothing to measure without one")
    res = {'device': torch.cuda.get_device_name(0), 'settings': dict(ARGS), 'results': []}
    for s in a.shapes.split(','):
        N, Hf, Wf = (int(v) for v in s.split('x'))
        r = bench_shape(N, Hf, Wf, a.iters)
        res['results'].append(r)
        ab, po = r['last_layer_ab'], r['pipeline_once']
        print(f"{s}: forward {r['forward_ms_median']:.3f} ms ({r['tflop']:.3f} TFLOP, {r['tflops_per_s']:.0f} TF/s); once pipeline "
              + (f"{po['ms_median']:.2f} ms = {po['bayer_mp_per_s']:.0f} Bayer MP/s" if 'error' not in po else po['error']), flush=True)
        for tag, d in sorted(r['layers'].items(), key=lambda kv: -kv[1]['ms']):
            print(f"    {tag:44s} {d['launches']:3d} launches {d['ms_per_launch']:8.3f} ms each {d['tflops_per_s'] or 0:7.0f} TF/s", flush=True)
        print(f"    last layer: new {ab['new_ms']:.3f} ms (min {ab['new_ms_min']:.3f}) vs padded Cout 32 + out4 {ab['padded_ms']:.3f} ms "
              f"(min {ab['padded_ms_min']:.3f}); max |diff| {ab['max_abs_diff']:.2e}; {ab['bytes'] / 1e6:.0f} MB -> {ab['new_tb_per_s']:.2f} TB/s = "
              f"{100 * ab['fraction_of_copy_rate']:.0f} % of the copy rate {ab['copy_tb_per_s']:.2f} TB/s; {ab['tflops_per_s']:.0f} TF/s fp32", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
        print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
