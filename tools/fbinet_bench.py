"""Measure the FBI_Net plug-in (runfile settings: nf 64, num_of_layers 17, linear, res) on the HIP kernels of csrc/fbinet.hip.

    python tools/fbinet_bench.py [--out profiles/fbinet_bench.json] [--iters 7] [--shape 3000x4000]

On one Bayer frame of H x W (the network sees the one-channel mosaic: activations [1][H][W][64]), after warm-up:
  * the whole forward (HIP events around plan.forward_nhwc4, median of --iters) and, from extra forwards with an event pair around every
    launch, the median time per launch of every entry, with the achieved TF/s of tapconv and rm against the 157.3 TF fp32-matrix peak;
  * the repo's dense fp32-mfma 3x3 64 -> 64 kernel (a DnCNN middle layer, precision 'fp32-mfma') on a tensor of the same size,
    interleaved with the two tapconv sets in one loop: time per launch, time per tap, and tapconv's time per LIVE tap over the dense
    kernel's time per tap;
  * the algorithmic HBM bytes of tapconv (read n and o, write n' and o': 4 x 4 nf per pixel) and of rm over their times, beside the rate
    of a device-to-device copy of as many bytes in the same loop;
  * Bayer megapixels per second of pipeline.IterDenoise with iter 'once' (host clock around calls that end in a synchronise);
  * the shader clock the chip held before and after (yond_clock_probe).
The fused forms the issue names (rm in tapconv's epilogue, out in the last rm) are not built: `fusion_ab` says so, there is no A/B.
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
import dncnn_common as DN  # noqa: E402
import fbinet_common as D  # noqa: E402

ARGS = D.fbi_args()                   # nf 64, num_of_layers 17, linear, res
PEAK_TF = 157.3


def clock_mhz():
    from yond_public_amd import _lib
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().yond_clock_probe(2000.0, _lib.ptr(out), _lib.stream()), "yond_clock_probe")
    c, t = out.cpu().tolist()
    return c / t * 100.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def per_launch(plan, x4, reps):
    """Median over `reps` profiled forwards of the mean time per launch of every tag."""
    acc = {}
    for _ in range(reps):
        plan.prof = []
        plan.forward_nhwc4(x4)
        torch.cuda.synchronize()
        one = {}
        for tag, flops, a, b in plan.prof:
            d = one.setdefault(tag, [0, 0.0, 0.0])
            d[0] += 1
            d[1] += a.elapsed_time(b)
            d[2] += flops
        plan.prof = None
        for tag, (n, ms, fl) in one.items():
            acc.setdefault(tag, {'launches': n, 'flop_per_launch': fl / n, 'ms': []})['ms'].append(ms / n)
    out = {}
    for tag, d in acc.items():
        ms = float(np.median(d['ms']))
        out[tag] = {'launches': d['launches'], 'ms_per_launch': ms, 'ms_per_launch_min': float(np.min(d['ms'])),
                    'tflops_per_s': d['flop_per_launch'] / (ms / 1e3) / 1e12, 'fraction_of_fp32_matrix_peak': d['flop_per_launch'] / (ms / 1e3) / 1e12 / PEAK_TF}
    return out


def dense_ab(plan, H, W, iters):
    """tapconv (both sets) against the dense fp32-mfma 3x3 64 -> 64 kernel and a copy of tapconv's bytes, interleaved."""
    from yond_public_amd import _lib as L
    nf, dev = plan.nf, plan.dev
    g = torch.Generator(device=dev).manual_seed(3)
    n_in, o_in = (torch.randn((1, H, W, nf), device=dev, generator=g) for _ in range(2))
    n_out, o_out = torch.empty_like(n_in), torch.empty_like(n_in)
    dn_args = DN.dn_args(depth=3, nf=nf, use_bn=False, res=True, precision='fp32-mfma')
    dn = DN.build(dn_args, DN.weights(dn_args, 5), dev)
    dplan = dn._get_plan(dev)
    pc = dplan.mid[0][0]
    dplan._tile_order = 0

    def tap(i):
        tset, wpk, b, s1, s2 = plan.taps[i]
        L.check(plan.lib.yond_fbi_tapconv_f32(L.ptr(n_in), L.ptr(o_in), tset, nf, L.ptr(wpk), L.ptr(b), L.ptr(s1), L.ptr(s2), 1, H, W, L.ptr(n_out),
                                              L.ptr(o_out), L.stream()), "yond_fbi_tapconv_f32")

    def dense():
        dplan._conv(pc, n_in, None, 1, H, W, n_out, post_act=2, slope=0.0)

    def rm():
        plan._rm(plan.rms[1], n_in, H * W, n_out, o_out, 2)

    nbytes_tap, nbytes_rm = H * W * nf * 4 * 4, H * W * nf * 4 * 4            # tapconv: n, o in, n', o' out; rm: v in, o out, sum in and out
    src = torch.empty(nbytes_tap // 8, dtype=torch.float32, device=dev)       # a copy moves its size twice
    dst = torch.empty_like(src)
    dplan.prof = []
    dense()
    torch.cuda.synchronize()
    dense_tag, dplan.prof = dplan.prof[0][0], None
    for _ in range(2):
        tap(0), tap(1), dense(), rm(), dst.copy_(src)
    torch.cuda.synchronize()
    t = {'tap0': [], 'tap1': [], 'dense': [], 'rm': [], 'copy': []}
    for _ in range(iters):
        t['tap0'].append(timed(lambda: tap(0)))
        t['dense'].append(timed(dense))
        t['tap1'].append(timed(lambda: tap(1)))
        t['rm'].append(timed(rm))
        t['copy'].append(timed(lambda: dst.copy_(src)))
    m = {k: float(np.median(v)) for k, v in t.items()}
    per_tap = {'tapconv_set0_9_taps': m['tap0'] / 9, 'tapconv_set1_5_taps': m['tap1'] / 5, 'dense_9_taps': m['dense'] / 9}
    return {'tensor': [1, H, W, nf], 'dense_kernel': dense_tag, 'ms': m, 'ms_min': {k: float(np.min(v)) for k, v in t.items()},
            'ms_per_tap': per_tap,
            'tapconv_per_live_tap_over_dense_per_tap': {'set0': per_tap['tapconv_set0_9_taps'] / per_tap['dense_9_taps'],
                                                        'set1': per_tap['tapconv_set1_5_taps'] / per_tap['dense_9_taps']},
            'tflops_per_s': {'tap0': 2.0 * 9 * nf * nf * H * W / (m['tap0'] / 1e3) / 1e12, 'tap1': 2.0 * 5 * nf * nf * H * W / (m['tap1'] / 1e3) / 1e12,
                             'dense': 2.0 * 9 * nf * nf * H * W / (m['dense'] / 1e3) / 1e12, 'rm': 4.0 * nf * nf * H * W / (m['rm'] / 1e3) / 1e12},
            'algorithmic_bytes': {'tapconv': nbytes_tap, 'rm': nbytes_rm},
            'tb_per_s': {'tap0': nbytes_tap / (m['tap0'] / 1e3) / 1e12, 'tap1': nbytes_tap / (m['tap1'] / 1e3) / 1e12,
                         'rm': nbytes_rm / (m['rm'] / 1e3) / 1e12, 'copy': nbytes_tap / (m['copy'] / 1e3) / 1e12}}


def pipeline_once(net, Hf, Wf, reps=3):
    from yond_public_amd import pipeline as P
    from yond_public_amd import synthetic as S
    pipe = {'k': 29, 'vst_type': 'exact', 'bias_corr': 'pre', 'iter': 'once', 'max_iter': 1, 'full_dn': True, 'denoiser_type': 'fbi'}
    lr = torch.from_numpy(S.synth_noisy(Hf, Wf, 4.0, 6.0, 5)[0]).cuda()
    P.IterDenoise(lr, net, ARGS, pipe)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        P.IterDenoise(lr, net, ARGS, pipe)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return {'ms_median': med * 1e3, 'bayer_mp_per_s': Hf * Wf / 1e6 / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fbinet_bench.json'))
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--shape', default='3000x4000')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/fbinet_bench.py needs an MI355X: there is nothing to measure without one")
    Hf, Wf = (int(v) for v in a.shape.split('x'))
    res = {'device': torch.cuda.get_device_name(0), 'settings': dict(ARGS), 'frame': [Hf, Wf], 'clock_mhz_before': round(clock_mhz())}
    net = D.build(ARGS, D.weights(ARGS, 7), "cuda")
    x4 = torch.rand((1, Hf // 2, Wf // 2, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 0.9
    plan = net._get_plan(x4.device)
    for _ in range(2):
        plan.forward_nhwc4(x4)
    torch.cuda.synchronize()
    ms = [timed(lambda: plan.forward_nhwc4(x4)) for _ in range(a.iters)]
    med = float(np.median(ms))
    tflop = plan.flops(1, Hf // 2, Wf // 2) / 1e12
    res['forward'] = {'ms_median': med, 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)), 'iters': a.iters, 'tflop': tflop,
                      'mac_per_pixel': plan.flops(1, 1, 1) / 8, 'tflops_per_s': tflop / (med / 1e3),
                      'floor_ms_at_fp32_matrix_peak': tflop / PEAK_TF * 1e3, 'activation_tensors_gb': 5 * Hf * Wf * 64 * 4 / 1e9}
    res['entries'] = per_launch(plan, x4, 3)
    torch.cuda.empty_cache()
    res['tapconv_vs_dense'] = dense_ab(plan, Hf, Wf, a.iters)
    torch.cuda.empty_cache()
    res['pipeline_once'] = pipeline_once(net, Hf, Wf)
    res['fusion_ab'] = {'rm_in_tapconv_epilogue': 'not built, not measured', 'out_in_last_rm': 'not built, not measured'}
    res['clock_mhz_after'] = round(clock_mhz())
    f, po, ab = res['forward'], res['pipeline_once'], res['tapconv_vs_dense']
    print(f"{Hf}x{Wf}: forward {f['ms_median']:.1f} ms ({f['tflop']:.2f} TFLOP, {f['tflops_per_s']:.1f} TF/s, floor {f['floor_ms_at_fp32_matrix_peak']:.0f} ms); "
          f"once pipeline {po['ms_median']:.1f} ms = {po['bayer_mp_per_s']:.1f} Bayer MP/s; clock {res['clock_mhz_before']} -> {res['clock_mhz_after']} MHz", flush=True)
    for tag, d in sorted(res['entries'].items(), key=lambda kv: -kv[1]['ms_per_launch'] * kv[1]['launches']):
        print(f"    {tag:24s} {d['launches']:3d} launches {d['ms_per_launch']:8.3f} ms each {d['tflops_per_s']:7.1f} TF/s", flush=True)
    print(f"    interleaved: {json.dumps({k: round(v, 3) for k, v in ab['ms'].items()})} ms; per tap {json.dumps({k: round(v, 3) for k, v in ab['ms_per_tap'].items()})}; "
          f"ratio {json.dumps({k: round(v, 2) for k, v in ab['tapconv_per_live_tap_over_dense_per_tap'].items()})}; TB/s {json.dumps({k: round(v, 2) for k, v in ab['tb_per_s'].items()})}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
        print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
