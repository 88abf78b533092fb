"""GPU: the networks on checkpoint-like weights (oracle.stress_state_dict: heavy-tailed weights, output channels spread over 10^4,
dominant input channels, activations up to ~1e4) against the REFERENCE's own outputs (tests/golden/net_stress.npz, written by
tools/gen_golden_stress.py): its float32 output y at 1e-4 max(1, max|y|) as for the tame networks, and per output channel its float64
output y64 at max(1e-4 max|y64_c|, 4 max|y_c - y64_c|) -- the second term is four times the reference's own distance from float64 in that
channel, read from the fixture.  The fixture keeps two corner crops of every output; the per-channel maxima are those of the whole output.
The non-tripping cases must not raise the range guard; the tripping case (one decoder layer's output ~2e5..6e5) must, and still return
the reference's result.  The fp16 path must stay finite and guard-silent; its PSNR is printed (the 55 dB bar belongs to tame networks).

Measured on the MI355X (max over the output channels of err / tolerance against y64; max |y - reference y| / its tolerance): see
DESIGN.md section 3, "Checkpoint-like weights"."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from hip_common import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_stress as G  # noqa: E402  (the generator's seeds, input law and crops; its reference part is not imported here)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NET_CASES = [c for c in G.CASES if not c[4]]


def fixture_gains(g, aname, trip=False):
    gains = dict(zip([str(k) for k in g[f"gain_keys_{aname}"]], g[f"gains_{aname}"]))
    if trip:
        gains.update(zip([str(k) for k in g["trip_keys"]], g["trip_gains"]))
    return gains


def make(aname, gains, precision='fp32'):
    import yond_oracle as O
    from yond_public_amd import archs as A
    arch = dict(G.ARCHS[aname])
    sd = O.stress_state_dict(arch, G.SEED, gains)
    net = getattr(A, arch['name'])(dict(arch))
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    net.precision = precision
    return net, arch, sd


def run(net, arch, x, t):
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = net(x.to(DEV), t.to(DEV)) if arch.get('guided') else net(x.to(DEV))
    return y.cpu(), sum("fp16's range" in str(w.message) for w in wl)


def layer_outputs(net, arch, x, t):
    """[(layer, tag, output [N][Ho][Wo][C] float64 on the CPU)] of every MFMA convolution launch of one forward, in launch order: the
    plan's `_conv` is wrapped, its destination cloned behind the launch and decoded afterwards (split planes, planes of 4 channels, the
    fused output projection's [N][H][W][4]).  A conv1 that stores SiLU(value) is marked so that it can be compared with a plan whose
    conv1 stores the value itself.  (The two-sub-positions decoder form is switched off for the recording: its launch is bit-identical.)"""
    from test_hip_conv import from_p4, sp_decode
    from yond_public_amd import engine as E
    from yond_public_amd import pipeline as P
    plan = P._plan_of(net, torch.device(DEV))
    if hasattr(plan, 'blocks'):
        names = {id(pc): f"conv{i}.{k}" for i, blk in plan.blocks.items() for k, pc in blk.items() if hasattr(pc, 'ksize')}
    else:
        names = {id(pc): k for k, pc in plan.convs.items()}
    rec, orig, saved = [], plan._conv, E.K1_SUB2

    def wrapped(pc, src0, src1, N, H, W, dst, **kw):
        plan.prof = []
        r = orig(pc, src0, src1, N, H, W, dst, **kw)
        tag, plan.prof = plan.prof[0][0], None
        shuffle, stride = bool(pc.shuffle), pc.stride
        Ho, Wo = (2 * H, 2 * W) if shuffle else (((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W))
        C = pc.cout_real_p if shuffle else pc.coutp
        out = kw['out4'][4] if kw.get('out4') is not None else dst
        rec.append((names[id(pc)], tag, out.clone(), kw.get('out_fmt', 0) if kw.get('out4') is None else 0, (N, Ho, Wo, C), kw.get('post_act', 0) == 1))
        return r
    plan._conv, E.K1_SUB2 = wrapped, False
    try:
        run(net, arch, x, t)
    finally:
        E.K1_SUB2 = saved
        del plan._conv
        plan.prof = None
    rows = []
    for name, tag, buf, fmt, (N, Ho, Wo, C), silu in rec:
        if fmt == 1:
            val = sp_decode(buf, N, C, Ho, Wo)[0].permute(0, 2, 3, 1)
        elif fmt == 2:
            val = from_p4(buf, N, Ho, Wo, C).double()
        else:
            val = buf.cpu().double()
        rows.append((name, tag, val, silu))
    return rows


def print_layer_table(case, net, net_mfma, arch, x, t):
    """Every layer of the default path beside the precision='fp32-mfma' plan on the same weights: the place to look when a channel fails."""
    a, b = layer_outputs(net, arch, x, t), layer_outputs(net_mfma, arch, x, t)
    assert [r[0] for r in a] == [r[0] for r in b]
    for (name, tag, va, sa), (_, tagb, vb, sb) in zip(a, b):
        if sa != sb:
            va, vb = (va, torch.nn.functional.silu(vb)) if sa else (torch.nn.functional.silu(va), vb)
        if va.shape != vb.shape:                                    # (the fused output projection against the unfused last layer)
            print(f"[layers] {case} {name:14s} {tag}: fused output projection, no tensor to compare (fp32-mfma: {tagb})")
            continue
        scale = float(vb.abs().max())
        print(f"[layers] {case} {name:14s} {tag}: max|default - fp32-mfma| = {float((va - vb).abs().max()):.3e} = "
              f"{float((va - vb).abs().max()) / max(scale, 1e-30):.2e} of max|layer| {scale:.3e}")
    return [r[1] for r in a]


def case_input(case):
    ci = [c[0] for c in G.CASES].index(case)
    _, aname, shape, sigma, trip = G.CASES[ci]
    x = G.stress_input(shape, ci)
    return aname, x, (G.stress_t(x, sigma) if sigma else None), trip


@pytest.mark.parametrize("case", [c[0] for c in NET_CASES])
def test_net_on_checkpoint_like_weights(golden, case):
    g = golden("net_stress")
    aname, x, t, _ = case_input(case)
    if t is not None:
        assert float(t) == float(g[f"t_{case}"])
    net, arch, _ = make(aname, fixture_gains(g, aname))
    y, warned = run(net, arch, x, t)
    assert warned == 0, "range-guard warning on weights whose activations stay below 3e4"
    assert bool(torch.isfinite(y).all())
    net_mfma = make(aname, fixture_gains(g, aname), 'fp32-mfma')[0]
    y_mfma, _ = run(net_mfma, arch, x, t)
    # the test must measure the split-operand path: a weight beyond fp16's range would move its layer to the fp32-input kernels silently
    tags = print_layer_table(case, net, net_mfma, arch, x, t)
    assert tags and all(tg.startswith("conv_split_kernel<") or tg.endswith("/split") for tg in tags), tags
    ymax = float(g[f"y_absmax_{case}"])
    worst = 0.0
    for i, (got, mf) in enumerate(zip(G.crops(y), G.crops(y_mfma))):
        ref = g[f"y{i}_{case}"].astype(np.float64)
        y64 = ref - g[f"d{i}_{case}"].astype(np.float64)
        got = got.numpy().astype(np.float64)
        e32 = report(f"stress net {case} crop {i} vs reference float32", got, ref)
        print(f"[accuracy] stress net {case} crop {i}: vs reference float32 {e32:.3e} of {1e-4 * max(1.0, ymax):.3e} allowed")
        assert e32 <= 1e-4 * max(1.0, ymax)
        for c in range(4):
            t1, t2 = 1e-4 * float(g[f"y64_chmax_{case}"][c]), 4.0 * float(g[f"d_chmax_{case}"][c])
            err = float(np.abs(got[:, c] - y64[:, c]).max())
            err_mf = float(np.abs(mf.numpy().astype(np.float64)[:, c] - y64[:, c]).max())
            print(f"[accuracy] stress net {case} crop {i} channel {c} vs float64: err {err:.3e} (fp32-mfma plan {err_mf:.3e}); "
                  f"1e-4 max|y64_c| = {t1:.3e}, 4 max|y_c - y64_c| = {t2:.3e}; ratio {err / max(t1, t2):.3f}")
            worst = max(worst, err / max(t1, t2))
            assert err <= max(t1, t2), (case, i, c)
    print(f"[accuracy] stress net {case}: worst per-channel ratio {worst:.3f}")
    # the fp16 path on the same case: finite, guard-silent; PSNR against the reference's float32 output
    y16, warned = run(make(aname, fixture_gains(g, aname), 'fp16')[0], arch, x, t)
    assert warned == 0 and bool(torch.isfinite(y16).all())
    mse = np.mean([np.mean((a.numpy().astype(np.float64) - g[f"y{i}_{case}"]) ** 2) for i, a in enumerate(G.crops(y16))])
    print(f"[accuracy] stress net {case}: fp16 path PSNR {10 * np.log10(1.0 / max(mse, 1e-30)):.1f} dB against the reference's float32 output")


def vst_setup(g, case, trip):
    import yond_oracle as O
    H, W, K, s, idx = g[f"meta_{case}"]
    noisy, _ = O.synth_noisy(int(H), int(W), float(K), float(s), int(idx))
    p = O.default_params()
    p['gain'], p['sigma'] = np.float64(K), np.float64(s)
    net, arch, _ = make("gru32", fixture_gains(g, "gru32", trip))
    return torch.from_numpy(noisy).to(DEV), p, net, arch


def vst_check(g, case, name, dn, tol):
    dn = np.asarray(dn, np.float64)
    assert np.isfinite(dn).all()
    lim = tol * max(1.0, float(g[f"dn_absmax_{case}"]))
    for i, got in enumerate((dn[:48, :96], dn[-16:, -96:])):
        assert report(f"{name} crop {i}", got, g[f"dn{i}_{case}"]) <= lim


def test_vst_denoiser_on_checkpoint_like_weights(golden):
    from yond_public_amd import pipeline as P
    g = golden("net_stress")
    x, p, net, arch = vst_setup(g, "vst", False)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        dn = P.VST_Denoiser(x, p, net, arch, bias_corr='pre').cpu().numpy()
    assert not any("fp16's range" in str(w.message) for w in wl)
    vst_check(g, "vst", "stress VST_Denoiser vs reference", dn, 1e-4)


def test_tripping_decoder_layer_returns_the_reference(golden):
    """conv7.conv1 (decoder, level 2) ~2e5..6e5, conv7.conv2 brings it back: warning, and the reference's output at 2e-4 max(1, max|ref|)
    on net(x, t), VST_Denoiser and denoise_stream."""
    from yond_public_amd import pipeline as P
    g = golden("net_stress")
    aname, x, t, trip = case_input("gru32_trip")
    assert trip and float(g["layer_max_gru32_trip"].max()) > 65504.0
    net, arch, _ = make(aname, fixture_gains(g, aname, True))
    y, warned = run(net, arch, x, t)
    assert warned >= 1 and bool(torch.isfinite(y).all())
    lim = 2e-4 * max(1.0, float(g["y_absmax_gru32_trip"]))
    for i, got in enumerate(G.crops(y)):
        assert report(f"tripping net(x, t) crop {i} vs reference", got.numpy(), g[f"y{i}_gru32_trip"]) <= lim
    xv, p, net, arch = vst_setup(g, "vst_trip", True)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        dn = P.VST_Denoiser(xv, p, net, arch, bias_corr='pre').cpu().numpy()
    assert any("fp16's range" in str(w.message) for w in wl)
    vst_check(g, "vst_trip", "tripping VST_Denoiser vs reference", dn, 2e-4)
    pipe = {'k': 29, 'vst_type': 'exact', 'bias_corr': 'pre', 'iter': 'once', 'full_dn': True}
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        outs = list(P.denoise_stream([xv, xv.clone()], net, arch, pipe))
    assert len(outs) == 2 and all(bool(torch.isfinite(o['raw_dns'][0]).all()) for o in outs)
    assert sum("fp16's range" in str(w.message) for w in wl) == 2
