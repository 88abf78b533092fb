"""Per-launch times of one SNR-Net forward (HIP events around every convolution launch): at the cfg-2 shape by default,
`python tools/layer_times.py B H W` for a batch of B packed [H][W] inputs (cfg 3: 32 128 128).
AB="levels/form;levels/form;..." (experiment library, YOND_HIP_LIB=tools/probe/libyond_exp.so): the variants run INTERLEAVED in one process, REPS
(15) forwards each -- levels = engine.S2_TALL_LEVELS of the variant ("" = the template everywhere), form = YOND_S2T_FORM of csrc/conv_s2_tall.hip
(1 one image, 2 two images, 0 the shipped one), passed to the library through the environment ahead of every forward; median, minimum and
maximum per launch and variant, the outputs compared bit for bit.  AB="/0;0,1,2,3/1;0,1,2,3/2" is the table of profiles/s2_two_image_ab.txt."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yond_public_amd import archs as A, synthetic as S, pipeline as P
from yond_public_amd import engine as E
if os.environ.get("K1_D2_LEVELS") is not None:
    E.K1_D2_LEVELS = tuple(int(v) for v in os.environ["K1_D2_LEVELS"].split(",") if v)
if os.environ.get("K1_STATIONARY_LEVELS") is not None:     # decoder levels on the stationary-weight GEMM ("" = none: the template everywhere)
    E.K1_STATIONARY_LEVELS = tuple(int(v) for v in os.environ["K1_STATIONARY_LEVELS"].split(",") if v)
if os.environ.get("S2_TALL_LEVELS") is not None:            # levels (of the layer's input) whose stride-2 layer runs on 8-row tiles ("" = none)
    E.S2_TALL_LEVELS = tuple(int(v) for v in os.environ["S2_TALL_LEVELS"].split(",") if v)
if os.environ.get("K1_D2_LEVELS_HALF") is not None:
    E.K1_D2_LEVELS_HALF = tuple(int(v) for v in os.environ["K1_D2_LEVELS_HALF"].split(",") if v)
if os.environ.get("SP_CONV1_MIN_LEVEL"):            # A/B of the engine's data-flow constant (tools only)
    E.SP_CONV1_MIN_LEVEL = int(os.environ["SP_CONV1_MIN_LEVEL"])
arch = dict(name='GuidedResUnet', guided=True, in_nc=4, out_nc=4, nf=32, nframes=1, res=True, norm=True)
net = A.GuidedResUnet(dict(arch)); net.load_state_dict(S.procedural_state_dict(net, 0)); net = net.to('cuda').eval()
if os.environ.get("PRECISION"):                    # 'fp16': the BASELINE cfg 5 path (python tools/layer_times.py 1 2016 3008)
    net.precision = os.environ["PRECISION"]
plan = P._plan_of(net, torch.device('cuda'))
B, Hh, Ww = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (1, 1504, 2016)
x = torch.rand(B, Hh, Ww, 4, device='cuda'); t = torch.full((B,), 0.03, device='cuda'); ub = x.reshape(B, -1).max(1).values.contiguous()
for _ in range(3): plan.forward_nhwc4(x, t, ub=ub)
torch.cuda.synchronize()
if os.environ.get("AB"):
    variants = [(v.split("/")[0], v.split("/")[1]) for v in os.environ["AB"].split(";")]
    reps = int(os.environ.get("REPS", "15"))
    acc, outs, tags = {}, {}, {}
    for rep in range(-1, reps):                                # (rep -1: every variant once untimed -- a kernel's first launch loads its code)
        for vi, (levels, form) in enumerate(variants):
            E.S2_TALL_LEVELS = tuple(int(v) for v in levels.split(",") if v)
            os.environ["YOND_S2T_FORM"] = form                 # (the library reads it at every launch)
            plan.prof = []
            y = plan.forward_nhwc4(x, t, ub=ub)
            torch.cuda.synchronize()
            for i, (tag, fl, e0, e1) in enumerate(plan.prof if rep >= 0 else []):
                acc.setdefault((i, vi), []).append(e0.elapsed_time(e1) * 1e3)
                tags[(i, vi)] = tag
            plan.prof = None
            if rep == 0:
                outs[vi] = y.clone()
    print("variants (S2_TALL_LEVELS / YOND_S2T_FORM): " + "   ".join(f"[{vi}] {l or '-'} / {f}" for vi, (l, f) in enumerate(variants)))
    print("bit-equal outputs:", all(torch.equal(outs[0].view(torch.int32), outs[vi].view(torch.int32)) for vi in outs))
    nl = 1 + max(i for i, _ in acc)
    sums = {vi: [sum(acc[(i, vi)][r] for i in range(nl)) for r in range(reps)] for vi in range(len(variants))}
    for i in range(nl):
        row = f"{i:2d} {tags[(i, len(variants) - 1)]:42s}"
        for vi in range(len(variants)):
            v = sorted(acc[(i, vi)])
            row += f" | {v[len(v) // 2]:8.1f} {v[0]:8.1f} {v[-1]:8.1f}"
        print(row + ("  <-- stride 2" if "<2," in tags[(i, 0)] else ""))
    print("sum of conv launches per forward (med min max): " + " | ".join(f"{sorted(v)[len(v) // 2]:.1f} {min(v):.1f} {max(v):.1f}" for v in sums.values()))
    sys.exit(0)
acc = {}
for rep in range(5):
    plan.prof = []
    plan.forward_nhwc4(x, t, ub=ub)
    torch.cuda.synchronize()
    for i, (tag, fl, e0, e1) in enumerate(plan.prof):
        acc.setdefault((i, tag), []).append(e0.elapsed_time(e1) * 1e3)
    plan.prof = None
tot = 0
for (i, tag), v in sorted(acc.items()):
    m = sorted(v)[len(v) // 2]
    tot += m
    print(f"{i:2d} {tag:42s} {m:8.1f} us")
print("sum of conv launches: %.1f us" % tot)
