"""CPU: the float64 models and bounds of the fp32-input MFMA convolution kernels (tests/fp32_model.py) -- each model against torch's float64
conv2d / conv_transpose2d, a structure-faithful float32 simulation of each kernel under 1 x T on every operand kind, every listed single defect
above the FACTOR x T the GPU tests allow, the conditioning cap, and the walk regime and launch form each GPU case of
tests/test_hip_fp32_mfma.py claims (the library loads without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_model as M
import split_model as S

FR = M.FR
SMALL = [
    M.case('cpu_wino', 'wino64', (8, 16), 128, 2, 16, 64, (), pre=True, **FR),
    M.case('cpu_wino_plain', 'wino32', (16,), 32, 1, 9, 33, ()),
    M.case('cpu_s1', 's1_64_16', (16, 16), 128, 2, 16, 64, (), pre=True, **FR),
    M.case('cpu_s1_plain', 's1_32_8', (16,), 32, 1, 9, 33, ()),
    M.case('cpu_s2', 's2_32', (16,), 32, 2, 9, 37, (), st=2, **FR),
    M.case('cpu_k1', 'k1_64', (48, 80), 64, 2, 8, 40, (), ks=1, **FR),
    M.case('cpu_kt', 'k1_32', (128,), 32, 2, 5, 20, (), ks=1, sh=True, **FR),
]
# sums of 16 .. 48 products (the 1 x 1 walk cases of the GPU module have 16 .. 64 input channels)
SHORT = [
    M.case('cpu_k1_short', 'k1_64', (16, 32), 64, 2, 8, 40, (), ks=1, **FR),
    M.case('cpu_kt_short', 'k1_32', (32,), 32, 2, 5, 20, (), ks=1, sh=True, **FR),
    M.case('cpu_kt_one_chunk', 'k1_32', (16,), 32, 2, 5, 20, (), ks=1, sh=True, **FR),
]
BY_NAME = {c['name']: c for c in SMALL}
nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)


def torch_reference(c, o):
    x = nchw(torch.cat(o['xs'], 3))
    if c['pre']:
        x = F.silu(x)
    if c['sh']:
        z = F.conv_transpose2d(x, o['w'], stride=2)
    else:
        z = F.conv2d(x, o['w'], stride=c['st'], padding=c['ks'] // 2)
    if o['es'] is not None:
        z = z * o['es'][:, :, None, None]
    z = z + M.case_et(o)[:, :, None, None]
    if c['slope'] is not None:
        z = F.leaky_relu(z, c['slope'])
    if o['res'] is not None:
        z = z + nchw(o['res'])
    return nhwc(z)


@pytest.mark.parametrize("kind", ('tame', 'beyond'))
@pytest.mark.parametrize("name", list(BY_NAME))
def test_models_equal_torch_float64(name, kind):
    """The model's reference is torch's float64 layer (to float64 rounding, measured against Q); the Winograd algebra in float64 -- unrounded U --
    is the same convolution."""
    c = BY_NAME[name]
    o = M.case_operands(c, kind)
    m = M.case_model(c, o)
    ref = torch_reference(c, o)
    scale = m['Q'] + ref.abs() + 1e-300
    assert float(((m['y'] - ref).abs() / scale).max()) < 1e-12
    if c['form'].startswith('wino'):
        x = torch.cat(o['xs'], 3)
        a = M.silu64(x) if c['pre'] else x
        z = M.wino_forward(a, o['w'], False)
        zd = M.conv_nhwc(a, o['w'])
        q = M.direct_bound(a, o['w'], zd, 3, 1, False, False)[1]
        # (the exact algebra cancels the seven inputs outside the footprint only to float64 rounding of the 4 x 4 tile: measured against the tile)
        tile = M.wino_bound(a, o['w'], False) / M.U32
        assert float(((z - zd).abs() / (tile + 1e-300)).max()) < 1e-6
        assert bool((M.wino_model(x, o['w'])['T'] > 0).all()) and q.shape == z.shape


def test_an_output_of_winograd_reads_its_own_window_only():
    """The planes output (a, b) of a patch combines (A^T) are fed (B^T) by tile rows / columns a .. a + 2 alone: its 3 x 3 window.  The 4 x 4 tile of
    include/yond_hip.h's footprint rule is a superset; what widens the Winograd bound beside the direct one are the taps (U = G g G^T), not the tile."""
    for a in range(2):
        planes = [xi for xi in range(4) if M.AT[a][xi]]
        rows = sorted({r for xi in planes for r in range(4) if M.BT[xi][r]})
        assert rows == [a, a + 1, a + 2]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 8, 10, 8, generator=g, dtype=torch.float64)
    w = torch.randn(8, 8, 3, 3, generator=g, dtype=torch.float64)
    T0 = M.wino_bound(x, w, False)
    x2 = x.clone()
    x2[0, 3, 5, :] = 1e6                                      # one pixel: the bound moves on its 3 x 3 neighbourhood alone
    T1 = M.wino_bound(x2, w, False)
    changed = ((T1 - T0).abs() > 0).any(3)[0]
    assert bool(changed[2:5, 4:7].all()) and int(changed.sum()) == 9


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("name", list(BY_NAME))
def test_float32_simulation_stays_under_its_bound(name, kind):
    """Anything >= 1 means the simulation or the bound is wrong.  The [accuracy] lines are the worst ratios."""
    c = BY_NAME[name]
    o = M.case_operands(c, kind)
    m = M.case_model(c, o)
    r = S.ratio_report(f"float32 simulation {name} {kind}", M.case_sim(c, o).numpy(), m['y'].numpy(), m['T'].numpy(), ch_axis=3)
    assert r.max() < 1.0
    if m['D'] is not None:
        td = (m['T'] / m['D']).numpy()
        print(f"[accuracy] {name} {kind}: T / D max {td.max():.2f} median {np.median(td):.2f}")


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("c", SHORT, ids=[c['name'] for c in SHORT])
def test_short_sums_stay_inside_half_the_allowed_error(c, kind):
    """K = 16 .. 48: sqrt(K) u (Q + |z|) is a statistical level of the K roundings (about 3.4 sigma of their sum), not a ceiling, and over the
    25 .. 41 thousand outputs of a case the simulation's worst output lies at 0.6 .. 1.2 T before the epilogue (1.11 T after it on the tame
    two-source set).  The form of the term is the one every MFMA sum of this project is held to; the simulation must stay under 2 T, half of what the
    GPU tests allow, so that FACTOR keeps a factor two over the arithmetic itself."""
    o = M.case_operands(c, kind)
    m = M.case_model(c, o)
    r = S.ratio_report(f"float32 simulation {c['name']} {kind}", M.case_sim(c, o).numpy(), m['y'].numpy(), m['T'].numpy(), ch_axis=3)
    assert r.max() < M.FACTOR / 2


@pytest.mark.parametrize("defect,name", [(d, n) for n in ('cpu_wino', 'cpu_s1') for d in M.DEFECTS] + [(d, 'cpu_wino') for d in M.DEFECTS_WINO])
def test_single_defects_exceed_the_allowed_error(defect, name):
    """Every defect exceeds FACTOR x T on at least one operand kind of the case (the line lists all five)."""
    c = BY_NAME[name]
    worst = {}
    for kind in M.KINDS:
        o = M.case_operands(c, kind)
        m = M.case_model(c, o)
        y = M.defective(c, o, defect)
        worst[kind] = float(((y - m['y']).abs() / m['T']).max())
    print(f"[accuracy] defect {defect} on {name}: max err / T " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) > M.FACTOR
    assert sum(v > M.FACTOR for v in worst.values()) >= 3              # ... and not on one lucky set alone


def small_enough(c):
    g, gemm_n, Ho, Wo = M.case_geometry(c)
    return c['N'] * Ho * Wo * (4 if c['sh'] else 1) * c['cout'] <= 1 << 20


@pytest.mark.parametrize("kind", M.KINDS)
def test_cases_are_well_conditioned(kind):
    """No more than 1 % of the outputs with T > 0.1 |ref| + 0.1 Q -- on the CPU cases and on every GPU case of at most 2^20 outputs here; the GPU
    module asserts the same cap on every case it runs (the model is evaluated there anyway)."""
    worst = {}
    for c in SMALL + [c for c in M.CASES if small_enough(c)]:
        worst[c['name']] = M.ill_conditioned(M.case_model(c, M.case_operands(c, kind)))
    print(f"[accuracy] ill-conditioned fraction, {kind}: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items() if v > 0))
    assert max(worst.values()) <= 0.01, worst


# ---- walk coverage ------------------------------------------------------------------------------------------------------------------------

def lib():
    from yond_public_amd import _lib as L
    return L.load()


def test_restated_constants():
    """Tile shape, slots and chunk of each launch form, by hand from the kernels: WinoCfg<TN, TH, KC, VB> (TW 32, grid min(tiles, 256));
    ConvCfg<KS, STRIDE, TH, TN, KC> (TW 32) with 256 * conv_wgs_per_cu slots: 3x3 stride 1 at KC 8 two workgroups, stride 2 at TN 32 two, 1x1 three at
    TN 32 else two, every other form one -- and only one workgroup per CU defers its epilogue."""
    want = {'wino64': (8, 64, 8, 256, False), 'wino32': (16, 32, 8, 256, False), 's2_32': (4, 32, 8, 512, False), 'k1_64': (8, 64, 16, 512, False),
            'k1_32': (8, 32, 16, 768, False), 's1_32_16': (8, 32, 16, 256, True), 's1_64_16': (8, 64, 16, 256, True), 's1_32_8': (8, 32, 8, 512, False),
            's1_64_8': (8, 64, 8, 512, False), 's2_64': (8, 64, 8, 256, True)}
    assert set(want) == set(M.FORMS)
    for k, (th, tn, kc, slots, defer) in want.items():
        f = M.FORMS[k]
        assert (f['th'], f['tw'], f['tn'], f['kc'], f['slots'], f['defer']) == (th, 32, tn, kc, slots, defer), k
        assert defer == (slots == 256 and not k.startswith('wino')), k


@pytest.mark.parametrize("name", [c['name'] for c in M.CASES])
def test_case_is_in_the_regime_it_claims(name):
    c = next(x for x in M.CASES if x['name'] == name)
    assert c['claims']
    for claim in c['claims']:
        assert M.claim_holds(claim, c), (name, claim, M.case_geometry(c)[0])
    g = M.case_geometry(c)[0]
    if c['form'] in ('s1_32_16', 's1_64_16', 's2_64'):
        assert g['defer']                                    # the deferred epilogue runs inside the next tile's first step


@pytest.mark.parametrize("form", M.MANDATORY)
def test_mandatory_forms_cover_every_regime(form):
    have = set()
    for c in M.CASES:
        if c['form'] == form:
            have |= set(c['claims'])
    want = set(M.REGIMES) - set(M.UNREACHABLE.get(form, ()))
    if form == 's2_32':
        want.add('odd_s2')
    assert want <= have, sorted(want - have)
    for c in M.CASES:
        if c['form'] not in M.MANDATORY:
            assert {'one_to_two', 'ct2_img2'} <= set(c['claims']) and c['film'] == 'batch' and c['res'], c['name']
    assert {c['form'] for c in M.CASES} == set(M.FORMS)


@pytest.mark.parametrize("name", [c['name'] for c in M.CASES])
def test_library_chooses_the_form_the_case_names(name):
    """(tn, kc) of yond_conv_config at the case's extent / the tile width of yond_conv_wino_supported: a retune moves no case to another form
    unnoticed.  Forced cases: the form is what the configuration WITHOUT an extent gives (16-channel chunks; with the extent, a launch of 257 .. 511
    tiles of one width always scores higher on the 512-slot form), resp. what no configuration gives (stride 2 at 64 channels) -- and the
    configuration WITH the extent is pinned as well."""
    c = next(x for x in M.CASES if x['name'] == name)
    L = lib()
    g, gemm_n, Ho, Wo = M.case_geometry(c)
    cin = sum(c['splits'])
    f = M.FORMS[c['form']]
    if c['form'].startswith('wino'):
        assert int(L.yond_conv_wino_supported(cin, gemm_n)) == f['tn']
        return
    tn, kc = C.c_int(), C.c_int()
    assert L.yond_conv_config(c['ks'], c['st'], cin, gemm_n, int(c['sh']), c['N'], Ho, Wo, C.byref(tn), C.byref(kc)) == 0
    if c['force'] is None:
        assert (tn.value, kc.value) == (f['tn'], f['kc'])
    else:
        assert c['force'] == (f['tn'], f['kc'])
        assert (tn.value, kc.value) == {'s1_32_16': (32, 8), 's1_64_16': (32, 16), 's2_64': (32, 8)}[c['form']]
        if c['st'] == 1:
            assert L.yond_conv_config(c['ks'], c['st'], cin, gemm_n, 0, 0, 0, 0, C.byref(tn), C.byref(kc)) == 0
            assert (tn.value, kc.value) == c['force']
    # the direct kernels take channel counts in multiples of 16 only: what makes 1 and 3 eight-channel chunks unreachable
    assert L.yond_conv_config(c['ks'], c['st'], 8, gemm_n, int(c['sh']), 0, 0, 0, C.byref(tn), C.byref(kc)) != 0
    assert L.yond_conv_config(c['ks'], c['st'], 24, gemm_n, int(c['sh']), 0, 0, 0, C.byref(tn), C.byref(kc)) != 0
