"""GPU: frames the device chain FLAGS, end to end -- the drivers hand them to the host-side chain (DEVICE_CHAIN off around an
IterDenoise, back on in `finally`), and the result must be the host path's, with the chain switched on again for the next frame.
Frame A (a clipped black region: the selected threshold is 0, nothing lies below it, NO_FLAT_AREA, the 25 % backup threshold
takes over) and frame B (a flat grey half: threshold and backup both 0, every pixel fitted, beta2 < 0) are checked against the
oracle on the CPU in tests/test_chain_model.py."""
import numpy as np
import pytest
import torch

from hip_common import ARCHS, report
from test_chain_model import clipped_frame

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PIPE = {'k': 29, 'vst_type': 'exact', 'bias_corr': 'pre', 'iter': 'once', 'full_dn': True}
_CACHE = {}


def setup():
    """The network, the five frames [normal, A, normal, B, normal] and, per frame, the stand-alone host-chain IterDenoise (once)."""
    if _CACHE:
        return _CACHE
    import yond_oracle as O
    from yond_public_amd import archs as A
    from yond_public_amd import pipeline as P
    from yond_public_amd import synthetic as S
    arch = ARCHS["gru8"]
    net = A.GuidedResUnet(dict(arch))
    net.load_state_dict(S.denoising_state_dict(net, 3))
    net = net.to(DEV).eval()
    host = [O.synth_noisy(128, 192, 4.0, 6.0, 12)[0], clipped_frame('A'), O.synth_noisy(128, 192, 2.0, 10.0, 13)[0], clipped_frame('B'),
            O.synth_noisy(128, 192, 6.0, 3.0, 14)[0]]
    frames = [torch.from_numpy(f).to(DEV) for f in host]
    assert P.DEVICE_CHAIN
    P.DEVICE_CHAIN = False
    try:
        want = [P.IterDenoise(f, net, arch, PIPE) for f in frames]
    finally:
        P.DEVICE_CHAIN = True
    for w in want:
        assert 'nle_info' not in w                       # (the host-side chain's result)
    _CACHE.update(arch=arch, net=net, host=host, frames=frames, want=want)
    return _CACHE


def same_result(tag, got, want):
    assert len(got['raw_dns']) == len(want['raw_dns']) == 1 and len(got['regs']) == len(want['regs']) == 1
    for r, w in zip(got['regs'], want['regs']):
        np.testing.assert_allclose(r[0], w[0], rtol=1e-5)
        np.testing.assert_allclose(r[1], w[1], rtol=0, atol=1e-5 * abs(w[0]) + 1e-9)
    assert report(tag, got['raw_dns'][0].cpu().numpy(), want['raw_dns'][0].cpu().numpy()) <= 2e-7


@pytest.mark.parametrize("which,idx", [("A", 1), ("B", 3)])
def test_iter_denoise_hands_a_flagged_frame_to_the_host_chain(which, idx):
    """IterDenoise on frame A / B: the chain applies and is tried, returns None (flag), and the host-side chain's answer comes
    back: regs as the oracle's SimpleNLF, output equal to the host chain's; DEVICE_CHAIN is left on."""
    import yond_oracle as O
    from yond_public_amd import pipeline as P
    s = setup()
    x, net, arch = s['frames'][idx], s['net'], s['arch']
    assert P.chain_applies(x, net, arch, PIPE)
    tried = []
    orig = P._iter_denoise_chain
    P._iter_denoise_chain = lambda *a, **k: (tried.append(orig(*a, **k)), tried[-1])[1]
    try:
        res = P.IterDenoise(x, net, arch, PIPE)
    finally:
        P._iter_denoise_chain = orig
    assert tried == [None]                                # tried once, handed back
    flags = int(P._chain_buffers(x.device, 0).prm_host[P.PRM['flags']])
    print(f"[takeover] frame {which}: chain flags {flags}, host regs {res['regs'][0]}, params {res['params'][0]}")
    assert flags & (P.PRM_NO_FLAT_AREA | P.PRM_LUT_CAPACITY | P.PRM_BAD_ESTIMATE)
    assert flags & P.PRM_NO_FLAT_AREA                     # both frames: nothing below the selected threshold
    assert 'nle_info' not in res and P.DEVICE_CHAIN is True
    ref = O.SimpleNLF(s['host'][idx], k=29, setting={'mode': 'self'})
    np.testing.assert_allclose(res['regs'][0][0], ref[0], rtol=1e-5)
    np.testing.assert_allclose(res['regs'][0][1], ref[1], rtol=0, atol=1e-5 * abs(ref[0]) + 1e-9)
    if which == 'B':
        assert res['regs'][0][1] < 0 and res['params'][0][1] == 0.0        # beta2 < 0: sigma = 0
    same_result(f"takeover, IterDenoise frame {which} vs host chain", res, s['want'][idx])


def _counting(P):
    calls = []
    orig = P.IterDenoise

    def wrapper(*a, **k):
        calls.append(P.DEVICE_CHAIN)
        return orig(*a, **k)
    return calls, orig, wrapper


def test_denoise_stream_takes_over_flagged_frames():
    """denoise_stream on [normal, A, normal, B, normal]: every result is that frame's stand-alone host-chain IterDenoise, the
    inner IterDenoise ran exactly twice (with the chain off), the chain is on afterwards, and the normal frames -- the last
    included -- were served from their parameter blocks."""
    from yond_public_amd import pipeline as P
    s = setup()
    calls, orig, wrapper = _counting(P)
    P.IterDenoise = wrapper
    try:
        got = list(P.denoise_stream(iter(s['frames']), s['net'], s['arch'], PIPE))
        after = P.DEVICE_CHAIN
    finally:
        P.IterDenoise = orig
        P.DEVICE_CHAIN = True
    torch.cuda.synchronize()
    assert after is True
    assert calls == [False, False]
    assert len(got) == 5
    for i, (g, w) in enumerate(zip(got, s['want'])):
        same_result(f"takeover, denoise_stream frame {i} vs host chain", g, w)
        assert ('nle_info' in g) == (i in (0, 2, 4)), i
    last = P._chain_buffers(torch.device(DEV), ('once-stream', 4 % (P.STREAM_LANES + 2))).prm_host.numpy()
    assert int(last[P.PRM['flags']]) == 0
    assert got[4]['regs'][0][0] == last[P.PRM['beta1']] and got[4]['regs'][0][1] == last[P.PRM['beta2']]


def test_denoise_stream_batches_takes_over_flagged_frames():
    """The same five frames through denoise_stream_batches with B = 2 (batches [normal, A], [normal, B], [normal])."""
    from yond_public_amd import pipeline as P
    s = setup()
    calls, orig, wrapper = _counting(P)
    P.IterDenoise = wrapper
    try:
        got = list(P.denoise_stream_batches(iter(s['frames']), 2, s['net'], s['arch'], PIPE))
        after = P.DEVICE_CHAIN
    finally:
        P.IterDenoise = orig
        P.DEVICE_CHAIN = True
    torch.cuda.synchronize()
    assert after is True
    assert calls == [False, False]
    assert len(got) == 5
    for i, (g, w) in enumerate(zip(got, s['want'])):
        same_result(f"takeover, denoise_stream_batches frame {i} vs host chain", g, w)
        assert ('nle_info' in g) == (i in (0, 2, 4)), i
