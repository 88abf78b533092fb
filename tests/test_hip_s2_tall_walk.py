"""GPU: what tests/test_hip_s2_tall.py leaves open in the stride-2 layer on 8-row tiles (csrc/conv_s2_tall.hip, descriptor algo 7): its shapes
give every workgroup at most one tile, have even input sizes and at least two 16-channel chunks.  Here, each case BIT FOR BIT against the
stride-2 form of the template (algo 3) through that file's run_pair, status words included:
  * tile to tile: more tiles than the 256 workgroups, so that workgroups walk two tiles and a tile's first chunk is requested under the previous
    tile's last step -- 256 -> 512 channels, output 40 x 224 (280 tiles of 16 chunks) with the second output, and 32 -> 128 channels, two images,
    output 64 x 288 (288 tiles of two chunks) without it; both tile orders;
  * one chunk per tile (16 -> 64 channels, output 9 x 33, one and two images): every step is a tile's first and last;
  * odd input sizes (15 x 61 and 17 x 129, Ho = (H + 1) / 2, 64 -> 128 channels): the last input row and column of the last tiles lie outside the
    frame, the zero unit is read at the far edges as well as at the near ones.
Operands as there: stress activations with values planted at fp16's subnormal boundary, heavy-tailed weights.
(The library chooses the kernel's form by depth: 32 input channels run the one-image form, every other case here the two-image form.)"""
import numpy as np
import pytest
import torch

import split_model as M
from test_hip_conv import DEV, bare_plan, nhwc, to_sp
from test_hip_s2_tall import T_, bits, run_pair

pytestmark = pytest.mark.gpu

FILMS = ("bias", "scale + shift", "bias + LeakyReLU")


def check(cin, cout, N, H, W, d2, films=("bias",), orders=(0, 1)):
    from yond_public_amd.engine import _PackedConv
    rng = np.random.default_rng([41, cin, cout, N, H, W])
    wf = M.stress_weights(rng, cout, cin, 3)
    bf = (10.0 ** rng.uniform(-2, 2, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    plan = bare_plan()
    plan.status = torch.zeros(4, dtype=torch.int32, device=DEV)
    pc = _PackedConv(plan.dev, T_(wf), T_(bf), 3, 2, [cin])
    if pc.cinp != cin:
        # the engine pads every input to a multiple of 32 channels (zero weights); the library takes multiples of 16: packed again at the real width
        pc._wp = np.ascontiguousarray(pc._wp[:, :cin])
        pc.psplits, pc.cinp, pc._packed = [cin], cin, {}
    edge = np.float32(2.0 ** -14)
    plant = torch.tensor([edge, -edge, edge * (1 - 2.0 ** -11), edge * (1 + 2.0 ** -10), 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 0.0])
    x = nhwc(T_(M.stress_acts(rng, (N, cin, H, W), 'signed')))
    x[..., 0:8] = plant
    xin = to_sp(x)
    es, et = M.stress_film(rng, N, cout)
    kws = {"bias": {}, "scale + shift": dict(escale=T_(es).to(DEV), eshift=T_(et).to(DEV), ebatch=1), "bias + LeakyReLU": dict(post_act=2, slope=0.2)}
    for film in films:
        for order in orders:
            out = run_pair(plan, pc, xin, N, H, W, cout, d2, order, **kws[film])
            torch.cuda.synchronize()
            name = f"c{cin}->{cout} N{N} {H}x{W} film={film} order={order}"
            assert bool(torch.isfinite(out[False][0]).all()), name
            assert torch.equal(bits(out[True][0]), bits(out[False][0])), (name, int((bits(out[True][0]) != bits(out[False][0])).sum()))
            if d2:
                assert torch.equal(bits(out[True][1]), bits(out[False][1])), (name, int((bits(out[True][1]) != bits(out[False][1])).sum()))
                assert bool((bits(out[False][1]) != 0).any()), name
    st = plan.status.cpu()
    assert int(st[0]) == int(st[1]), st
    if not d2:
        assert int(st[0]) == 0, st                # (a consumer of finished planes raises nothing)


def test_s2_tall_walks_from_tile_to_tile_sixteen_chunks():
    """8 channel tiles x 5 x 7 = 280 tiles on 256 workgroups, 16 chunks per tile, the second output."""
    check(256, 512, 1, 80, 448, True)


def test_s2_tall_walks_from_tile_to_tile_two_chunks():
    """2 channel tiles x 8 x 9 x 2 images = 288 tiles on 256 workgroups, two chunks per tile, no second output."""
    check(32, 128, 2, 128, 576, False)


@pytest.mark.parametrize("d2", [False, True])
@pytest.mark.parametrize("N", [1, 2])
def test_s2_tall_one_chunk_per_tile(N, d2):
    """16 input channels: every step is the first and the last chunk of its tile (output 9 x 33: two row tiles, two column bands)."""
    check(16, 64, N, 18, 66, d2, films=FILMS)


@pytest.mark.parametrize("hw", [(15, 61), (17, 129)])
@pytest.mark.parametrize("N", [1, 2])
def test_s2_tall_odd_input_sizes(N, hw):
    """Ho = (H + 1) / 2: input row H and column W, which the last output row and column reach, lie outside the frame."""
    check(64, 128, N, hw[0], hw[1], False, films=FILMS)
