"""-m gpu: PS fused into its consumers (csrc/elementwise.hip: pnp_ps_pad_fwd / _bwd, pnp_critic_input_ps_fwd / _bwd) against the kernel
sequences they replace.  The fused kernels only move values and, where they sum, keep the order of sympad_bwd_kernel / critic_input_bwd_kernel:
every comparison is torch.equal.  The sequences themselves are held to the float64 references by tests/test_gpu_elementwise_domain.py.

Shapes: (1, 1, 1) is a single workgroup that owns all four borders; (2, 3, 5) has first, inner and last tiles in both directions and an odd
row length (T = 1 for the head, 1 coarse pixel per workgroup for the critic: 5 has no divisor 2); (2, 4, 4) takes the critic's two coarse
pixels per workgroup, the model's tiling.
"""
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

R8 = 8
CRITIC_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 4, 4)]
CRITIC_CHANNELS = [(2, 4, 8, 8), (1, 2, 3, 5)]              # after PS; x 64 coarse.  With tile_a, ncls below: Ctot 32 (vector stores) and odd
# the generator step wants everything, a step that trains the critic alone wants nothing of the sources; mixed subsets on top
NEEDS = [(True,) * 5, (False, False, False, False, True), (False,) * 5, (True, False, True, False, False), (False, True, False, True, True)]
# (r, nc, p): the head; a small unspecialised one (scalar stores: nc % 4 != 0); p = r, the widest mirror the kernels take; p = 0
PAD_CASES = [(8, 40, 2), (2, 3, 1), (2, 4, 2), (8, 4, 0)]
PAD_SHAPES = [(1, 1, 1), (2, 3, 5)]


def _gen(seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device, dtype=torch.float32)


@pytest.mark.parametrize("shape", CRITIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("chans", CRITIC_CHANNELS, ids=lambda c: "-".join(map(str, c)))
def test_critic_input_from_coarse(dev, shape, chans):
    K = pkg("kernels")
    N, A, B = shape
    for tile_a in (1, 3):
        for ncls in (2, 5):
            assert K.critic_input_ps_served(chans, tile_a, ncls, R8)
            g = _gen(1000 * A + 100 * B + 10 * tile_a + ncls + chans[0], dev)
            coarse = [_randn(g, N, A, B, c * R8 * R8) + 0.1 for c in chans]
            lg = _randn(g, N, A * R8, B * R8, ncls)
            lg[0, 0, 0] = 1.5                               # every class tied: class 0
            lg[0, 1, 2] = -1.0
            lg[0, 1, 2, 1::2] = 2.0                         # the odd classes tied: class 1
            lg[-1, -1, -1, :] = 0.25
            lg[-1, -1, -1, -1] = 0.5                        # a plain maximum in the last class
            lg[-1, 3, 4, :] = lg[-1, 3, 4, :].abs() + 1.0
            lg[-1, 3, 4, 0] = float(lg[-1, 3, 4].max())     # first and a later class tied at the maximum: class 0
            fine = [K.ps_fwd(t, R8, c) for t, c in zip(coarse, chans)]
            want = K.critic_input_fwd(fine[0], tile_a, fine[1], fine[2], fine[3], lg)
            got = K.critic_input_ps_fwd(coarse[0], tile_a, coarse[1], coarse[2], coarse[3], lg, R8)
            assert float(want[0, 0, 0, -1]) == 0.0 and float(want[0, 1, 2, -1]) == 1.0 and float(want[-1, -1, -1, -1]) == ncls - 1
            assert float(want[-1, 3, 4, -1]) == 0.0
            assert got.shape == want.shape and torch.equal(got, want), (shape, chans, tile_a, ncls)
            dout = _randn(g, *want.shape)
            fshapes = tuple(tuple(t.shape) for t in fine) + (tuple(lg.shape),)
            cshapes = tuple(tuple(t.shape) for t in coarse) + (tuple(lg.shape),)
            for need in NEEDS:
                ref = K.critic_input_bwd(dout, fshapes, tile_a, need=need)
                ref = [None if t is None else K.ps_bwd(t, R8, c) for t, c in zip(ref[:4], chans)] + [ref[4]]
                out = K.critic_input_ps_bwd(dout, cshapes, tile_a, R8, need=need)
                for j in range(5):
                    assert (out[j] is None) == (not need[j]), need
                    assert out[j] is None or (out[j].shape == ref[j].shape and torch.equal(out[j], ref[j])), (shape, chans, tile_a, ncls, need, j)


@pytest.mark.parametrize("shape", PAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", PAD_CASES, ids=lambda c: "r%d-nc%d-p%d" % c)
def test_ps_pad(dev, shape, case):
    K = pkg("kernels")
    (N, A, B), (r, nc, p) = shape, case
    assert K.ps_pad_served(r, nc, p)
    n = N * A * B * nc * r * r
    x = torch.arange(n, dtype=torch.float32, device=dev).reshape(N, A, B, nc * r * r)      # every element distinguishable
    want = K.sympad_fwd(K.ps_fwd(x, r, nc), p)
    got = K.ps_pad_fwd(x, r, nc, p)
    assert got.shape == want.shape and torch.equal(got, want), (shape, case)
    # backward: values of mixed sign and magnitude, so that the up to nine terms of a corner sum and the three of an edge sum round
    # differently in another order
    g = _gen(10 * A + B + r + nc + p, dev)
    dxp = _randn(g, *want.shape) * torch.exp(3.0 * _randn(g, *want.shape))
    ref = K.ps_bwd(K.sympad_bwd(dxp, p), r, nc)
    out = K.ps_pad_bwd(dxp, r, nc, p)
    assert out.shape == ref.shape == x.shape and torch.equal(out, ref), (shape, case)
    if p:       # (the sums are not all trivial: a corner pixel differs from its un-mirrored value)
        assert not torch.equal(out, K.ps_bwd(dxp[:, p:-p, p:-p, :].contiguous(), r, nc))


def test_functions_through_autograd(dev):
    """PSPadFn / CriticInputPsFn against PSFn + SymPadFn / PSFn x4 + CriticInputFn: same outputs, same gradients, bit for bit"""
    F = pkg("functional")
    g = _gen(7, dev)
    N, A, B = 2, 2, 3
    x = (_randn(g, N, A, B, 40 * 64) * 0.1).requires_grad_(True)
    dyp = _randn(g, N, A * 8 + 4, B * 8 + 4, 40)
    y1 = F.PSPadFn.apply(x, 8, 40, 2)
    (g1,) = torch.autograd.grad(y1, x, dyp)
    y0 = F.SymPadFn.apply(F.PSFn.apply(x, 8, 40), 2)
    (g0,) = torch.autograd.grad(y0, x, dyp)
    assert torch.equal(y1, y0) and torch.equal(g1, g0)

    chans = (2, 4, 8, 8)
    coarse = [(_randn(g, N, A, B, c * 64)).requires_grad_(i != 1) for i, c in enumerate(chans)]      # b takes no gradient
    lg = _randn(g, N, A * 8, B * 8, 5).requires_grad_(True)
    dout = _randn(g, N, A * 8, B * 8, 32)
    wrt = [t for t in coarse if t.requires_grad] + [lg]
    o1 = F.CriticInputPsFn.apply(*coarse, lg, 3, 8)
    o0 = F.CriticInputFn.apply(*(F.PSFn.apply(t, 8, c) for t, c in zip(coarse, chans)), lg, 3)
    assert torch.equal(o1, o0)
    for a, b in zip(torch.autograd.grad(o1, wrt, dout), torch.autograd.grad(o0, wrt, dout)):
        assert torch.equal(a, b)


def test_switch_leaves_the_segmenter_logits_alone(dev):
    """a B = 2 segmenter forward (its head goes through ops.PS_conv2d) under both settings of functional.PS_FUSE: the same bits.
    Inference-mode batch norm: two training-mode forwards of one network differ in the last bits whatever the setting"""
    F, ss = pkg("functional"), pkg("source_segmenter")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=2, device=dev,
                      cost_kwargs={"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0})
    x = _randn(_gen(11, dev), 2, 256, 256, 3)
    prev, outs = F.PS_FUSE, {}
    try:
        for fuse in (True, False):
            F.PS_FUSE = fuse
            with torch.no_grad():
                outs[fuse] = net.forward(x, keep_prob=1.0, main_bn=False, adapt_bn=False)
    finally:
        F.PS_FUSE = prev
    assert outs[True].shape == (2, 256, 256, 5) and float(outs[True].abs().max()) > 0.0
    assert torch.equal(outs[True], outs[False])
