"""The ResNet stems without their stem-resolution activation: BatchNorm + ReLU inside the pooling pass
(ops.stem_bn_relu_maxpool) and a BatchNorm backward fed by the pooled gradient (ops.stem_bn_bwd_pooled).

The reference is always the op sequence these replace, run in the same test on the same inputs (bn_apply + maxpool_fwd;
maxpool_bwd + bn_bwd with the written activation as the ReLU mask).  The new kernels keep those kernels' expressions, comparison
order, row partition and fp64 combine order, so every comparison is torch.equal - no tolerance anywhere.  The stem convolution and
its weight gradient are the unchanged im2col + GEMM pair: with a bit-identical dco their outputs are bit-identical too."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 64


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _bits(t):
    """Bit pattern, so that NaNs compare equal to themselves and -0.0 differs from 0.0."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _bn_params(g):
    mean = torch.randn(C, device=DEV, generator=g) * 0.3
    rstd = torch.rand(C, device=DEV, generator=g) + 0.5
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta = torch.randn(C, device=DEV, generator=g) * 0.2
    gamma[3] = -gamma[3]          # a negative scale flips which inputs survive the ReLU
    return mean, rstd, gamma, beta


def _co(kind, B, H, W, g):
    co = torch.randn(B, H, W, C, device=DEV, generator=g) * 2
    if kind == "ties":
        # coarse values: about half of every window is exactly 0 after the ReLU and the positive maxima repeat inside a window,
        # so the first-maximum rule decides most argmax taps
        co = torch.round(co)
    elif kind == "nan":
        co[0, 5, 7, 11] = float("nan")
        co[B - 1, H - 1, W - 1, 63] = float("nan")
    return co


def _old_fwd(ops, co, mean, rstd, gamma, beta):
    B, H, W, _ = co.shape
    M = B * H * W
    y = torch.empty_like(co)
    ops.bn_apply(co.view(M, C), y.view(M, C), mean, rstd, gamma, beta, True)
    pooled = torch.empty(B, (H + 1) // 2, (W + 1) // 2, C, device=DEV)
    idx = torch.empty(pooled.shape, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(y, pooled, idx)
    return y, pooled, idx


@pytest.mark.parametrize("kind", ["plain", "ties", "nan"])
@pytest.mark.parametrize("B,H,W", [(2, 128, 128), (32, 128, 128), (3, 6, 10)])
def test_bn_relu_maxpool_is_bit_identical_to_apply_then_pool(B, H, W, kind):
    from mmfn_amd import ops
    g = _gen(B * 1000 + H + len(kind))
    mean, rstd, gamma, beta = _bn_params(g)
    if kind == "ties":   # an affine map that keeps the coarse values coarse: exact zeros and exact repeats after the ReLU
        mean, rstd, gamma, beta = torch.zeros_like(mean), torch.ones_like(rstd), torch.ones_like(gamma), torch.zeros_like(beta)
    co = _co(kind, B, H, W, g)
    assert ops.stem_pool_ok(co.shape)
    y, pooled_ref, idx_ref = _old_fwd(ops, co, mean, rstd, gamma, beta)
    pooled = torch.full_like(pooled_ref, float("nan"))
    idx = torch.full_like(idx_ref, 255)
    ops.stem_bn_relu_maxpool(co, mean, rstd, gamma, beta, pooled, idx)
    torch.cuda.synchronize()
    if kind == "ties":
        assert (pooled_ref == 0).float().mean().item() > 0.01 and (idx_ref != 0).any()
    assert torch.equal(_bits(pooled), _bits(pooled_ref))
    assert torch.equal(idx, idx_ref)


@pytest.mark.parametrize("kind", ["plain", "ties"])
@pytest.mark.parametrize("B,H,W", [(2, 128, 128), (32, 128, 128), (3, 6, 10)])
def test_bn_bwd_from_pooled_gradient_is_bit_identical(B, H, W, kind):
    """dgamma, dbeta and dco against maxpool_bwd + bn_bwd: the old path gets the written activation y as its ReLU mask, the new one
    gets neither y nor the stem-resolution gradient."""
    from mmfn_amd import ops
    g = _gen(B * 77 + W + len(kind))
    mean, rstd, gamma, beta = _bn_params(g)
    if kind == "ties":
        mean, rstd, gamma, beta = torch.zeros_like(mean), torch.ones_like(rstd), torch.ones_like(gamma), torch.zeros_like(beta)
    co = _co(kind, B, H, W, g)
    M = B * H * W
    y, pooled, idx = _old_fwd(ops, co, mean, rstd, gamma, beta)
    gp = torch.randn(pooled.shape, device=DEV, generator=g)
    gy = torch.empty_like(co)
    ops.maxpool_bwd(gp, idx, gy)
    dco_ref, dg_ref, db_ref = torch.empty_like(co), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.bn_bwd(gy.view(M, C), y.view(M, C), co.view(M, C), mean, rstd, gamma, dco_ref.view(M, C), dg_ref, db_ref)
    dco, dg, db = torch.full_like(co, float("nan")), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ops.stem_bn_bwd_pooled(gp, idx, co, mean, rstd, gamma, beta, dco, dg, db)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dg), _bits(dg_ref)) and torch.equal(_bits(db), _bits(db_ref))
    assert torch.equal(_bits(dco), _bits(dco_ref))


def test_entries_refuse_what_they_do_not_take():
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    assert not ops.stem_pool_ok((2, 125, 125, C))          # odd extents (a 250 x 250 frame)
    assert not ops.stem_pool_ok((2, 128, 128, 6))          # channels not a multiple of four
    assert not ops.stem_pool_ok((2, 128, 128, C), torch.bfloat16)
    g = _gen(5)
    mean, rstd, gamma, beta = _bn_params(g)
    co = torch.randn(2, 5, 8, C, device=DEV, generator=g)
    pooled = torch.empty(2, 3, 4, C, device=DEV)
    idx = torch.empty(pooled.shape, dtype=torch.uint8, device=DEV)
    with pytest.raises(MMFNLibraryError):
        ops.stem_bn_relu_maxpool(co, mean, rstd, gamma, beta, pooled, idx)
    with pytest.raises(MMFNLibraryError):
        ops.stem_bn_bwd_pooled(pooled, idx, co, mean, rstd, gamma, beta, torch.empty_like(co), torch.empty(C, device=DEV),
                               torch.empty(C, device=DEV))
    co = torch.randn(2, 8, 8, C, device=DEV, generator=g)
    with pytest.raises(MMFNLibraryError):   # NULL operand
        ops.stem_bn_relu_maxpool(co, mean, rstd, gamma, None, torch.empty(2, 4, 4, C, device=DEV), torch.empty(2, 4, 4, C, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------ through the engine's stem (ResNetTrunk.stem_fwd / stem_bwd)
class _Layout(object):
    def __init__(self, cin, g):
        self.p = {"conv1.weight": torch.randn(C, 7, 7, cin, device=DEV, generator=g) * 0.1,
                  "bn1.weight": torch.rand(C, device=DEV, generator=g) + 0.5,
                  "bn1.bias": torch.randn(C, device=DEV, generator=g) * 0.2}
        self.gr = {k: torch.full_like(v, float("nan")) for k, v in self.p.items()}

    def w(self, name):
        return self.p[name]

    def g(self, name):
        return self.gr[name]


def _trunk(cin, seed):
    """A ResNetTrunk that is only its stem (the layers are not touched by stem_fwd / stem_bwd)."""
    from mmfn_amd import engine
    g = _gen(seed)
    lay = _Layout(cin, g)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    t = engine.ResNetTrunk.__new__(engine.ResNetTrunk)
    t.name = "t%d" % cin
    t.stem = engine.ConvBN(t.name + ".stem", lay, "conv1", "bn1", bn, 2, 3)
    t.layers = {}
    ctx = engine.Ctx(engine.Buffers(DEV), True, (0.0, 0.0, 0.0), None)
    return t, lay, bn, ctx


def _stem_step(trunk, lay, bn, ctx, x, gp):
    p = trunk.stem_fwd(ctx, x)
    out = [p.clone(), trunk.pool_saved[1].clone(), trunk.stem.saved[3].clone(), trunk.stem.saved[4].clone()]
    trunk.stem_bwd(ctx, gp)
    torch.cuda.synchronize()
    out += [lay.gr[k].clone() for k in sorted(lay.gr)]
    out += [bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]
    return out


@pytest.mark.parametrize("cin", [3, 2])
@pytest.mark.parametrize("B,S", [(2, 256), (32, 256), (2, 250)])
def test_engine_stem_matches_the_unfused_sequence(cin, B, S, monkeypatch):
    """Both real stem geometries (camera 3 channels, LiDAR 2; 256 x 256 frames, B = 2 and the benched B = 32) and a frame size the
    predicate refuses (250 x 250 -> a 125 x 125 convolution output): pooled output, argmax taps, batch and running statistics and
    all three parameter gradients of one training step, against the same step with the fusion switched off."""
    from mmfn_amd import ops
    g = _gen(cin * 100 + B + S)
    x = torch.randn(B, S, S, cin, device=DEV, generator=g)
    gp = torch.randn(B, S // 4 + (1 if S % 4 else 0), S // 4 + (1 if S % 4 else 0), C, device=DEV, generator=g)
    trunk, lay, bn, ctx = _trunk(cin, 7)
    got = _stem_step(trunk, lay, bn, ctx, x, gp)
    took_fused = trunk.pool_saved[0] is None
    assert took_fused == (S == 256)
    if took_fused:   # the activation and its gradient were never allocated
        names = {k[0] for k in ctx.bufs._bufs}
        assert trunk.name + ".stem.out" not in names and trunk.name + ".dpool" not in names
    monkeypatch.setattr(ops, "stem_pool_ok", lambda *a, **k: False)
    trunk2, lay2, bn2, ctx2 = _trunk(cin, 7)
    ref = _stem_step(trunk2, lay2, bn2, ctx2, x, gp)
    assert trunk2.pool_saved[0] is not None
    assert tuple(got[0].shape) == tuple(gp.shape)
    for a, b in zip(got, ref):
        assert not torch.isnan(a.float()).any()
        assert torch.equal(_bits(a), _bits(b))


def test_eval_forward_matches_the_unfused_sequence(monkeypatch):
    """Unfolded eval: the same pass over the running statistics."""
    from mmfn_amd import ops
    g = _gen(11)
    x = torch.randn(2, 256, 256, 3, device=DEV, generator=g)
    outs = []
    for fused in (True, False):
        if not fused:
            monkeypatch.setattr(ops, "stem_pool_ok", lambda *a, **k: False)
        trunk, lay, bn, ctx = _trunk(3, 9)
        with torch.no_grad():
            bn.running_mean.copy_(torch.randn(C, device=DEV, generator=_gen(1)) * 0.1)
            bn.running_var.copy_(torch.rand(C, device=DEV, generator=_gen(2)) + 0.5)
        ctx.training = False
        outs.append(trunk.stem_fwd(ctx, x).clone())
        assert (trunk.pool_saved[0] is None) == fused
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


def test_stem_step_replays_inside_a_captured_graph():
    """One stem forward + backward captured with torch.cuda.graph and replayed on fresh inputs equals the eager run."""
    g = _gen(21)
    B = 2
    x = torch.randn(B, 256, 256, 3, device=DEV, generator=g)
    gp = torch.randn(B, 64, 64, C, device=DEV, generator=g)
    trunk, lay, bn, ctx = _trunk(3, 3)
    xs, gs = x.clone(), gp.clone()
    _stem_step(trunk, lay, bn, ctx, xs, gs)          # eager first: allocates every buffer
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st, capture_error_mode="thread_local"):
            p = trunk.stem_fwd(ctx, xs)
            trunk.stem_bwd(ctx, gs)
    assert trunk.pool_saved[0] is None
    x2 = torch.randn(B, 256, 256, 3, device=DEV, generator=g)
    g2 = torch.randn(B, 64, 64, C, device=DEV, generator=g)
    xs.copy_(x2)
    gs.copy_(g2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [p.clone()] + [lay.gr[k].clone() for k in sorted(lay.gr)]
    trunk2, lay2, bn2, ctx2 = _trunk(3, 3)
    ref = _stem_step(trunk2, lay2, bn2, ctx2, x2, g2)
    assert torch.equal(_bits(got[0]), _bits(ref[0]))
    for a, b in zip(got[1:], ref[4:7]):
        assert torch.equal(_bits(a), _bits(b))
