"""The statistics and fold kernels of the ResNet trunks' fp32 path against plain torch in float64 (CPU) on the same fp32 inputs:
the Winograd output transform that emits BatchNorm batch statistics (mmfn_wino_output_stats_f32 + mmfn_bn_finalize_stats_f32),
mmfn_bn_train_stats_f32 at the edges of col_partial_kernel / bn_grid, bn_bwd and bn_bwd_reduce in their three mask modes, the
grouped filter transform (mmfn_wino_weight_group_f32), bn_fold and bn_eval_prepare.

Every output buffer is NaN-filled before the call.  Tolerances: 2e-6 * max |y| between two output transforms (the fma-contraction
allowance of test_gemm_gpu.py), 1e-6 for statistics (test_batchnorm_train_and_backward's bound; the sums are fp64), 2e-5 for the
BatchNorm backward (test_kernels_gpu.py).  Each comparison prints its error (profiles/trunk_tests_err.txt)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = "code -1"   # MMFN_EINVAL as ops._call reports it
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32).double())   # what the kernels add: the float argument widened to double
MOM = 0.1
MOM32 = float(torch.tensor(MOM, dtype=torch.float32).double())
NAN = float("nan")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _cpu(t):
    return t.detach().cpu().double()


def _close(got, ref, tol, what):
    """max |got - ref| <= tol * (max |ref| + 1e-6)"""
    got, ref = _cpu(got), ref.detach().double()
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    print("trunk-err kernel | %s | err/scale %.3g | tol %.3g" % (what, err / scale, tol))
    assert torch.isfinite(got).all(), what
    assert err <= tol * scale, "%s max err %g vs scale %g" % (what, err, scale)


def _rel(got, ref, tol, what):
    """element-wise relative"""
    got, ref = _cpu(got), ref.detach().double()
    err = ((got - ref).abs() / ref.abs()).max().item()
    print("trunk-err kernel | %s | max rel err %.3g | tol %.3g" % (what, err, tol))
    assert torch.isfinite(got).all(), what
    assert err <= tol, "%s max relative err %g" % (what, err)


def _spy(monkeypatch):
    from mmfn_amd import ops
    taken, real = [], ops._call

    def spy(name, *a):
        taken.append(name)
        return real(name, *a)

    monkeypatch.setattr(ops, "_call", spy)
    return taken


def _running(C, g):
    return torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5


def _check_stats(x2d64, mean, rstd, rm0, rv0, rm, rv, nbt, nbt0, what, rstd_tol=1e-6):
    """mean / rstd / running statistics / step counter against the float64 statistics of x2d64 [M, C] (two-pass)."""
    M = x2d64.shape[0]
    mu = x2d64.mean(0)
    var = ((x2d64 - mu) ** 2).mean(0)
    std = var.sqrt()
    err = ((_cpu(mean) - mu).abs() / (mu.abs() + std + 1e-30)).max().item()
    print("trunk-err kernel | %s mean | err/(|ref|+std) %.3g | tol %.3g" % (what, err, 1e-6))
    assert torch.isfinite(mean).all() and err <= 1e-6, "%s mean: %g" % (what, err)
    _rel(rstd, (var + EPS32).rsqrt(), rstd_tol, what + " rstd")
    unbiased = var * M / (M - 1) if M > 1 else var          # a single row: the kernels keep the biased (zero) variance
    _close(rm, (1.0 - MOM32) * rm0.double() + MOM32 * mu, 1e-6, what + " running_mean")
    _close(rv, (1.0 - MOM32) * rv0.double() + MOM32 * unbiased, 1e-6, what + " running_var")
    assert int(nbt.item()) == nbt0 + 1, what + " num_batches_tracked"


# ------------------------------------------------------------------ a. output transform with statistics
@pytest.mark.parametrize("B,H,W,C", [(1, 4, 4, 16), (1, 4, 8, 64), (17, 4, 4, 64), (2, 8, 12, 128), (9, 64, 64, 256), (3, 64, 64, 1024)])
def test_wino_output_stats_and_finalize_against_fp64(B, H, W, C):
    """T = 1 with 63 idle tile lanes; T = 2 < TL; T = TL + 1 (a ragged block); H != W; T > 512 * TL (tpb = 5, 461 blocks, the last one
    short); TL = 1 with tpb = 2."""
    from mmfn_amd import ops
    from mmfn_amd._lib import ptr, stream
    g = _g(B * 1000 + H + W + C)
    T = B * (H // 4) * (W // 4)
    Mt = (torch.randn(36, T, C, generator=g) + 0.5 * torch.randn(C, generator=g)).to(DEV)
    rm0, rv0 = _running(C, g)
    rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor([3], dtype=torch.int64, device=DEV)
    y, y_plain, mean, rstd = _nan(B, H, W, C), _nan(B, H, W, C), _nan(C), _nan(C)
    ws = ops.norm_workspace(DEV)
    ws.fill_(NAN)      # a partial row the transform did not write poisons the finalize
    nblk = ctypes.c_int(-1)
    ops._call("mmfn_wino_output_stats_f32", ptr(Mt), ptr(y), ptr(ws), ctypes.cast(ctypes.pointer(nblk), ctypes.c_void_p), B, H, W, C, stream())
    TL = 256 // (C // 4)
    tpb = max(TL, (T + 511) // 512)
    assert nblk.value == (T + tpb - 1) // tpb
    ops.bn_finalize_stats(ws, nblk.value, B * H * W, C, mean, rstd, rm, rv, nbt, EPS, MOM)
    ops._call("mmfn_wino_output_f32", ptr(Mt), None, ptr(y_plain), B, H, W, C, 4, stream())
    torch.cuda.synchronize()
    what = "wino_output_stats (%d,%d,%d,%d)" % (B, H, W, C)
    _close(y, _cpu(y_plain), 2e-6, what + " y vs plain transform")
    _check_stats(_cpu(y).view(-1, C), mean, rstd, rm0, rv0, rm, rv, nbt, 3, what)


@pytest.mark.parametrize("C", [48, 2048])
def test_wino_output_stats_refuses_channel_counts_it_cannot_lane(C):
    """256 % (C / 4) != 0, and C / 4 above the block: MMFN_EINVAL before anything is launched."""
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError, ptr, stream
    Mt, y = torch.zeros(36, 1, C, device=DEV), _nan(1, 4, 4, C)
    nblk = ctypes.c_int(-1)
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops._call("mmfn_wino_output_stats_f32", ptr(Mt), ptr(y), ptr(ops.norm_workspace(DEV)),
                  ctypes.cast(ctypes.pointer(nblk), ctypes.c_void_p), 1, 4, 4, C, stream())
    torch.cuda.synchronize()
    assert nblk.value == -1 and torch.isnan(y).all()


@pytest.mark.parametrize("Co,fused", [(96, False), (64, True)])
def test_conv2d_fwd_bn_stats_fused_and_fallback(Co, fused, monkeypatch):
    """Co = 96: 256 % (Co / 4) != 0, so the statistics must come from the plain output transform + bn_train_stats; Co = 64 takes
    the statistics-emitting transform.  Either way: the convolution against float64 and the statistics of what was written.

    mmfn_bn_train_stats_f32 refuses C = 96 itself (test_bn_kernels_refuse_channel_counts_they_cannot_lane), so the fallback hands
    it the output widened with zero columns to 128 channels and copies the 96 real statistics back."""
    from mmfn_amd import ops
    g = _g(Co)
    B, H, W, Ci = 2, 8, 8, 64
    x = torch.randn(B, H, W, Ci, generator=g)
    w = torch.randn(Co, 3, 3, Ci, generator=g) * (2.0 / (9 * Ci)) ** 0.5
    rm0, rv0 = _running(Co, g)
    rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor([0], dtype=torch.int64, device=DEV)
    out, mean, rstd = _nan(B, H, W, Co), _nan(Co), _nan(Co)
    taken = _spy(monkeypatch)
    ops.conv2d_fwd_bn_stats(x.to(DEV), w.to(DEV), 1, 1, out, mean, rstd, rm, rv, nbt, EPS, MOM)
    torch.cuda.synchronize()
    if fused:
        assert "mmfn_wino_output_stats_f32" in taken and "mmfn_bn_finalize_stats_f32" in taken
        assert "mmfn_bn_train_stats_f32" not in taken and "mmfn_wino_output_f32" not in taken
    else:
        assert "mmfn_wino_output_f32" in taken and "mmfn_bn_train_stats_f32" in taken
        assert "mmfn_wino_output_stats_f32" not in taken and "mmfn_bn_finalize_stats_f32" not in taken
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    what = "conv2d_fwd_bn_stats Co=%d" % Co
    _close(out, ref, 2e-5, what + " conv")
    _check_stats(_cpu(out).view(-1, Co), mean, rstd, rm0, rv0, rm, rv, nbt, 0, what)


# ------------------------------------------------------------------ b. bn_train_stats at the edges
def _exact_mean(x):
    """Nudge row 0 of each column (by less than 2^-6) so that the column mean of x ~ 100 is itself an fp32 number: the fp32 `mean`
    a BatchNorm backward is handed then carries no rounding, which at mean / std = 1e4 would otherwise shift xhat by up to 4e-4."""
    M = x.shape[0]
    assert M == 2048 and (x > 64).all() and (x < 128).all()       # values are multiples of 2^-17; the mean must become one
    s = x.double().sum(0)
    x = x.clone()
    x[0] -= torch.remainder(s, 2.0 ** -6).float()
    assert (x > 64).all() and (x < 128).all()
    mu = x.double().mean(0)
    assert torch.equal(mu.float().double(), mu)
    return x


def _bn_input(kind, M, C, g):
    if kind == "offset":     # mean^2 / var = 1e8: a float accumulation of sum and sum of squares loses the variance entirely
        return 100.0 + 0.01 * torch.randn(M, C, generator=g)
    x = torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) * 2 + 0.5) + torch.randn(C, generator=g) * 1.5
    if kind == "const":      # two constant channels (one of them not a short binary fraction): variance 0, or rounding below 0
        x[:, 1] = 3.25
        x[:, C - 2] = 0.1
    return x


BN_SHAPES = [("plain", 1, 64), ("plain", 33, 4), ("plain", 77, 1024), ("plain", 40000, 64), ("offset", 2048, 64), ("const", 512, 64)]


@pytest.mark.parametrize("kind,M,C", BN_SHAPES)
def test_bn_train_stats_edges_against_fp64(kind, M, C):
    """M = 1 (the unbiased variance falls back to the biased one); cq = 1 with 256 row lanes and one short block; cq = 256 with one
    row lane; rows_per_block above its floor of 32; mean^2 / var = 1e8; zero variance (rstd = 1 / sqrt(eps), no NaN)."""
    from mmfn_amd import ops
    g = _g(M + C)
    x = _bn_input(kind, M, C, g)
    rm0, rv0 = _running(C, g)
    rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor([5], dtype=torch.int64, device=DEV)
    mean, rstd = _nan(C), _nan(C)
    ops.norm_workspace(DEV).fill_(NAN)
    ops.bn_train_stats(x.to(DEV), mean, rstd, rm, rv, nbt, EPS, MOM)
    torch.cuda.synchronize()
    what = "bn_train_stats %s (%d,%d)" % (kind, M, C)
    _check_stats(x.double(), mean, rstd, rm0, rv0, rm, rv, nbt, 5, what, rstd_tol=1e-5 if kind == "offset" else 1e-6)
    if kind == "const":
        for c in (1, C - 2):
            assert abs(rstd[c].item() * EPS32 ** 0.5 - 1.0) <= 1e-6, "zero variance: rstd = 1 / sqrt(eps)"
    if M == 1:
        assert abs(rstd.double().cpu() * EPS32 ** 0.5 - 1.0).max().item() <= 1e-6


@pytest.mark.parametrize("C", [96, 1028])
def test_bn_kernels_refuse_channel_counts_they_cannot_lane(C):
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    M = 8
    x, v = torch.zeros(M, C, device=DEV), torch.ones(C, device=DEV)
    mean, rstd, dx = _nan(C), _nan(C), _nan(M, C)
    nbt = torch.tensor([0], dtype=torch.int64, device=DEV)
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops.bn_train_stats(x, mean, rstd, v.clone(), v.clone(), nbt)
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops.bn_bwd(x, None, x, v, v, v, dx, _nan(C), _nan(C))
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops.bn_bwd_reduce(x, None, x, v, v, _nan(C), _nan(C), _nan(2, C))
    torch.cuda.synchronize()
    assert torch.isnan(mean).all() and torch.isnan(dx).all() and int(nbt.item()) == 0


# ------------------------------------------------------------------ c. bn_bwd / bn_bwd_reduce in the three mask modes
_bwd_refs = {}


def _bwd_ref(kind, M, C):
    """Inputs and the float64 autograd of sum(relu(bn(x)) * g) and of sum(bn(x) * g), computed once per shape."""
    key = (kind, M, C)
    if key in _bwd_refs:
        return _bwd_refs[key]
    g = _g(7 * M + C)
    x = _bn_input(kind, M, C, g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    w[0] = -w[0]           # a negative scale flips which inputs survive the ReLU
    gy = torch.randn(M, C, generator=g)

    def bn64(xx, ww, bb):
        mu = xx.mean(0)
        var = ((xx - mu) ** 2).mean(0)
        rs = (var + EPS32).rsqrt()
        return (xx - mu) * rs * ww + bb, mu, rs

    # keep every |bn(x)| away from zero, so that the sign recomputed in fp32 is the sign of the reference: move the few offenders.
    # The kernels evaluate bn(x) as fma(x, alpha, beta) with alpha = w * rstd and beta = b - mean * alpha rounded to fp32 (the
    # forward's own expression: the recomputed mask must be the forward's), which is off by a few 2^-24 * (|mean * alpha| + |beta|):
    # 2e-3 at mean / std = 1e4.  Eight times that, and at least 2e-4, is the distance kept.
    for _ in range(20):
        if kind == "offset":
            x = _exact_mean(x)
        z, mu, rs = bn64(x.double(), w.double(), b.double())
        alpha = rs * w.double()
        thr = (8 * 2.0 ** -24 * ((mu * alpha).abs() + (b.double() - mu * alpha).abs())).clamp(min=2e-4)
        near = z.abs() < thr
        if kind == "const":
            near[:, 1] = near[:, C - 2] = False
        if not near.any():
            break
        sgn = torch.where(z >= 0, 1.0, -1.0).double()
        x = torch.where(near, (x.double() + (1.5 * thr * sgn - z) / alpha).float(), x)
    out = {"x": x, "w": w, "b": b, "g": gy}
    for relu in (True, False):
        x64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (x, w, b))
        z, mu, rs = bn64(x64, w64, b64)
        (torch.relu(z) if relu else z).mul(gy.double()).sum().backward()
        ge = gy.double() * (z.detach() > 0).double() if relu else gy.double()
        xhat = (x64.detach() - mu.detach()) * rs.detach()
        out[relu] = dict(z=z.detach(), dx=x64.grad, dw=w64.grad, db=b64.grad, ge=ge, means=torch.stack([ge.mean(0), (ge * xhat).mean(0)]))
    out["mean"], out["rstd"] = mu.detach().float(), rs.detach().float()
    _bwd_refs[key] = out
    return out


@pytest.fixture(scope="module", autouse=True)
def _release_refs():
    yield
    _bwd_refs.clear()


@pytest.mark.parametrize("mode", ["y", "recompute", "none"])
@pytest.mark.parametrize("kind,M,C", [s for s in BN_SHAPES if s[1] > 1])
def test_bn_bwd_and_reduce_against_fp64_autograd(kind, M, C, mode):
    """dx, ge_out, dweight, dbias of bn_bwd and dweight, dbias, means of bn_bwd_reduce, with the ReLU mask read from y, recomputed
    from x (relu_bias) and absent."""
    from mmfn_amd import ops
    R = _bwd_ref(kind, M, C)
    relu = mode != "none"
    ref = R[relu]
    z = R[True]["z"]
    if kind == "const":    # the constant channels sit at bn(x) = bias exactly
        z = z[:, [c for c in range(C) if c not in (1, C - 2)]]
        assert (R["b"][[1, C - 2]].abs() >= 1e-4).all()
    assert z.abs().min().item() >= 1e-4, "a property of the inputs: no bn(x) within 1e-4 of zero"
    x, g, w, b, mean, rstd = (R[k].to(DEV) for k in ("x", "g", "w", "b", "mean", "rstd"))
    y = torch.relu(R[True]["z"]).float().to(DEV) if mode == "y" else None
    relu_bias = b if mode == "recompute" else None
    what = "bn_bwd %s (%d,%d) mask=%s" % (kind, M, C, mode)
    dx, ge, dw, db = _nan(M, C), _nan(M, C), _nan(C), _nan(C)
    ops.norm_workspace(DEV).fill_(NAN)
    ops.bn_bwd(g, y, x, mean, rstd, w, dx, dw, db, ge_out=ge, relu_bias=relu_bias)
    torch.cuda.synchronize()
    _close(dx, ref["dx"], 2e-5, what + " dx")
    _close(ge, ref["ge"], 2e-5, what + " ge_out")
    _close(dw, ref["dw"], 2e-5, what + " dweight")
    _close(db, ref["db"], 2e-5, what + " dbias")
    assert torch.equal(_cpu(ge), ref["ge"]), "ge_out is g or exactly 0"
    dw2, db2, means = _nan(C), _nan(C), _nan(2, C)
    ops.norm_workspace(DEV).fill_(NAN)
    ops.bn_bwd_reduce(g, y, x, mean, rstd, dw2, db2, means, relu_wb=None if relu_bias is None else (w, relu_bias))
    torch.cuda.synchronize()
    what = "bn_bwd_reduce %s (%d,%d) mask=%s" % (kind, M, C, mode)
    _close(dw2, ref["dw"], 2e-5, what + " dweight")
    _close(db2, ref["db"], 2e-5, what + " dbias")
    _close(means[0], ref["means"][0], 1e-6, what + " means[0] = mean(ge)")
    _close(means[1], ref["means"][1], 1e-6, what + " means[1] = mean(ge * xhat)")
    dx_nomask = _nan(M, C)
    ops.bn_bwd(g, y, x, mean, rstd, w, dx_nomask, _nan(C), _nan(C), relu_bias=relu_bias)      # the instantiation without ge_out
    torch.cuda.synchronize()
    assert torch.equal(dx_nomask, dx)


# ------------------------------------------------------------------ d. grouped filter transform
def test_wino_weight_group_is_bit_equal_to_the_per_layer_transform():
    """Four layers in one table; (16, 20) puts the starts of the layers after it off the 256-thread grid.  Each U bit-equal to the
    per-layer F(4x4) transform, the word after each U untouched."""
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError, ptr, stream
    g = _g(4)
    layers = [(64, 64), (128, 64), (16, 20), (256, 128)]
    ws = [torch.randn(co, 3, 3, ci, generator=g).to(DEV) for co, ci in layers]
    us = [_nan(36 * co * ci + 1) for co, ci in layers]
    table, n, total = ops.make_wino_group_table([(w, u) for w, u in zip(ws, us)], DEV)
    assert n == 4 and total == sum(co * ci for co, ci in layers) and (64 * 64 + 128 * 64 + 16 * 20) % 256 != 0
    ops.wino_weight_group(table, n, total)
    torch.cuda.synchronize()
    for (co, ci), w, u in zip(layers, ws, us):
        ref = _nan(36 * co * ci)
        ops._call("mmfn_wino_weight_f32", ptr(w), ptr(ref), co, ci, 4, stream())
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all()
        same = torch.equal(u[:-1].view(torch.int32), ref.view(torch.int32))
        print("trunk-err kernel | wino_weight_group layer (%d,%d) | bit-equal %s | max diff %.3g" % (co, ci, same, (u[:-1] - ref).abs().max().item()))
        assert same
        assert torch.isnan(u[-1]).item(), "guard word after U"
    for bad_n, bad_total in ((0, total), (n, 0)):
        with pytest.raises(MMFNLibraryError, match=EINVAL):
            ops.wino_weight_group(table, bad_n, bad_total)


# ------------------------------------------------------------------ e. BatchNorm fold / eval statistics
@pytest.mark.parametrize("Cout,K", [(64, 147), (64, 576), (128, 64), (512, 4608)])
def test_bn_fold_and_eval_prepare_against_fp64(Cout, K):
    """Stem (7x7x3), 3x3x64, 1x1 downsample and 3x3x512 filters: K below, equal to a multiple of and far above the 256-thread block."""
    from mmfn_amd import ops
    g = _g(Cout + K)
    w = torch.randn(Cout, K, generator=g)
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    gamma[0] = -gamma[0]
    rm, rv = torch.randn(Cout, generator=g) * 0.3, torch.rand(Cout, generator=g) * 2 + 0.01
    rv[1] = 0.0            # a dead channel: only eps keeps the scale finite
    wf, bf, mean, rstd = _nan(Cout, K), _nan(Cout), _nan(Cout), _nan(Cout)
    ops.bn_fold(w.to(DEV), gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), EPS, wf, bf)
    ops.bn_eval_prepare(rm.to(DEV), rv.to(DEV), mean, rstd, EPS)
    torch.cuda.synchronize()
    rs = (rv.double() + EPS32).rsqrt()
    s = gamma.double() * rs
    what = "bn_fold (%d,%d)" % (Cout, K)
    _close(wf, w.double() * s[:, None], 1e-6, what + " filter")
    _close(bf, beta.double() - rm.double() * s, 1e-6, what + " shift")
    _rel(rstd, rs, 1e-6, "bn_eval_prepare (%d) rstd" % Cout)
    assert torch.equal(mean.cpu(), rm)
