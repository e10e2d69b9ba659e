"""The convolution forms of mmfn_gemm_bf16 (implicit GEMM forward, data gradient in its three gathers - lean, parity tiles, plain
strided - and the weight gradient) and mmfn_conv3x3_halo_bf16 against float64 F.conv2d / its autograd on the CPU, with the error
budget, the two bf16 assertions and the statistics bounds of tests/test_gemm16_fp64_gpu.py (whose helper this file imports; its
docstring derives them).  Every output buffer is NaN-filled before the call; tile / stages / splitk are always explicit; each
comparison prints one `bf16-err` line (profiles/bf16_gemm_tests_err.txt)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gemm16_fp64_gpu as H   # noqa: E402  (the shared reference / budget helper)

pytestmark = pytest.mark.gpu
DEV = H.DEV
BF = H.BF
U = H.U


def _nchw(t):
    return t.double().permute(0, 3, 1, 2).contiguous()


def _nhwc2d(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


_refs = {}


def conv_refs(geom, seed=0):
    """inputs (bf16, CPU, NHWC) and the float64 forward / data gradient / weight gradient of one geometry with the same products
    of absolute values, computed once and shared"""
    if geom in _refs:
        return _refs[geom]
    B, Hh, W, Ci, Co, k, s, p = geom
    x, w = H._bf(B, Hh, W, Ci, seed=seed + 1), H._bf(Co, k, k, Ci, scale=0.05, seed=seed + 2)
    OH, OW = (Hh + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = H._bf(B, OH, OW, Co, seed=seed + 3)
    out = {"x": x, "w": w, "dy": dy, "oshape": (B, OH, OW, Co)}
    for tag, f in (("", lambda t: t), ("abs", torch.abs)):
        xn, wn = f(_nchw(x)).requires_grad_(True), f(_nchw(w)).requires_grad_(True)
        y = F.conv2d(xn, wn, stride=s, padding=p)
        gx, gw = torch.autograd.grad(y, (xn, wn), f(_nchw(dy)))
        out["y" + tag], out["dx" + tag], out["dw" + tag] = _nhwc2d(y.detach()), _nhwc2d(gx), gw.permute(0, 2, 3, 1).reshape(Co, -1)
    _refs[geom] = out
    return out


ALL = [(t, s) for t in (1, 2, 3, 4) for s in (2, 3, 4)]
FEW = [(1, 4), (2, 2), (3, 3), (4, 2)]
FWD = [((1, 8, 8, 64, 64, 3, 1, 1), ALL), ((1, 6, 10, 64, 64, 3, 1, 1), FEW), ((3, 5, 7, 64, 128, 3, 2, 1), ALL),
       ((2, 8, 8, 128, 64, 1, 2, 0), FEW), ((1, 4, 4, 256, 64, 3, 1, 1), FEW)]


# ------------------------------------------------------------------ e. the implicit-GEMM forms
def test_convolution_forward_against_fp64():
    """ragged M (64, 60, 36, 32, 16 output pixels), stride 1 and 2, 1x1, K = 2304 (four k-tiles per tap); statistics mode 0"""
    from mmfn_amd import ops16
    worst = 0.0
    for geom, combos in FWD:
        B, Hh, W, Ci, Co, k, s, p = geom
        r = conv_refs(geom)
        K = k * k * Ci
        E = H.acc_budget(r["yabs"], K)
        x, w = r["x"].to(DEV), r["w"].to(DEV)
        M = r["y"].shape[0]
        for tile, stages in combos:
            y = H._nan(*r["oshape"])
            rows = H.gemm_stats_rows(ops16.G16_CONV_FWD, M, Co, K, tile)
            stats = H._nan(rows + 2, 2, Co, dtype=torch.float64)
            ops16.conv2d_fwd(x, w, s, p, y, stats=stats, tile=tile, stages=stages)
            what = "conv fwd %s tile %d stages %d" % (geom, tile, stages)
            worst = max(worst, H.check_bf16(y.view(M, Co), r["y"], E, what, K))
            H.check_stats(stats, rows, ((r["y"], E), None), what)
    print("bf16-err | conv forward | largest err/bound %.3g" % worst)


DGRAD = FWD + [((4, 8, 8, 64, 64, 3, 2, 1), ALL),       # parity tiles at the 64-row tile (M / 4 = 64); plain gather at the 128-row tile
               ((2, 16, 16, 64, 64, 3, 2, 1), FEW),     # parity tiles at both
               ((1, 8, 8, 64, 64, 3, 2, 1), FEW),       # M / 4 = 16: the plain strided gather
               ((1, 9, 9, 64, 64, 3, 2, 1), FEW)]       # odd sides: the plain strided gather


def _dgrad(r, geom, out, **kw):
    from mmfn_amd import ops16
    B, Hh, W, Ci, Co, k, s, p = geom
    w_t = r["w"].permute(3, 1, 2, 0).contiguous().to(DEV)      # the [Ci, kh, kw, Co] shadow
    return ops16.conv2d_dgrad(r["dy"].to(DEV), w_t, (B, Hh, W, Ci), (Co, k, k, Ci), s, p, out, **kw)


def test_convolution_data_gradient_against_fp64():
    """the lean gather (stride 1), parity tiles (stride 2, even sides, (M / 4) % tile rows == 0) and the plain strided gather"""
    worst = 0.0
    for geom, combos in DGRAD:
        B, Hh, W, Ci, Co, k, s, p = geom
        r = conv_refs(geom)
        K = k * k * Co
        E = H.acc_budget(r["dxabs"], K)
        for tile, stages in combos:
            dx = H._nan(B, Hh, W, Ci)
            _dgrad(r, geom, dx, tile=tile, stages=stages)
            worst = max(worst, H.check_bf16(dx.view(-1, Ci), r["dx"], E, "conv dgrad %s tile %d stages %d" % (geom, tile, stages), K))
    print("bf16-err | conv dgrad | largest err/bound %.3g" % worst)


def test_data_gradient_1x1_stride2_parity_classes_without_a_tap():
    """1x1 stride 2 pad 0 in parity tiles: three of the four pixel classes have no live tap, the k-loop is skipped and the epilogue
    must write exact zeros (exactly the residual when one is given)"""
    geom = (2, 16, 16, 64, 128, 1, 2, 0)
    B, Hh, W, Ci, Co, k, s, p = geom
    r = conv_refs(geom)
    K = Co
    E = H.acc_budget(r["dxabs"], K)
    res = H._bf(B * Hh * W, Ci, seed=9)
    ii, jj = torch.meshgrid(torch.arange(Hh), torch.arange(W), indexing="ij")
    empty = ((ii % 2 == 1) | (jj % 2 == 1)).view(1, Hh, W, 1).expand(B, Hh, W, Ci).reshape(-1, Ci)
    assert (r["dxabs"][empty] == 0).all() and (r["dxabs"][~empty] > 0).all()
    for tile, stages in [(2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (3, 4)]:
        for with_res in (False, True):
            dx = H._nan(B, Hh, W, Ci)
            kw = dict(res=res.to(DEV), ldr=Ci) if with_res else {}
            _dgrad(r, geom, dx, tile=tile, stages=stages, **kw)
            ref = r["dx"] + res.double() if with_res else r["dx"]
            Et = E + U * ref.abs() if with_res else E
            what = "conv dgrad 1x1 s2 parity tile %d stages %d res %d" % (tile, stages, with_res)
            H.check_bf16(dx.view(-1, Ci), ref, Et, what, K)
            got = dx.view(-1, Ci).cpu()
            want = res if with_res else torch.zeros_like(res)
            assert torch.equal(H._bits(got)[empty], H._bits(want)[empty]), what + ": a pixel without a tap is not exactly the residual / 0"


@pytest.mark.parametrize("geom,tile", [((1, 8, 8, 64, 64, 3, 1, 1), 2), ((4, 8, 8, 64, 64, 3, 2, 1), 2), ((4, 8, 8, 64, 64, 3, 2, 1), 4),
                                       ((1, 8, 8, 64, 64, 3, 2, 1), 2), ((1, 9, 9, 64, 64, 3, 2, 1), 2)],
                         ids=["lean", "parity", "parity-64x128", "plain", "plain-odd"])
def test_data_gradient_with_residual_and_batchnorm_backward_sums(geom, tile):
    """residual + statistics mode 2 once per gather path (with a last tile's empty wave row at M = 81)"""
    from mmfn_amd import ops16
    B, Hh, W, Ci, Co, k, s, p = geom
    r = conv_refs(geom)
    K, M = k * k * Co, B * Hh * W
    res, y, x = H._bf(M, Ci, seed=11), H._bf(M, Ci, seed=12).clamp(min=0), H._bf(M, Ci, scale=2.0, seed=13)   # y: post-ReLU, half zeros
    mean, rstd = H._f32(Ci, scale=0.1, seed=14), torch.rand(Ci, generator=H._g(15)) + 0.5
    ref = r["dx"] + res.double()
    E = H.acc_budget(r["dxabs"], K) + U * ref.abs()
    for with_y in (True, False):
        rows = H.gemm_stats_rows(ops16.G16_CONV_DGRAD, M, Ci, K, tile)
        stats = H._nan(rows + 2, 2, Ci, dtype=torch.float64)
        dx = H._nan(B, Hh, W, Ci)
        _dgrad(r, geom, dx, tile=tile, stages=3, res=res.to(DEV), ldr=Ci, stats=stats, stats_mode=2,
               bn=(y.to(DEV) if with_y else None, x.to(DEV), mean.to(DEV), rstd.to(DEV)))
        what = "conv dgrad+res+stats2 %s tile %d mask %d" % (geom, tile, with_y)
        H.check_bf16(dx.view(M, Ci), ref, E, what, K)
        H.check_stats(stats, rows, H.stats2_terms(dx.view(M, Ci), y if with_y else None, x, mean, rstd), what)


def test_convolution_weight_gradient_against_fp64():
    """one k-tile of 64 pixels (the lean staging), 16 and 48 pixels (ragged contraction, the per-pixel gather); splitk 0 / 1 / 3,
    ACCUM, every tile whose column tile stays inside one tap (Cin % tile columns == 0) x stages"""
    from mmfn_amd import ops16
    worst = 0.0
    for geom in [(1, 8, 8, 64, 64, 3, 1, 1), (2, 4, 8, 64, 128, 3, 2, 1), (3, 8, 8, 128, 64, 1, 2, 0), (4, 8, 8, 64, 64, 3, 1, 1)]:
        B, Hh, W, Ci, Co, k, s, p = geom
        r = conv_refs(geom)
        Kc = r["y"].shape[0]
        nkt = (Kc + 63) // 64
        c0 = H._f32(Co, k * k * Ci, seed=21)
        x, dy = r["x"].to(DEV), r["dy"].to(DEV)
        tiles = [t for t in (1, 2, 3, 4) if Ci % H.TILE_BN[t] == 0]
        runs = [(t, st, 1, False) for t in tiles for st in (2, 3, 4)]
        runs += [(t, 2 + (t + sk) % 3, sk, acc) for t in tiles for sk in (0, 1, 3) for acc in (False, True)]
        for tile, stages, sk, acc in runs:
            dw = H._nan(Co, k, k, Ci, dtype=torch.float32)
            ref, E = r["dw"], H.acc_budget(r["dwabs"], Kc) + (min(max(sk, 1), nkt) + 1) * U * r["dwabs"]
            if acc:
                dw.view(Co, -1).copy_(c0.to(DEV))
                ref = ref + c0.double()
                E = E + U * ref.abs()
            ops16.conv2d_wgrad(dy, x, (Co, k, k, Ci), s, p, dw, tile=tile, stages=stages, splitk=sk, accum=acc)
            what = "conv wgrad %s tile %d stages %d splitk %d accum %d" % (geom, tile, stages, sk, acc)
            worst = max(worst, H.check_f32(dw.view(Co, -1), ref, E, what))
    print("bf16-err | conv wgrad | largest err/E %.3g" % worst)


# ------------------------------------------------------------------ f. the halo convolution
def _halo_tiles(B, Hh, W, K, N, pro=0):
    from mmfn_amd import ops16
    from mmfn_amd._lib import lib
    return [t for t in (1, 2, 3, 4) if lib().mmfn_conv3x3_halo_bf16_ok(ctypes.byref(ops16._halo_desc(B, Hh, W, K, N, pro, tile=t, stages=2))) == t]


def _conv64(a, w, K):
    """float64 3x3 pad-1 convolution of a [B,H,W,K] (bf16, exact) with w [N,3,3,K], its |.| twin -> ([M,N], budget)"""
    y = _nhwc2d(F.conv2d(_nchw(a), _nchw(w), padding=1))
    S = _nhwc2d(F.conv2d(_nchw(a).abs(), _nchw(w).abs(), padding=1))
    return y, H.acc_budget(S, 9 * K)


HALO = [(1, 8, 8, 64, 64), (3, 8, 8, 64, 64), (2, 4, 8, 64, 64), (4, 4, 8, 64, 128), (1, 8, 32, 64, 64), (1, 32, 8, 64, 64),
        (1, 16, 16, 128, 64), (1, 8, 8, 512, 512)]
HALO_TILES = {(1, 8, 8, 64, 64): [3], (3, 8, 8, 64, 64): [3], (2, 4, 8, 64, 64): [3], (4, 4, 8, 64, 128): [1, 2, 3, 4],
              (1, 8, 32, 64, 64): [1, 3], (1, 32, 8, 64, 64): [1, 3], (1, 16, 16, 128, 64): [1, 3], (1, 8, 8, 512, 512): [3, 4]}


@pytest.mark.parametrize("shape", HALO, ids=lambda s: "x".join(str(v) for v in s))
def test_halo_convolution_against_fp64(shape):
    """pro 0 with statistics mode 0: every tile the library accepts x stages 2..4; the tilings no other test launches (H = 4 with
    two and four images per tile, W = 8 under H > 8, W = 32 at H = 8, one 8x8 image, an odd batch at 8x8)"""
    from mmfn_amd import ops16
    B, Hh, W, K, N = shape
    tiles = _halo_tiles(B, Hh, W, K, N)
    assert tiles == HALO_TILES[shape], "tiles accepted: %s" % tiles
    x, w = H._bf(B, Hh, W, K, seed=31), H._bf(N, 3, 3, K, scale=0.05, seed=32)
    ref, E = _conv64(x, w, K)
    xd, wd = x.to(DEV), w.to(DEV)
    M = B * Hh * W
    for tile in tiles:
        for stages in (2, 3, 4):
            out = H._nan(B, Hh, W, N)
            want_rows = 2 * M // H.TILE_BM[{1: 1, 2: 1, 3: 2, 4: 2}[tile]]
            stats = H._nan(want_rows + 2, 2, N, dtype=torch.float64)
            rows = ops16.conv3x3_halo(xd, wd, out, stats=stats, stats_mode=0, tile=tile, stages=stages)
            assert rows == want_rows
            what = "halo %s tile %d stages %d" % (shape, tile, stages)
            H.check_bf16(out.view(M, N), ref, E, what, 9 * K)
            H.check_stats(stats, rows, ((ref, E), None), what)


def test_halo_odd_batch_refuses_the_two_image_tiles():
    """B = 3 at 8x8: the 128-pixel tiles hold two images, B % 2 != 0 -> tiles 1 and 2 are refused by _ok and by the launch, `out`
    untouched; tile 3 (one image per tile) serves it (test_halo_convolution_against_fp64)"""
    from mmfn_amd import ops16
    from mmfn_amd._lib import MMFNLibraryError
    B, Hh, W, K, N = 3, 8, 8, 64, 64
    assert _halo_tiles(B, Hh, W, K, N) == [3]
    x, w = H._bf(B, Hh, W, K, seed=31).to(DEV), H._bf(N, 3, 3, K, scale=0.05, seed=32).to(DEV)
    for tile in (1, 2):
        out = H._nan(B, Hh, W, N)
        with pytest.raises(MMFNLibraryError, match="code -1"):
            ops16.conv3x3_halo(x, w, out, tile=tile, stages=2)
        torch.cuda.synchronize()
        assert torch.isnan(out).all()


def _bn_apply_model(co, mean, rstd, gamma, beta, res, relu):
    """float64 y = fma(x, alpha, beta') [+ res] [relu] with alpha = w * rstd, beta' = fma(-mean, alpha, b) and the fp32 budget"""
    x = co.double()
    a = gamma.double() * rstd.double()
    Ea = U * a.abs()
    b = beta.double() - mean.double() * a
    Eb = mean.double().abs() * Ea + U * b.abs()
    f = x * a + b
    Ef = x.abs() * Ea + Eb + U * f.abs()
    if res is not None:
        f = f + res.double()
        Ef = Ef + U * f.abs()
    if relu:
        f, Ef = H.relu_model(f, Ef)
    return f, Ef


@pytest.mark.parametrize("shape", HALO[:7], ids=lambda s: "x".join(str(v) for v in s))
def test_halo_batchnorm_apply_in_the_loader_against_fp64(shape):
    """pro 1: a_out against the float64 BatchNorm apply (+ residual, ReLU), `out` against the float64 convolution of the a_out the
    launch wrote (exact in bf16: the tensor the kernel really convolved)"""
    from mmfn_amd import ops16
    B, Hh, W, K, N = shape
    tiles = _halo_tiles(B, Hh, W, K, N, pro=1)
    assert tiles == HALO_TILES[shape]
    co, w = H._bf(B, Hh, W, K, scale=2.0, seed=41), H._bf(N, 3, 3, K, scale=0.05, seed=42)
    res = H._bf(B, Hh, W, K, seed=43)
    mean, rstd = H._f32(K, scale=0.3, seed=44), torch.rand(K, generator=H._g(45)) + 0.5
    gamma, beta = torch.rand(K, generator=H._g(46)) + 0.5, H._f32(K, scale=0.2, seed=47)
    dev = [t.to(DEV) for t in (mean, rstd, gamma, beta)]
    M = B * Hh * W
    n = 0
    for relu, with_res in [(True, False), (True, True), (False, True)]:
        a_ref, a_E = _bn_apply_model(co.view(M, K), mean, rstd, gamma, beta, res.view(M, K) if with_res else None, relu)
        for tile in tiles:
            stages = 2 + n % 3
            n += 1
            a_out, out = H._nan(B, Hh, W, K), H._nan(B, Hh, W, N)
            ops16.conv3x3_halo(co.to(DEV), w.to(DEV), out, bn_apply=(*dev, res.to(DEV) if with_res else None, relu, a_out), tile=tile,
                               stages=stages)
            what = "halo pro 1 %s relu %d res %d tile %d stages %d" % (shape, relu, with_res, tile, stages)
            H.check_bf16(a_out.view(M, K), a_ref, a_E, what + " a_out", 10 ** 9)      # assertion 1 only
            ref, E = _conv64(a_out.cpu(), w, K)
            H.check_bf16(out.view(M, N), ref, E, what, 9 * K)


@pytest.mark.parametrize("shape", [HALO[0], HALO[3], HALO[6]], ids=lambda s: "x".join(str(v) for v in s))
def test_halo_data_gradient_with_skip_gradient_and_batchnorm_backward_sums(shape):
    """flip 1 with out_res and statistics mode 2 (here K = channels of dco, N = channels of dx)"""
    from mmfn_amd import ops16
    B, Hh, W, K, N = shape
    dco, w_t = H._bf(B, Hh, W, K, seed=51), H._bf(N, 3, 3, K, scale=0.05, seed=52)      # w_t: the [Cin,3,3,Cout] shadow
    res, y, x = H._bf(B, Hh, W, N, seed=53), H._bf(B, Hh, W, N, seed=54).clamp(min=0), H._bf(B, Hh, W, N, scale=2.0, seed=55)
    mean, rstd = H._f32(N, scale=0.1, seed=56), torch.rand(N, generator=H._g(57)) + 0.5
    M = B * Hh * W
    # dx[n] = sum over taps of dco[pixel + (1 - kh, 1 - kw)] . w_t[n, kh, kw, :]: a convolution with the taps reversed
    ref, E = _conv64(dco, w_t.flip(1, 2), K)
    ref = ref + res.view(M, N).double()
    E = E + U * ref.abs()
    n = 0
    for tile in _halo_tiles(B, Hh, W, K, N):
        for with_y in (True, False):
            stages = 2 + n % 3
            n += 1
            dx = H._nan(B, Hh, W, N)
            want_rows = 2 * M // (128 if tile in (1, 2) else 64)
            stats = H._nan(want_rows + 2, 2, N, dtype=torch.float64)
            rows = ops16.conv3x3_halo(dco.to(DEV), w_t.to(DEV), dx, flip=True, out_res=res.to(DEV), stats=stats, stats_mode=2,
                                      bn2=(y.to(DEV) if with_y else None, x.to(DEV), mean.to(DEV), rstd.to(DEV)), tile=tile, stages=stages)
            assert rows == want_rows
            what = "halo flip %s tile %d stages %d mask %d" % (shape, tile, stages, with_y)
            H.check_bf16(dx.view(M, N), ref, E, what, 9 * K)
            H.check_stats(stats, rows, H.stats2_terms(dx.view(M, N), y.view(M, N) if with_y else None, x.view(M, N), mean, rstd), what)


# ------------------------------------------------------------------ g. refusals of the halo launch
def test_halo_launch_refusals_leave_the_outputs_untouched():
    """the launch-side twins of what halo_ok refuses, and the descriptors only the launch can see"""
    from mmfn_amd import ops16
    from mmfn_amd._lib import lib, stream
    L = lib()
    big = torch.zeros(1 << 20, dtype=BF, device=DEV)       # operands large enough for every shape below
    f32v = torch.zeros(1024, device=DEV)
    base = dict(B=2, H=8, W=8, K=64, N=64, tile=3, stages=2)
    pro1 = dict(p_mean=f32v, p_rstd=f32v, p_weight=f32v, p_bias=f32v, pro=1)
    table = [
        ("H not a power of two", dict(base, H=6)),
        ("W not a power of two", dict(base, W=12)),
        ("W < 8", dict(base, W=4)),
        ("H < 4", dict(base, H=2)),
        ("K % 64", dict(base, K=32)),
        ("K > 512", dict(base, K=1024)),
        ("N % 64", dict(base, N=32)),
        ("tile 2 with N % 128", dict(base, tile=2)),
        ("tile 4 with N % 128", dict(base, tile=4)),
        ("odd batch, two images per tile", dict(base, B=3, tile=1)),
        ("B = 2 at 4x8 with four images per tile", dict(base, H=4, tile=1)),
        ("B = 0", dict(base, B=0)),
        ("the patch does not fit the LDS", dict(base, H=16, W=16, K=512, N=128, tile=2)),
        ("pro 2", dict(base, pro=2)),
        ("pro 1 without p_mean", dict(base, **dict(pro1, p_mean=None))),
        ("pro 1 without p_bias", dict(base, **dict(pro1, p_bias=None))),
        ("stats mode 1", dict(base, stats=True, stats_mode=1)),
        ("stats mode 2 without bn2_x", dict(base, stats=True, stats_mode=2, bn2_mean=f32v, bn2_rstd=f32v)),
        ("null x", dict(base, x=None)),
        ("null w", dict(base, w=None)),
    ]
    for name, f in table:
        f = dict(f)
        out, a_out = H._nan(1 << 16), H._nan(1 << 16)
        stats = H._nan(64, 2, 128, dtype=torch.float64)
        d = ops16._halo_desc(f.pop("B"), f.pop("H"), f.pop("W"), f.pop("K"), f.pop("N"), f.pop("pro", 0), 0, f.pop("tile"), f.pop("stages"))
        d.x, d.w, d.out, d.a_out = big.data_ptr(), big.data_ptr(), out.data_ptr(), a_out.data_ptr()
        if f.get("stats") is True:
            f["stats"] = stats
        for k, v in f.items():
            setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        assert L.mmfn_conv3x3_halo_bf16_ok(ctypes.byref(d)) == 0 or name.startswith(("pro", "stats", "null")), name + ": _ok accepts it"
        rc = L.mmfn_conv3x3_halo_bf16(ctypes.byref(d), stream())
        torch.cuda.synchronize()
        print("bf16-err | halo refusal %s | code %d" % (name, rc))
        assert rc == H.EINVAL, "%s: returned %d" % (name, rc)
        assert torch.isnan(out).all() and torch.isnan(a_out).all() and torch.isnan(stats).all(), name + ": an output was written"
