"""The VectorNet lane-attention kernels, the radar GAT kernels and the small element-wise / layout kernels against plain torch in
float64 (CPU) on the same fp32 inputs.  Every output buffer is NaN-filled before the call, so "written completely" is part of
each comparison.  Tolerances are the ones test_kernels_gpu.py uses for comparable kernels (relative to max |ref|): 1e-5 forwards,
2e-5 element-wise / row-wise backwards, 5e-5 the attention backward.  Each comparison prints its error (profiles/branch_tests_err.txt)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = "code -1"   # MMFN_EINVAL as ops._call reports it


def _close(got, ref, tol=2e-5, what=""):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    print("branch-err kernel | %s | err/scale %.3g | tol %.3g" % (what, err / scale, tol))
    assert err <= tol * scale, "%s max err %g vs scale %g" % (what, err, scale)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _state():
    return torch.tensor([1234, 7], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------ VectorNet lane attention, query 0
HEADS, HD = 2, 64
D = HEADS * HD


def _lane0_ref(qkv, kv, L, g0):
    """_MaskSelfAttention.forward before to_out in fp64, all L x L interactions; only row 0 of the output receives a gradient."""
    B = kv.numel()
    x = qkv.double().view(B, L, 3 * D).clone().requires_grad_(True)
    q, k, v = (t.reshape(B, L, HEADS, HD).transpose(1, 2) for t in x.chunk(3, dim=-1))
    mask = (torch.arange(L)[None, :] < kv[:, None].long()).double()[:, None, :]
    dots = (q @ k.transpose(-1, -2)) * HD ** -0.5
    dots = dots.masked_fill(mask.unsqueeze(1) == 0, -1e9)
    prob = torch.softmax(dots, dim=-1)
    out = (prob @ v).transpose(1, 2).reshape(B, L, D)
    out[:, 0, :].backward(g0.double())
    return out[:, 0, :].detach(), prob[:, :, 0, :].detach(), x.grad.view(B * L, 3 * D)


def _lane0_run(qkv, kv, L, g0, what, tol_f=1e-5, tol_b=5e-5):
    from mmfn_amd import ops
    B = g0.shape[0]
    att_ref, prob_ref, dqkv_ref = _lane0_ref(qkv, kv if kv is not None else torch.full((B,), L), L, g0)
    qd, gd = qkv.to(DEV), g0.to(DEV)
    kvd = None if kv is None else kv.to(device=DEV, dtype=torch.int32)
    att0, prob = _nan(B, D), _nan(B, HEADS, L)
    ops.lane0_attention_fwd(qd, kvd, B, L, HEADS, HD, HD ** -0.5, att0, prob)
    dqkv = _nan(B * L, 3 * D)
    ops.lane0_attention_bwd(qd, prob, gd, kvd, B, L, HEADS, HD, HD ** -0.5, dqkv)
    torch.cuda.synchronize()
    _close(att0, att_ref, tol_f, what + " att0")
    _close(prob, prob_ref, tol_f, what + " prob")
    _close(dqkv, dqkv_ref, tol_b, what + " dqkv")
    assert torch.isfinite(att0).all() and torch.isfinite(prob).all() and torch.isfinite(dqkv).all()
    return att0, prob, dqkv.view(B, L, 3 * D)


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 130, 300])
@pytest.mark.parametrize("kvset", [0, 1])
def test_lane0_attention_against_fp64(L, kvset):
    """1, 2, 3 and 5 passes of the 64-key wave loop, with and without a ragged tail; per-sample key counts 0, 1, L-1 / L, L+5, -1."""
    B = 3
    g = _g(100 * L + kvset)
    qkv = torch.randn(B * L, 3 * D, generator=g)
    g0 = torch.randn(B, D, generator=g)
    kv = torch.tensor([0, 1, L - 1] if kvset == 0 else [L, L + 5, -1])
    att0, prob, dqkv = _lane0_run(qkv, kv, L, g0, "lane0 L=%d kv=%s" % (L, kv.tolist()))
    # each probability is a few ulp off and they are summed over <= 300 keys: the forward tolerance covers it
    assert (prob.double().sum(-1) - 1.0).abs().max().item() <= 1e-5
    for b in range(B):
        n = min(L, int(kv[b]))
        dq, dk, dv = dqkv[b, :, :D], dqkv[b, :, D:2 * D], dqkv[b, :, 2 * D:]
        assert (dq[1:] == 0).all(), "dead query rows"
        if n <= 0:   # no keys: uniform attention (to the last bit or two of 1/L), constant scores pass no gradient to q and k
            assert (prob[b].double() - 1.0 / L).abs().max().item() <= 2.0 ** -22 / L
            assert (dq == 0).all() and (dk == 0).all()
            _close(dv, (g0[b].double() / L).expand(L, D), 1e-6, "lane0 L=%d no keys dv = g / L" % L)
        else:
            assert (prob[b, :, n:] == 0).all(), "masked keys"
            assert (dk[n:] == 0).all() and (dv[n:] == 0).all(), "masked keys' gradients"


def test_lane0_attention_without_kv_len_equals_all_keys():
    from mmfn_amd import ops
    B, L = 3, 65
    g = _g(7)
    qkv = torch.randn(B * L, 3 * D, generator=g).to(DEV)
    g0 = torch.randn(B, D, generator=g).to(DEV)
    full = torch.full((B,), L, dtype=torch.int32, device=DEV)
    outs = []
    for kv in (None, full):
        att0, prob, dqkv = _nan(B, D), _nan(B, HEADS, L), _nan(B * L, 3 * D)
        ops.lane0_attention_fwd(qkv, kv, B, L, HEADS, HD, HD ** -0.5, att0, prob)
        ops.lane0_attention_bwd(qkv, prob, g0, kv, B, L, HEADS, HD, HD ** -0.5, dqkv)
        outs.append((att0, prob, dqkv))
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    _lane0_run(qkv.cpu(), None, L, g0.cpu(), "lane0 L=65 kv_len=None")


def test_lane0_attention_large_logits():
    """q and k scaled so that the scores have magnitude ~60 (the largest well above 100): exp() of an unshifted score overflows
    fp32, so this passes only with the row maximum subtracted."""
    B, L = 3, 130
    g = _g(11)
    qkv = torch.randn(B * L, 3 * D, generator=g)
    qkv[:, :2 * D] *= 60.0 ** 0.5   # q.k / 8 has standard deviation 60
    g0 = torch.randn(B, D, generator=g)
    kv = torch.tensor([130, 100, 65])
    x = qkv.view(B, L, 3 * D)
    scores = (x[:, :1, :HD] * x[:, :, D:D + HD]).sum(-1) / 8.0   # head 0, query 0
    assert scores.abs().max().item() > 100.0
    _lane0_run(qkv, kv, L, g0, "lane0 large logits")


def test_lane0_attention_refusals():
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    B, L = 2, 4
    qkv, g0 = torch.zeros(B * L, 3 * D, device=DEV), torch.zeros(B, D, device=DEV)
    att0, prob, dqkv = _nan(B, D), _nan(B, HEADS, L), _nan(B * L, 3 * D)
    for hd, l in ((32, L), (HD, 0)):
        with pytest.raises(MMFNLibraryError, match=EINVAL):
            ops.lane0_attention_fwd(qkv, None, B, l, HEADS, hd, 0.125, att0, prob)
        with pytest.raises(MMFNLibraryError, match=EINVAL):
            ops.lane0_attention_bwd(qkv, prob, g0, None, B, l, HEADS, hd, 0.125, dqkv)
    torch.cuda.synchronize()
    assert torch.isnan(att0).all() and torch.isnan(dqkv).all()   # a refused call launches nothing


# ------------------------------------------------------------------ radar GAT softmax
ALPHA = 0.2


def _gat_inputs(R, N):
    g = _g(R * 1000 + N)
    e = torch.randn(R, N, generator=g) * 3.0
    u = torch.rand(R, N, generator=g)
    e[u < 0.03] = 80.0
    e[u > 0.97] = -80.0
    adj = torch.randint(0, 2, (R, N), generator=g).float()
    u = torch.rand(R, N, generator=g)
    adj[u < 0.1] = -1.5    # negative and -0.0 entries count as masked, like 0
    adj[u > 0.9] = -0.0
    adj[2::3] = 0.0        # rows without a neighbour: uniform attention, as the reference's -9e15 fill gives
    if R > 4:
        adj[4] = -0.0
    gy = torch.randn(R, N, generator=g)
    return e, adj, gy


def _gat_ref(e, adj, gy, mask=None):
    e64 = e.double().clone().requires_grad_(True)
    a64 = adj.double()
    le = F.leaky_relu(e64, ALPHA)
    p = torch.softmax(torch.where(a64 > 0, le, torch.full_like(le, -9e15)), dim=-1)
    att = p if mask is None else p * mask.double()
    att.backward(gy.double())
    return p.detach(), att.detach(), e64.grad


@pytest.mark.parametrize("R,N", [(1, 1), (5, 63), (7, 64), (6, 65), (243, 81), (9, 128)])
def test_gat_softmax_against_fp64(R, N):
    from mmfn_amd import ops
    e, adj, gy = _gat_inputs(R, N)
    ed, ad, gd = e.to(DEV), adj.to(DEV), gy.to(DEV)
    masked = ~(adj > 0)
    what = "gat R=%d N=%d" % (R, N)
    # dropout off
    p_ref, att_ref, ge_ref = _gat_ref(e, adj, gy)
    p, att, ge = _nan(R, N), _nan(R, N), _nan(R, N)
    ops.gat_softmax_fwd(ed, ad, ALPHA, p, att)
    ops.gat_softmax_bwd(gd, p, ed, ad, ALPHA, ge)
    assert torch.isfinite(p).all() and torch.equal(p, att)
    _close(p, p_ref, 1e-5, what + " p")
    _close(ge, ge_ref, 2e-5, what + " g_epre")
    assert (ge.cpu()[masked] == 0).all(), "masked entries pass no gradient"
    # dropout 0.1: the kept entries are those of dropout_apply over the same flat index row * N + col
    state, sid = _state(), 901
    p2, att2, ge2 = _nan(R, N), _nan(R, N), _nan(R, N)
    ops.gat_softmax_fwd(ed, ad, ALPHA, p2, att2, 0.1, state, sid)
    assert torch.equal(p2, p)
    assert torch.equal(att2.view(-1), ops.dropout_apply(p2.view(-1), _nan(R * N), 0.1, state, sid))
    mask = ops.dropout_apply(torch.ones(R * N, device=DEV), _nan(R * N), 0.1, state, sid).view(R, N).cpu()
    assert set(mask.unique().tolist()) <= {0.0, (1.0 / (1.0 - torch.tensor(0.1))).item()}
    _, att_ref2, ge_ref2 = _gat_ref(e, adj, gy, mask)
    ops.gat_softmax_bwd(gd, p2, ed, ad, ALPHA, ge2, 0.1, state, sid)
    _close(att2, att_ref2, 1e-5, what + " att dropout 0.1")
    _close(ge2, ge_ref2, 2e-5, what + " g_epre dropout 0.1")
    assert (ge2.cpu()[masked] == 0).all()
    if R * N >= 64:
        assert (mask == 0).any() and (mask > 0).any()
        att3 = _nan(R, N)
        ops.gat_softmax_fwd(ed, ad, ALPHA, _nan(R, N), att3, 0.1, state, sid + 1)
        assert torch.isfinite(att3).all() and not torch.equal(att3, att2), "another stream id, another mask"


def test_gat_softmax_refuses_rows_longer_than_two_columns_per_lane():
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    R, N = 4, 129
    e, adj, out = torch.zeros(R, N, device=DEV), torch.ones(R, N, device=DEV), _nan(R, N)
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops.gat_softmax_fwd(e, adj, ALPHA, out, out)
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops.gat_softmax_bwd(e, e, e, adj, ALPHA, out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------ log-softmax with the (8, 8) swap
@pytest.mark.parametrize("R,C,swap", [(64, 512, 1), (192, 512, 1), (128, 64, 1), (3, 128, 0), (70, 320, 0)])
def test_log_softmax_against_fp64(R, C, swap):
    from mmfn_amd import ops
    g = _g(R * 7 + C + swap)
    x = torch.randn(R, C, generator=g) + (torch.rand(R, 1, generator=g) * 200.0 - 100.0)   # per-row offsets up to +-100
    x[1] = 3.25                                                                           # one row of equal values
    gy = torch.randn(R, C, generator=g)       # gradient in the OUTPUT's layout, as the engine passes it
    x64 = x.double().clone().requires_grad_(True)
    if swap:   # _SpGAT.forward's last two lines; the kernel's output is that result in NHWC
        B = R // 64
        y64 = F.log_softmax(x64.reshape(B, 8, 8, C).transpose(1, 3), dim=1).permute(0, 2, 3, 1).reshape(R, C)
    else:
        y64 = F.log_softmax(x64, dim=-1)
    y64.backward(gy.double())
    xd, gd = x.to(DEV), gy.to(DEV)
    y, dx = _nan(R, C), _nan(R, C)
    ops.log_softmax_fwd(xd, y, R, C, swap)
    ops.log_softmax_bwd(gd, y, dx, R, C, swap)
    what = "log_softmax R=%d C=%d swap=%d" % (R, C, swap)
    _close(y, y64, 1e-5, what + " fwd")
    _close(dx, x64.grad, 2e-5, what + " bwd")
    # y = x - lse with both near |x|max: a few ulp at that magnitude is the error of y, hence the relative error of exp(y)
    bound = 4 * 2.0 ** -23 * (x.abs().max().item() + 10.0)
    dev = (y.double().exp().sum(-1) - 1.0).abs().max().item()
    print("branch-err kernel | %s sum exp(y) - 1 | err %.3g | tol %.3g" % (what, dev, bound))
    assert dev <= bound


def test_log_softmax_refusals():
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    x, out = torch.zeros(70 * 576, device=DEV), _nan(70 * 576)
    for R, C, swap in ((64, 96, 0), (64, 576, 0), (70, 64, 1)):
        with pytest.raises(MMFNLibraryError, match=EINVAL):
            ops.log_softmax_fwd(x, out, R, C, swap)
        with pytest.raises(MMFNLibraryError, match=EINVAL):
            ops.log_softmax_bwd(x, x, out, R, C, swap)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------ ELU, relu_mask, axpby, dropout_apply
SIZES = [1, 255, 256 * 4096 + 3]   # the last: one element past a full grid of the largest launch, so the grid-stride loop runs
SPECIALS = [-1e-7, 0.0, -0.0, 1e-7, -20.0, -100.0, 50.0]


def _values(n, seed):
    g = _g(seed)
    x = torch.randn(n, generator=g) * 3.0
    k = min(n, len(SPECIALS))
    x[:k] = torch.tensor(SPECIALS[:k])
    if n > 2 * len(SPECIALS):
        x[-len(SPECIALS):] = torch.tensor(SPECIALS)   # ... and in the tail the second trip of the loop handles
    return x, torch.randn(n, generator=g)


@pytest.mark.parametrize("n", SIZES)
def test_elu_against_fp64(n):
    from mmfn_amd import ops
    x, gy = _values(n, n)
    x64 = x.double().clone().requires_grad_(True)
    F.elu(x64).backward(gy.double())
    ref = torch.where(x.double() > 0, x.double(), torch.expm1(x.double()))
    xd, gd = x.to(DEV), gy.to(DEV)
    y, dx = _nan(n), _nan(n)
    ops.elu_fwd(xd, y)
    ops.elu_bwd(gd, y, dx)
    _close(y, ref, 1e-5, "elu fwd n=%d" % n)
    # element-wise RELATIVE error: expm1 keeps it at an ulp or two for tiny negative inputs, exp(x) - 1 loses every digit there
    nz = ref != 0
    rel = ((y.cpu().double() - ref)[nz] / ref[nz]).abs().max().item() if nz.any() else 0.0
    print("branch-err kernel | elu fwd n=%d element-wise relative | err %.3g | tol 1e-06" % (n, rel))
    assert rel <= 1e-6
    assert (y.cpu()[ref == 0] == 0).all()
    _close(dx, x64.grad, 2e-5, "elu bwd n=%d" % n)
    at0 = x == 0
    assert torch.equal(dx.cpu()[at0], gy[at0]), "the slope exactly at 0 is 1"


@pytest.mark.parametrize("n", SIZES)
def test_relu_mask_in_place_and_out_of_place(n):
    from mmfn_amd import ops
    y, gy = _values(n, n + 1)
    if n > 2:
        y[2] = float("nan")
        y[-1] = float("nan")
    else:
        y[0] = float("nan")
    for special in (0.0, -0.0, float("nan")):
        yy = y.clone()
        yy[0] = special
        yd, gd = yy.to(DEV), gy.to(DEV)
        want = torch.where(yy > 0, gy, torch.zeros_like(gy))
        out = ops.relu_mask(gd, yd, _nan(n))
        assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)), "bit for bit, +0.0 where y is not > 0"
        assert out[0].item() == 0.0
        g2 = gd.clone()
        assert ops.relu_mask(g2, yd) is g2 and torch.equal(g2, out), "in place"
        assert torch.equal(gd.cpu(), gy), "the out-of-place call leaves g alone"


@pytest.mark.parametrize("n", SIZES)
def test_axpby(n):
    from mmfn_amd import ops
    x, y0 = _values(n, n + 2)
    xd = x.to(DEV)
    y = ops.axpby(_nan(n), xd, 1.7, 0.0)
    assert torch.equal(y.cpu(), x * 1.7), "b = 0 ignores what y held, NaN included"
    y = ops.axpby(y0.to(DEV), xd, 1.0, 1.0)
    assert torch.equal(y.cpu(), x + y0), "(1, 1) accumulates"
    y = ops.axpby(y0.to(DEV), xd, 0.5, 2.0)
    _close(y, 0.5 * x.double() + 2.0 * y0.double(), 1e-5, "axpby (0.5, 2) n=%d" % n)


@pytest.mark.parametrize("n", SIZES)
def test_dropout_apply_in_place_equals_out_of_place(n):
    from mmfn_amd import ops
    from mmfn_amd._lib import MMFNLibraryError
    x, _ = _values(n, n + 3)
    xd, state = x.to(DEV), _state()
    out = ops.dropout_apply(xd, _nan(n), 0.1, state, 905)
    inplace = xd.clone()
    ops.dropout_apply(inplace, inplace, 0.1, state, 905)
    assert torch.isfinite(out).all() and torch.equal(out.view(torch.int32), inplace.view(torch.int32))
    keep = 1.0 / (1.0 - torch.tensor(0.1))
    kept = out.cpu() != 0
    assert torch.equal(out.cpu()[kept], (x * keep)[kept])
    if n > 1000:   # Bernoulli(0.9) over a million draws: sigma = 3e-4
        rate = (kept | (x == 0)).float().mean().item()
        assert abs(rate - 0.9) <= 2e-3, rate
    assert torch.equal(ops.dropout_apply(xd, _nan(n), 0.0, state, 905).view(torch.int32), xd.view(torch.int32)), "p = 0 is the identity"
    refused = _nan(n)
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops.dropout_apply(xd, refused, 1.0, state, 905)
    with pytest.raises(MMFNLibraryError, match=EINVAL):
        ops.dropout_apply(xd, refused, 0.1, None, 905)
    torch.cuda.synchronize()
    assert torch.isnan(refused).all()


# ------------------------------------------------------------------ repitch_rows, conv_weight_flip, bn_fold
@pytest.mark.parametrize("R,K,ps,pd", [(64, 147, 147, 160), (64, 98, 128, 98)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_repitch_rows(R, K, ps, pd, dtype):
    from mmfn_amd import ops
    src = torch.randn(R, ps, generator=_g(K + pd))
    want = F.pad(src[:, :K], (0, pd - K)).to(dtype)
    dst = ops.repitch_rows(src.to(DEV), _nan(R, pd, dtype=dtype), R, K, ps, pd)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(dst.cpu().view(bits), want.view(bits))
    assert (dst[:, K:] == 0).all(), "pad columns"


@pytest.mark.parametrize("Co,T,Ci", [(64, 9, 64), (33, 9, 70), (5, 49, 3)])
def test_conv_weight_flip(Co, T, Ci):
    """w[Co][T][Ci] -> wt[Ci][T][Co] with the taps reversed: full 32x32 tiles and ragged ones on both sides."""
    from mmfn_amd import ops
    w = torch.randn(Co, T, Ci, generator=_g(Co + T + Ci))
    wd, wt = w.to(DEV), _nan(Ci, T, Co)
    ops._call("mmfn_conv_weight_flip_f32", ops.ptr(wd), ops.ptr(wt), Co, T, Ci, ops.stream())
    assert torch.equal(wt.cpu(), w.flip(1).permute(2, 1, 0).contiguous())


@pytest.mark.parametrize("Cout,taps,Cin", [(70, 9, 3), (64, 9, 64)])
def test_bn_fold_against_fp64(Cout, taps, Cin):
    from mmfn_amd import ops
    g = _g(Cout + Cin)
    K = taps * Cin   # 27 and 576
    w = torch.randn(Cout, 3, 3, Cin, generator=g)
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    rm, rv = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.5
    rv[3] = 1e-8   # a channel that never varied: eps carries the scale
    eps = 1e-5
    s = gamma.double() / torch.sqrt(rv.double() + eps)
    w_out, b_out = _nan(Cout, 3, 3, Cin), _nan(Cout)
    ops.bn_fold(*(t.to(DEV) for t in (w, gamma, beta, rm, rv)), eps, w_out, b_out)
    # per output channel (their scales differ by 300x): w_out / s against w
    _close(w_out.cpu().double().view(Cout, K) / s[:, None], w.view(Cout, K), 1e-5, "bn_fold w Cout=%d K=%d" % (Cout, K))
    _close(w_out, w.double() * s[:, None, None, None], 1e-5, "bn_fold w (whole) Cout=%d K=%d" % (Cout, K))
    b_ref = beta.double() - rm.double() * s
    rel = ((b_out.cpu().double() - b_ref).abs() / (beta.double().abs() + (rm.double() * s).abs())).max().item()
    print("branch-err kernel | bn_fold b Cout=%d K=%d | err/scale %.3g | tol 1e-05" % (Cout, K, rel))
    assert rel <= 1e-5
