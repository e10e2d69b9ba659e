"""mmfn_gemm_bf16 (csrc/gemm_bf16.hip), the Linear forms, against float64 on the CPU with an error budget derived from the
arithmetic instead of one max-norm tolerance.

Reference: the bf16 inputs are generated on the CPU and widened to float64 (exact), pre = A64 @ B64^T, S = |A64| @ |B64|^T, and
the epilogue is replayed in float64 in the kernel's order (stats0, bias, relu, gelu, mask, dropout, residual, stats1/2, accum,
relu_last, store).  Budget per element: E = 8 sqrt(K) 2^-24 S_ij for the K fp32 additions of the accumulation (Higham-Mary,
lambda = 8), carried through the epilogue (every step 1-Lipschitz except the dropout scale and GELU, 1.13; ReLU as the interval
[relu(v - E), relu(v + E)], so a value clamped with certainty is exactly 0) plus 2^-24 |value| per fp32 operation.  GELU's own
term is measured on the reference side (CPU fp32 F.gelu against float64, four times its largest error in units of
2^-24 (|x| + 1)).
  fp32 outputs: |got - ref| <= E for every element.
  bf16 outputs: (1) |got - ref| <= E + 2^-8 (|ref| + E) for every element; (2) where bf16_rne(ref - E) and bf16_rne(ref + E)
  are the same bit pattern, got must be that pattern (signed zeros compare equal); cases with K <= 576 only, and there at least
  75 % of the elements must be unambiguous.
  Statistics by-products: partial rows summed in float64, per column; |sum - ref| <= sum E + 64 * 2^-24 sum |term| for plain sums,
  sum 2 |v| E + 66 * 2^-24 sum v^2 for squares.
Every output buffer and every padding column is NaN-filled before the call.  Each comparison prints one `bf16-err` line
(profiles/bf16_gemm_tests_err.txt).  tile / stages / splitk are always explicit: no case depends on the tuning table."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
U = 2.0 ** -24
NAN = float("nan")
EINVAL = -1
TILE_BM = {1: 128, 2: 64, 3: 128, 4: 64}
TILE_BN = {1: 128, 2: 64, 3: 64, 4: 128}


# ------------------------------------------------------------------ shared helper (test_conv16_fp64_gpu.py imports it)
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(*shape, scale=1.0, seed=0):
    """bf16 tensor generated on the CPU"""
    return (torch.randn(*shape, generator=_g(seed)) * scale).to(BF)


def _f32(*shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=_g(seed)) * scale


def _nan(*shape, dtype=BF):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _padded(t, ld):
    """t [R, C] on the device inside a NaN-filled [R, ld] buffer: (buffer, view of the first C columns)"""
    buf = _nan(t.shape[0], ld, dtype=t.dtype)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, buf[:, :t.shape[1]]


def _bits(t):
    """bit pattern of a bf16 tensor with -0 folded onto +0"""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b == 0x8000, torch.zeros_like(b), b)


def bf16_rne(x):
    """float64 -> bf16, round to nearest even in ONE rounding (no detour through fp32): the value is scaled by a power of two so
    that one bf16 ulp becomes 1.0 (exact), rounded half-to-even to an integer and scaled back (exact).  Normal range only; values
    below 2^-126 are rounded on the subnormal grid."""
    _, ex = torch.frexp(x)                                  # |x| = m * 2^ex, m in [0.5, 1)
    ex = ex.clamp(min=-125).double()
    ulp = torch.pow(2.0, ex - 8.0)
    return (torch.round(x / ulp) * ulp).to(BF)              # representable: the cast is exact


def _worst(err, bound):
    """largest err / bound over the elements with a non-zero bound (where the bound is an exact 0 the assertion wants err == 0)"""
    nz = bound > 0
    return (err[nz] / bound[nz]).max().item() if nz.any() else 0.0


def check_f32(got, ref, E, what):
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err = (got - ref).abs()
    ratio = _worst(err, E)
    print("bf16-err | %s | fp32 out | err/E %.3g | n %d" % (what, ratio, got.numel()))
    bad = err > E
    assert not bad.any(), "%s: %d elements beyond the budget (%d of them where the budget is an exact 0), worst err/E %.3g" % (
        what, int(bad.sum()), int((bad & (E == 0)).sum()), ratio)
    return ratio


def check_bf16(got, ref, E, what, K):
    """the two bf16 assertions of the module docstring; K decides whether the bit-pattern assertion applies"""
    assert got.dtype == BF
    got = got.detach().cpu()
    g64 = got.double()
    assert torch.isfinite(g64).all(), what + ": non-finite output"
    err = (g64 - ref).abs()
    bound = E + 2.0 ** -8 * (ref.abs() + E)
    r1 = _worst(err, bound)
    bad = err > bound
    share = float("nan")
    msg = ""
    if K <= 576:
        lo, hi = _bits(bf16_rne(ref - E)), _bits(bf16_rne(ref + E))
        unamb = lo == hi
        share = unamb.double().mean().item()
        wrong = unamb & (_bits(got) != lo)
        msg = " | wrong bits %d" % int(wrong.sum())
    print("bf16-err | %s | bf16 out | err/bound %.3g | unambiguous %.1f%%%s" % (what, r1, 100 * share, msg))
    assert not bad.any(), "%s: %d elements beyond E + half an ulp (%d of them where the bound is an exact 0), worst err/bound %.3g" % (
        what, int(bad.sum()), int((bad & (bound == 0)).sum()), r1)
    if K <= 576:
        assert share >= 0.75, "%s: only %.1f%% of the elements are unambiguous" % (what, 100 * share)
        assert not wrong.any(), "%s: %d of %d unambiguous elements are not the correctly rounded bf16" % (
            what, int(wrong.sum()), int(unamb.sum()))
    return r1


def check_out(got, ref, E, what, K):
    return check_f32(got, ref, E, what) if got.dtype == torch.float32 else check_bf16(got, ref, E, what, K)


def acc_budget(S, K):
    return 8.0 * math.sqrt(K) * U * S


_gelu_term = {}


def gelu_model(v, E, what):
    """float64 GELU of the modelled value and its budget: 1.13-Lipschitz, plus four times the largest error of torch's CPU fp32
    F.gelu on the same pre-activations in units of 2^-24 (|x| + 1) (erff's device accuracy is not documented)."""
    x32 = v.float()
    e32 = (F.gelu(x32).double() - F.gelu(x32.double())).abs() / (U * (x32.double().abs() + 1.0))
    term = e32.max().item()
    _gelu_term[what] = term
    print("bf16-err | %s | GELU term: CPU fp32 F.gelu is off by at most %.3g * 2^-24 (|x| + 1); allowed 4x" % (what, term))
    return F.gelu(v), 1.13 * E + 4.0 * term * U * (v.abs() + 1.0)


def drop_scale(p):
    """the kernels' 1.0f / (1.0f - p) in float32, widened"""
    one = torch.tensor(1.0, dtype=torch.float32)
    return float((one / (one - torch.tensor(p, dtype=torch.float32))).double())


_keep = {}


def keep_mask(M, N, p, rng, stream_id):
    """keep-mask [M, N] of (state, stream) from the fp32 path's mmfn_dropout_apply_f32 on ones (index = row * N + col)"""
    from mmfn_amd import ops
    key = (M, N, p, tuple(rng.tolist()), stream_id)
    if key not in _keep:
        ones = torch.ones(M, N, device=DEV)
        _keep[key] = (ops.dropout_apply(ones, torch.empty_like(ones), p, rng.to(DEV), stream_id) > 0).cpu()
    return _keep[key]


def relu_model(v, E):
    """ReLU is monotone: a value inside [v - E, v + E] lands inside [relu(v - E), relu(v + E)] - exactly 0 once v + E <= 0"""
    r = v.clamp(min=0.0)
    return r, torch.maximum((v + E).clamp(min=0.0) - r, r - (v - E).clamp(min=0.0))


def epilogue_model(pre, E, bias=None, relu=False, gelu=False, aux=None, keep=None, p=0.0, res=None, c0=None, relu_last=False,
                   what=""):
    """(final value, budget, value before accum / relu_last, its budget) in float64; operands already widened"""
    v = pre
    if bias is not None:
        v = v + bias
        E = E + U * v.abs()
    if relu:
        v, E = relu_model(v, E)
    if gelu:
        v, E = gelu_model(v, E, what)
    if aux is not None:
        v = torch.where(aux > 0, v, torch.zeros_like(v))
        E = torch.where(aux > 0, E, torch.zeros_like(E))
    if keep is not None:
        sc = keep.double() * drop_scale(p)
        v = v * sc
        E = E * sc + U * v.abs()
    if res is not None:
        v = v + res
        E = E + U * v.abs()
    v1, E1 = v, E
    if c0 is not None:
        v = v + c0
        E = E + U * v.abs()
    if relu_last:
        v, E = relu_model(v, E)
    return v, E, v1, E1


def check_stats(stats, rows, ref_terms, what):
    """stats [rows + extra, 2, N] (NaN-filled before the launch); ref_terms = ((terms1, E1), (terms2, E2) or None) with
    terms [M, N]: the first sum's terms with their per-element budget, the second sum's (None: the squares of the first)."""
    st = stats.detach().cpu()
    assert rows > 0 and torch.isfinite(st[:rows]).all(), what + ": a partial row inside the count is not finite"
    assert torch.isnan(st[rows:]).all(), what + ": a partial row beyond the count was written"
    got = st[:rows].sum(0)
    (t1, e1), second = ref_terms
    b1 = e1.sum(0) + 64 * U * t1.abs().sum(0)
    if second is None:
        t2 = t1 * t1
        b2 = (2 * t1.abs() * e1).sum(0) + 66 * U * t2.sum(0)
    else:
        t2, e2 = second
        b2 = e2.sum(0) + 64 * U * t2.abs().sum(0)
    r1 = ((got[0] - t1.sum(0)).abs() / (b1 + 1e-300)).max().item()
    r2 = ((got[1] - t2.sum(0)).abs() / (b2 + 1e-300)).max().item()
    print("bf16-err | %s | stats rows %d | sum err/bound %.3g | second sum err/bound %.3g" % (what, rows, r1, r2))
    assert ((got[0] - t1.sum(0)).abs() <= b1).all(), "%s first sum: err/bound %.3g" % (what, r1)
    assert ((got[1] - t2.sum(0)).abs() <= b2).all(), "%s second sum: err/bound %.3g" % (what, r2)
    return max(r1, r2)


def stats2_terms(out, bn_y, bn_x, mean, rstd):
    """mode 2 from the launch's own STORED bf16 output: ge = out masked by bn_y > 0, (sum ge, sum ge * xhat), xhat from the fp32
    mean / rstd widened.  ge is exact; the product carries three fp32 roundings."""
    ge = out.detach().cpu().double()
    if bn_y is not None:
        ge = torch.where(bn_y.double() > 0, ge, torch.zeros_like(ge))
    t2 = ge * ((bn_x.double() - mean.double()) * rstd.double())
    return (ge, torch.zeros_like(ge)), (t2, 3 * U * t2.abs())


def gemm_stats_rows(form, M, N, K, tile):
    from mmfn_amd import ops16
    return ops16.stats_rows(M, N, K, form, tile)


# ------------------------------------------------------------------ a. NT pipeline
def _nt_inputs(M, N, K, seed):
    A, B = _bf(M, K, seed=seed), _bf(N, K, scale=0.1, seed=seed + 1)
    A64, B64 = A.double(), B.double()
    return A, B, A64 @ B64.t(), A64.abs() @ B64.abs().t()


def test_nt_pipeline_tiles_and_stages():
    """form 0, fp32 out, no epilogue: tiles 1..4 x stages 2, 3, 4 at one k-tile (prologue only), three (the NS boundaries), five
    (NS = 4 wraps; N > 256, N % 128 != 0, a 2-row last tile); K = 576 once; one pass with padded lda / ldb / ldc."""
    from mmfn_amd import ops16
    worst = 0.0
    for (M, N, K) in [(72, 72, 64), (200, 136, 192), (130, 264, 320), (64, 64, 576)]:
        A, B, pre, S = _nt_inputs(M, N, K, seed=M + K)
        E = acc_budget(S, K)
        Ad, Bd = A.to(DEV), B.to(DEV)
        combos = [(t, s) for t in (1, 2, 3, 4) for s in (2, 3, 4)] if K != 576 else [(2, 4)]
        for tile, stages in combos:
            C = _nan(M, N, dtype=torch.float32)
            ops16.gemm16(ops16.G16_NT, Ad, Bd, C, M, N, K, K, K, N, tile=tile, stages=stages)
            worst = max(worst, check_f32(C, pre, E, "NT (%d,%d,%d) tile %d stages %d" % (M, N, K, tile, stages)))
        # leading dimensions that differ from the packed ones
        (Ab, Av), (Bb, Bv) = _padded(A, K + 8), _padded(B, K + 16)
        for tile, stages in [(1, 3), (2, 2), (4, 4)]:
            Cb = _nan(M, N + 8, dtype=torch.float32)
            ops16.gemm16(ops16.G16_NT, Av, Bv, Cb, M, N, K, K + 8, K + 16, N + 8, tile=tile, stages=stages)
            check_f32(Cb[:, :N], pre, E, "NT (%d,%d,%d) tile %d stages %d lda K+8 ldb K+16 ldc N+8" % (M, N, K, tile, stages))
            assert torch.isnan(Cb[:, N:]).all(), "padding columns of C were written"
    print("bf16-err | NT pipeline | largest err/E %.3g" % worst)


# ------------------------------------------------------------------ b. epilogue order
EPI_M, EPI_N, EPI_K = 136, 72, 128
# name -> flags.  res: "bf16" / "bf16pad" / "f32"; aux: "packed" / "pad"
EPI_CASES = [
    ("none", {}),
    ("bias", dict(bias=1)),
    ("relu", dict(relu=1)),
    ("gelu", dict(gelu=1)),
    ("mask", dict(aux="packed")),
    ("dropout 0.1", dict(p=0.1)),
    ("residual", dict(res="bf16")),
    ("residual f32", dict(res="f32")),
    ("accum", dict(accum=1)),
    ("relu_last", dict(relu_last=1)),
    ("bias+relu", dict(bias=1, relu=1)),
    ("bias+gelu", dict(bias=1, gelu=1)),
    ("mask, padded ldaux", dict(aux="pad")),
    ("bias+dropout 0.1+residual, padded ldr", dict(bias=1, p=0.1, res="bf16pad")),
    ("bias+dropout 0.25+residual, padded ldr", dict(bias=1, p=0.25, res="bf16pad")),
    ("bias+dropout 0.1+residual f32", dict(bias=1, p=0.1, res="f32")),
    ("bias+residual+relu_last", dict(bias=1, res="bf16", relu_last=1)),
    ("accum+relu_last", dict(accum=1, relu_last=1)),
    ("bias+relu+mask+dropout 0.25+residual+accum+relu_last", dict(bias=1, relu=1, aux="pad", p=0.25, res="bf16pad", accum=1, relu_last=1)),
]
RNG = torch.tensor([1234, 7], dtype=torch.int64)
STREAM = 11


def _epi_operands(M, N, spec, out_dtype, seed=50):
    """(kwargs of ops16.gemm16, kwargs of epilogue_model, C buffer, ldc) for one case"""
    kw, mk = {}, {}
    if spec.get("bias"):
        b = _f32(N, seed=seed + 1)
        kw["bias"], mk["bias"] = b.to(DEV), b.double()
    kw["relu"] = mk["relu"] = bool(spec.get("relu"))
    kw["gelu"] = mk["gelu"] = bool(spec.get("gelu"))
    if spec.get("aux"):
        a = _bf(M, N, seed=seed + 2).clamp(min=0)      # a post-ReLU activation: half of it exact zeros (the mask is > 0, not >= 0)
        ld = N + 8 if spec["aux"] == "pad" else N
        kw["aux"], kw["ldaux"] = _padded(a, ld)[1], ld
        mk["aux"] = a.double()
    if spec.get("p"):
        kw.update(drop_p=spec["p"], rng_state=RNG.to(DEV), rng_stream=STREAM)
        mk.update(keep=keep_mask(M, N, spec["p"], RNG, STREAM), p=spec["p"])
    if spec.get("res"):
        r = _f32(M, N, seed=seed + 3) if spec["res"] == "f32" else _bf(M, N, seed=seed + 3)
        ld = N + 16 if spec["res"] == "bf16pad" else N
        kw["res"], kw["ldr"] = _padded(r, ld)[1], ld
        mk["res"] = r.double()
    ldc = N + 8
    C = _nan(M, ldc, dtype=out_dtype)
    if spec.get("accum"):
        c0 = _f32(M, N, seed=seed + 4).to(out_dtype)
        C[:, :N] = c0.to(DEV)
        kw["accum"], mk["c0"] = True, c0.double()
    kw["relu_last"] = mk["relu_last"] = bool(spec.get("relu_last"))
    return kw, mk, C, ldc


@pytest.mark.parametrize("out_dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_epilogue_order(out_dtype):
    """every flag alone and every combination the engine issues, tiles 1 and 2, in the order gemm16_nt_kernel applies them"""
    from mmfn_amd import ops16
    M, N, K = EPI_M, EPI_N, EPI_K
    A, B, pre, S = _nt_inputs(M, N, K, seed=40)
    Ad, Bd = A.to(DEV), B.to(DEV)
    worst = 0.0
    for name, spec in EPI_CASES:
        if spec.get("res") == "f32" and out_dtype != torch.float32:
            continue          # MMFN_EPI16_RES_F32 is the transformers' fp32 residual stream: issued with an fp32 output only
        for tile, stages in [(1, 3), (2, 2)]:
            kw, mk, C, ldc = _epi_operands(M, N, spec, out_dtype)
            what = "epilogue %s | tile %d" % (name, tile)
            ref, E, _, _ = epilogue_model(pre, acc_budget(S, K), what=what, **mk)
            ops16.gemm16(ops16.G16_NT, Ad, Bd, C, M, N, K, K, K, ldc, tile=tile, stages=stages, **kw)
            worst = max(worst, check_out(C[:, :N], ref, E, what, K))
            assert torch.isnan(C[:, N:]).all(), what + ": padding columns of C were written"
    print("bf16-err | NT epilogue %s | largest err/bound %.3g" % (out_dtype, worst))


def test_gelu_at_its_own_error_term():
    """bias + GELU over products a thousand times smaller than the bias: the accumulation budget (which hides a GELU constant that is
    off in the fifth digit at K = 128) shrinks below GELU's own term, so the activation itself is pinned to a few fp32 ulps"""
    from mmfn_amd import ops16
    M, N, K = EPI_M, EPI_N, 64
    A, B = _bf(M, K, seed=45), _bf(N, K, scale=1e-3, seed=46)
    bias = _f32(N, scale=1.5, seed=47)
    pre, S = A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()
    for tile in (1, 2):
        what = "epilogue bias+gelu, small products | tile %d" % tile
        ref, E, _, _ = epilogue_model(pre, acc_budget(S, K), bias=bias.double(), gelu=True, what=what)
        C = _nan(M, N, dtype=torch.float32)
        ops16.gemm16(ops16.G16_NT, A.to(DEV), B.to(DEV), C, M, N, K, K, K, N, bias=bias.to(DEV), gelu=True, tile=tile, stages=2)
        check_f32(C, ref, E, what)


# ------------------------------------------------------------------ c. statistics by-products
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_statistics_by_products(mode):
    """M = 136: the last 64-row tile holds 8 rows and its second wave row none - that partial row must be 0, not stale"""
    from mmfn_amd import ops16
    M, N, K = EPI_M, EPI_N, EPI_K
    A, B, pre, S = _nt_inputs(M, N, K, seed=60)
    Ad, Bd = A.to(DEV), B.to(DEV)
    E0 = acc_budget(S, K)
    variants = {0: [("bias", dict(bias=1)), ("plain", {})],
                1: [("mask", dict(aux="packed")), ("bias+relu", dict(bias=1, relu=1))],
                2: [("residual, relu mask", dict(res="bf16")), ("residual, no mask", dict(res="bf16"))]}[mode]
    for vi, (name, spec) in enumerate(variants):
        for tile in (1, 2, 3, 4):
            kw, mk, C, ldc = _epi_operands(M, N, spec, BF)
            C = _nan(M, N)       # mode 2 indexes bn_x / bn_y with ldc: packed
            what = "stats mode %d %s | tile %d" % (mode, name, tile)
            ref, E, _, _ = epilogue_model(pre, E0, what=what, **mk)
            rows = gemm_stats_rows(ops16.G16_NT, M, N, K, tile)
            assert rows == 2 * ((M + TILE_BM[tile] - 1) // TILE_BM[tile])
            stats = _nan(rows + 2, 2, N, dtype=torch.float64)
            bn = None
            if mode == 2:
                y, x = (_bf(M, N, seed=61).clamp(min=0) if vi == 0 else None), _bf(M, N, scale=2.0, seed=62)
                mean, rstd = _f32(N, scale=0.1, seed=63), torch.rand(N, generator=_g(64)) + 0.5
                bn = (None if y is None else y.to(DEV), x.to(DEV), mean.to(DEV), rstd.to(DEV))
            ops16.gemm16(ops16.G16_NT, Ad, Bd, C, M, N, K, K, K, N, tile=tile, stages=3, stats=stats, stats_mode=mode, bn=bn, **kw)
            check_bf16(C, ref, E, what, K)
            if mode == 0:
                terms = ((pre, E0), None)
            elif mode == 1:
                terms = ((ref, E), None)
            else:
                terms = stats2_terms(C, y, x, mean, rstd)
            check_stats(stats, rows, terms, what)


# ------------------------------------------------------------------ d. TN (form 3)
def test_tn_tiles_stages_splits_and_accumulate():
    """C[M,N] (+)= sum_k A[k,M] B[k,N] through the LDS transpose reads: the smallest legal problem, a contraction that is no multiple
    of 8, tiles x stages, splitk 0 / 1 / 2 / 3 / more than the k-tiles (clamped), with and without ACCUM, ldc = N + 4"""
    from mmfn_amd import ops16
    worst = 0.0
    for (M, N, Kc) in [(8, 8, 8), (72, 136, 300), (136, 72, 328)]:
        A, B = _bf(Kc, M, seed=70 + M), _bf(Kc, N, seed=71 + M)
        A64, B64 = A.double(), B.double()
        pre, S = A64.t() @ B64, A64.abs().t() @ B64.abs()
        c0 = _f32(M, N, seed=72)
        Ad, Bd = A.to(DEV), B.to(DEV)
        nkt = (Kc + 63) // 64
        runs = [(t, s, 1, False) for t in (1, 2, 3, 4) for s in (2, 3, 4)]
        runs += [(t, 2 + (t + sk) % 3, sk, acc) for t in (1, 2, 3, 4) for sk in (0, 1, 2, 3, 99) for acc in (False, True)]
        for tile, stages, sk, acc in runs:
            Cb = _nan(M, N + 4, dtype=torch.float32)
            ref, E = pre, acc_budget(S, Kc) + (min(max(sk, 1), nkt) + 1) * U * S
            if acc:
                Cb[:, :N] = c0.to(DEV)
                ref = pre + c0.double()
                E = E + U * ref.abs()
            ops16.gemm16(ops16.G16_TN, Ad, Bd, Cb, M, N, Kc, M, N, N + 4, tile=tile, stages=stages, splitk=sk, accum=acc)
            what = "TN (%d,%d,%d) tile %d stages %d splitk %d accum %d" % (M, N, Kc, tile, stages, sk, acc)
            worst = max(worst, check_f32(Cb[:, :N], ref, E, what))
            assert torch.isnan(Cb[:, N:]).all(), what + ": padding columns of C were written"
    print("bf16-err | TN | largest err/E %.3g" % worst)


# ------------------------------------------------------------------ g. refusals
def _desc(**f):
    from mmfn_amd._lib import Gemm16Desc
    d = Gemm16Desc()
    for k, v in f.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


def test_gemm_bf16_refusals_leave_the_outputs_untouched():
    """every descriptor the launcher must refuse returns MMFN_EINVAL, and C / stats / workspace are still all NaN afterwards"""
    from mmfn_amd._lib import EPI16_OUT_F32, EPI_ACCUM, EPI_MASK_AUX, EPI_RELU_LAST, EPI_RESIDUAL, lib, stream
    L = lib()
    a = torch.zeros(256, 256, dtype=BF, device=DEV)          # large enough for every operand shape below
    b = torch.zeros(1152, 256, dtype=BF, device=DEV)
    f32v = torch.zeros(256, device=DEV)
    nt = dict(A=a, B=b, M=128, N=64, K=128, lda=128, ldb=128, ldc=64, form=0, tile=2, stages=2)
    conv = dict(H=8, W=8, Cin=64, OH=8, OW=8, Cout=64, KH=3, KW=3, stride=1, pad=1)
    tn = dict(A=a, B=b, M=64, N=64, K=128, lda=64, ldb=64, ldc=64, form=3, tile=2, stages=2, flags=EPI16_OUT_F32)
    wg = dict(tn, form=4, N=576, ldc=576, **conv)
    table = [
        ("K % 64", dict(nt, K=96, lda=96, ldb=96)),
        ("N % 8", dict(nt, N=60)),
        ("lda % 8", dict(nt, lda=132)),
        ("ldb % 8", dict(nt, ldb=132)),
        ("ldc % 8", dict(nt, ldc=68)),
        ("RESIDUAL, null res", dict(nt, flags=EPI_RESIDUAL, ldr=64)),
        ("RESIDUAL, ldr % 8", dict(nt, flags=EPI_RESIDUAL, res=a, ldr=68)),
        ("MASK_AUX, null aux", dict(nt, flags=EPI_MASK_AUX, ldaux=64)),
        ("MASK_AUX, ldaux % 8", dict(nt, flags=EPI_MASK_AUX, aux=a, ldaux=68)),
        ("stats mode 2, fp32 out", dict(nt, flags=EPI16_OUT_F32, stats=True, stats_mode=2, bn_x=a, bn_mean=f32v, bn_rstd=f32v)),
        ("stats mode 2, no bn_x", dict(nt, stats=True, stats_mode=2, bn_mean=f32v, bn_rstd=f32v)),
        ("stats mode 3", dict(nt, stats=True, stats_mode=3)),
        ("stats mode 1 + ACCUM", dict(nt, stats=True, stats_mode=1, flags=EPI_ACCUM)),
        ("stats mode 1 + RELU_LAST", dict(nt, stats=True, stats_mode=1, flags=EPI_RELU_LAST)),
        ("conv, channels / 64 = 3", dict(nt, form=1, M=64, K=9 * 192, ldb=9 * 192, **dict(conv, Cin=192))),
        ("conv, K != KH * KW * channels", dict(nt, form=1, M=64, K=512, ldb=512, **conv)),
        ("dgrad, K != KH * KW * channels", dict(nt, form=2, M=64, K=512, ldb=512, **conv)),
        ("TN, bf16 out", dict(tn, flags=0)),
        ("TN, M % 8", dict(tn, M=60, lda=64)),
        ("TN, M < 8", dict(tn, M=4, lda=8)),
        ("TN, N % 8", dict(tn, N=60)),
        ("wgrad, OW = 6", dict(wg, OW=6, OH=8, K=96)),
        ("wgrad, Cin % tile", dict(wg, tile=1, Cin=64, M=128, lda=128)),
        ("split without workspace", dict(tn, K=256, splitk=2, workspace=None)),
        ("form 5", dict(tn, form=5)),
        ("form 5, bf16", dict(nt, form=5)),
    ]
    for name, f in table:
        C = _nan(256 * 1152, dtype=torch.float32)
        stats = _nan(8, 2, 256, dtype=torch.float64)
        f = dict(f)
        if f.get("stats") is True:
            f["stats"] = stats
        d = _desc(C=C, **f)
        rc = L.mmfn_gemm_bf16(ctypes.byref(d), stream())
        torch.cuda.synchronize()
        print("bf16-err | refusal %s | code %d" % (name, rc))
        assert rc == EINVAL, "%s: returned %d" % (name, rc)
        assert torch.isnan(C).all() and torch.isnan(stats).all(), name + ": an output was written"
    # the same table through the wrapper: MMFNLibraryError with "code -1"
    from mmfn_amd import ops16
    from mmfn_amd._lib import MMFNLibraryError
    with pytest.raises(MMFNLibraryError, match="code -1"):
        ops16.gemm16(ops16.G16_NT, a, b, _nan(128, 64), 128, 64, 96, 96, 96, 64, tile=2, stages=2)
