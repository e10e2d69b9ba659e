"""Chains of ResNet BasicBlocks through the engine's fp32 path (engine.BasicBlock / ResNetTrunk.layer_fwd / layer_bwd), each chain
alone against the same oracle._BasicBlock modules in float64 on the CPU.

The blocks are built standalone at the smallest shapes that still reach every path: the lazy BatchNorm apply inside the next
convolution's F(4x4) input transform (PendingBN), the ReLU sign recomputed from the convolution output, the BatchNorm backward
formed inside the Winograd output-gradient transform, the skip gradient as ge_out / dx_res, batch statistics out of the output
transform, and - on a second step - the filter transforms from the grouped launch.  A spy on ops._call / ops.gemm asserts, per case,
that the claimed kernels really ran.

ReLU signs.  A pre-activation within rounding of zero may take either sign in fp32, and one flipped element breaks any gradient
bound.  Every case therefore has a fixed seed (tools/trunk_test_seeds.py scans for them on the CPU) for which the float64
reference has, at every ReLU site (bn1 output and block output of every block), min |pre| >= tau * max |pre|; the test asserts
that on the reference alone, then asserts that the GPU's pre-activation at every site is within tau * max |pre| of the reference
(tau = 2e-5, the bound test_winograd_conv_and_dgrad holds F(4x4) to).  Together the two exclude a flip.  Where the activation was
never written, the GPU pre-activation is formed in float64 on the host from the engine's saved convolution output, its batch
mean / rstd, the BatchNorm parameters and the skip tensor.

Batch statistics follow from the convolution output, which carries an error of up to tau * max |co| per element, so
|mean - ref| <= tau * max |co| and |rstd / ref - 1| <= tau * max |co| * ref (first order: d std <= the per-element error).

Gradients, per tensor in L2 norm (test_branches_gpu.py's construction with test_train_step_matches_oracle's trunk factor):
    |g_gpu - g64| <= 12 * max(e_cpu, med_cpu * |g64|) + 2e-5 * |g64|
e_cpu: the error of the fp32 CPU evaluation of the same modules against float64, med_cpu: its median relative error over the
case's tensors.  Figures of one run: profiles/trunk_tests_err.txt; what the tests catch: profiles/trunk_tests_mutations.txt."""
import copy
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = 2e-5
NAN = float("nan")

# blocks: (cin, cout, stride) per block; x: (B, H, W) of the NHWC input; seed: the step-one draw; seed2: the step-two draw
# (perturbed filters, new input and gradient) for the cases that run a second step.  Seeds from tools/trunk_test_seeds.py.
CASES = {
    "A": dict(blocks=((64, 64, 1),) * 3, x=(2, 8, 8), seed=1305, seed2=7, tau=TAU),
    "B": dict(blocks=((64, 128, 2), (128, 128, 1)), x=(4, 8, 8), seed=381, seed2=None, tau=TAU),
    "C": dict(blocks=((256, 256, 1),) * 2, x=(2, 4, 4), seed=83, seed2=375, tau=TAU),
    "D": dict(blocks=((512, 512, 1),), x=(2, 4, 4), seed=225, seed2=None, tau=TAU),
    "E": dict(blocks=((64, 64, 1),) * 2, x=(4, 6, 6), seed=12, seed2=None, tau=TAU),
    "F": dict(blocks=((64, 64, 1),) * 2, x=(3, 7, 7), seed=248, seed2=None, tau=TAU),
    "G": dict(blocks=((64, 64, 1),) * 2, x=(2, 4, 8), seed=49, seed2=None, tau=TAU),
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ the modules and their inputs (CPU only: the seed scan uses these)
def out_shape(case):
    B, H, W = CASES[case]["x"]
    for _, cout, s in CASES[case]["blocks"]:
        H, W = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    return B, H, W, cout


def draw_io(case, g):
    """x = relu(randn) as a previous block would leave it (NHWC), and the upstream gradient randn."""
    B, H, W = CASES[case]["x"]
    x = torch.relu(torch.randn(B, H, W, CASES[case]["blocks"][0][0], generator=g))
    return x, torch.randn(out_shape(case), generator=g)


def build_case(case, seed):
    """fp32 master copy of the chain (nn.Sequential of oracle._BasicBlock, train mode): He-scaled filters, gamma = rand + 0.5,
    beta = 0.2 * randn; and the step-one input / upstream gradient."""
    from oracle.model import _BasicBlock
    g = _gen(seed)
    mods = []
    for cin, cout, stride in CASES[case]["blocks"]:
        m = _BasicBlock(cin, cout, stride)
        m.stride = stride           # what engine.BasicBlock reads off its module
        with torch.no_grad():
            for sub in m.modules():
                if isinstance(sub, torch.nn.Conv2d):
                    fan_in = sub.weight[0].numel()
                    sub.weight.copy_(torch.randn(sub.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                elif isinstance(sub, torch.nn.BatchNorm2d):
                    sub.weight.copy_(torch.rand(sub.weight.shape, generator=g) + 0.5)
                    sub.bias.copy_(torch.randn(sub.bias.shape, generator=g) * 0.2)
        mods.append(m)
    seq = torch.nn.Sequential(*mods).train()
    x, gout = draw_io(case, g)
    return seq, x, gout


def draw_step_two(case, seq, seed2):
    """{conv weight name: additive perturbation (5 % of the filter's rms)}, new input, new upstream gradient."""
    g = _gen(1000003 + seed2)
    delta = {n: torch.randn(p.shape, generator=g) * (0.05 * p.detach().pow(2).mean().sqrt().item())
             for n, p in seq.named_parameters() if p.dim() == 4}
    x, gout = draw_io(case, g)
    return delta, x, gout


def perturb(seq, delta):
    with torch.no_grad():
        for n, p in seq.named_parameters():
            if n in delta:
                p.add_(delta[n].to(p.dtype))


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().double()


def run_ref(ref, x, gout=None):
    """One pass of the chain `ref` (any dtype; train or eval mode as it stands) on the NHWC input x, spelled out block by block so
    that the intermediates can be kept (it is checked against the modules' own forward); with gout also the backward.
    -> dict: out, sites {name: pre-activation}, co {bn name: convolution output}, stats {bn name: (mean, rstd)}, grads {name: g},
    everything float64, NHWC / [Co,KH,KW,Ci]."""
    dt = next(ref.parameters()).dtype
    for p in ref.parameters():
        p.grad = None
    xin = x.to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(gout is not None)
    with torch.no_grad():
        chk = copy.deepcopy(ref)(xin.detach().clone())
    sites, co = {}, {}
    with torch.set_grad_enabled(gout is not None):
        h = xin
        for j, m in enumerate(ref):
            pre = "%d." % j
            c1 = m.conv1(h)
            p1 = m.bn1(c1)
            c2 = m.conv2(torch.relu(p1))
            if m.downsample is None:
                skip = h
            else:
                cd = m.downsample[0](h)
                skip = m.downsample[1](cd)
                co[pre + "downsample.1"] = cd
                sites[pre + "downsample.1"] = skip      # no ReLU here: not part of the sign margin
            p2 = m.bn2(c2) + skip
            co[pre + "bn1"], co[pre + "bn2"] = c1, c2
            sites[pre + "bn1"], sites[pre + "out"] = p1, p2
            h = torch.relu(p2)
        assert torch.equal(h.detach(), chk), "the spelled-out chain is the modules' own forward"
        if gout is not None:
            h.backward(gout.to(dt).permute(0, 3, 1, 2))
    r = dict(out=_nhwc(h), sites={k: _nhwc(v) for k, v in sites.items()}, co={k: _nhwc(v) for k, v in co.items()}, stats={}, grads={})
    bns = dict(ref.named_modules())
    for k, c in r["co"].items():
        c2d = c.reshape(-1, c.shape[-1])
        if ref.training:
            r["stats"][k] = (c2d.mean(0), (c2d.var(0, unbiased=False) + bns[k].eps).rsqrt())
        else:
            r["stats"][k] = (bns[k].running_mean.double(), (bns[k].running_var.double() + bns[k].eps).rsqrt())
    if gout is not None:
        r["grads"]["x"] = _nhwc(xin.grad)
        for n, p in ref.named_parameters():
            r["grads"][n] = _nhwc(p.grad) if p.dim() == 4 else p.grad.detach().double()
    return r


def relu_sites(sites):
    return {k: v for k, v in sites.items() if not k.endswith("downsample.1")}


def sign_margin(sites):
    """min over the ReLU sites of min |pre| / max |pre|: the tau a case's seed qualifies for."""
    return min((v.abs().min() / v.abs().max()).item() for v in relu_sites(sites).values())


# ------------------------------------------------------------------ the engine side
class _Layout(object):
    """Parameters [Co,KH,KW,Ci] / [C] on the device under the names "layer1.<block>.<param>"; gradient views NaN-filled."""

    def __init__(self, seq):
        self.p = {}
        for n, p in seq.named_parameters():
            t = p.detach().permute(0, 2, 3, 1) if p.dim() == 4 else p.detach()
            self.p["layer1." + n] = t.contiguous().to(DEV)
        self.gr = {k: torch.full_like(v, NAN) for k, v in self.p.items()}

    def w(self, name):
        return self.p[name]

    def g(self, name):
        return self.gr[name]

    def load(self, seq):
        for n, p in seq.named_parameters():
            t = p.detach().permute(0, 2, 3, 1) if p.dim() == 4 else p.detach()
            self.p["layer1." + n].copy_(t.contiguous())      # in place: the engine's ConvBN objects hold these tensors

    def poison(self):
        for v in self.gr.values():
            v.fill_(NAN)


class _Spy(object):
    """Every ops._call as (name, args) and every ops.gemm as ("gemm", a_mode, b_mode, conv geometry or None, batch)."""

    def __init__(self, monkeypatch):
        from mmfn_amd import ops
        self.calls = []
        real_call, real_gemm = ops._call, ops.gemm

        def call(name, *a):
            self.calls.append((name, a))
            return real_call(name, *a)

        def gemm(A, B, C, M, N, K, lda, ldb, ldc, a_mode=0, b_mode=0, **kw):
            self.calls.append(("gemm", (a_mode, b_mode, kw.get("conv"), kw.get("batch", 1))))
            return real_gemm(A, B, C, M, N, K, lda, ldb, ldc, a_mode, b_mode, **kw)

        monkeypatch.setattr(ops, "_call", call)
        monkeypatch.setattr(ops, "gemm", gemm)

    def clear(self):
        del self.calls[:]

    def named(self, name):
        return [a for n, a in self.calls if n == name]

    def names(self):
        return {n for n, _ in self.calls}

    def convs(self, a_mode, b_mode):
        """Geometries (H, W, Cin, OH, OW, Cout, KH, KW, stride, pad) of the implicit-GEMM launches of this operand form."""
        return [a[2] for n, a in self.calls if n == "gemm" and a[2] is not None and (a[0], a[1]) == (a_mode, b_mode)]


class _Setup(object):
    def __init__(self, case, monkeypatch):
        from mmfn_amd import engine
        cfg = CASES[case]
        self.case, self.tau = case, cfg["tau"]
        seq, self.x, self.gout = build_case(case, cfg["seed"])
        self.seq = seq                                        # fp32 master
        self.ref64 = copy.deepcopy(seq).double()
        self.ref32 = copy.deepcopy(seq)
        self.lay = _Layout(seq)
        self.mods = copy.deepcopy(seq).to(DEV)                # the `mod` of engine.BasicBlock: stride, the BatchNorm modules
        self.stub = types.SimpleNamespace(wino_layers={}, wino_table=None, act_dtype=torch.float32, fz=lambda *g: False, folded={})
        t = engine.ResNetTrunk.__new__(engine.ResNetTrunk)
        t.name, t.stem = "t", None
        t.layers = {1: [engine.BasicBlock("t.l1.%d" % j, self.lay, "layer1.%d" % j, m) for j, m in enumerate(self.mods)]}
        self.trunk, self.blocks = t, t.layers[1]
        self.ctx = engine.Ctx(engine.Buffers(DEV), True, (0.0, 0.0, 0.0), None, engine=self.stub)
        self.spy = _Spy(monkeypatch)

    def bn_modules(self):
        """{reference bn name: the engine's ConvBN}"""
        out = {}
        for j, blk in enumerate(self.blocks):
            out["%d.bn1" % j], out["%d.bn2" % j] = blk.c1, blk.c2
            if blk.down is not None:
                out["%d.downsample.1" % j] = blk.down
        return out


def _cpu(t):
    return t.detach().cpu().double()


def _close(case, what, got, ref, tol, scale=None):
    """max |got - ref| <= tol * scale (default: max |ref|); prints the figure."""
    scale = ref.abs().max().item() if scale is None else scale
    err = (got - ref).abs().max().item()
    print("trunk-err block | %s %s | err/scale %.3g | tol %.3g" % (case, what, err / max(scale, 1e-300), tol))
    assert torch.isfinite(got).all(), "%s %s: not finite" % (case, what)
    assert err <= tol * scale, "%s %s: max err %g vs scale %g (tol %g)" % (case, what, err, scale, tol)


def _gpu_forward_state(S, x):
    """Pre-activations at every site formed in float64 on the host from what the engine saved, the written activations (None
    where never written), the convolution outputs and the batch statistics."""
    sites, written, co, stats = {}, {}, {}, {}
    h = x.double()
    for j, blk in enumerate(S.blocks):
        def bn(cb, key):
            c, mean, rstd = _cpu(cb.saved[1]), _cpu(cb.saved[3]), _cpu(cb.saved[4])
            co[key], stats[key] = c, (mean, rstd)
            return (c - mean) * rstd * _cpu(cb.bn_w) + _cpu(cb.bn_b)
        pre = "%d." % j
        sites[pre + "bn1"] = bn(blk.c1, pre + "bn1")
        written[pre + "bn1"] = None if blk.c1.saved[2] is None else _cpu(blk.c1.saved[2])
        skip = h
        if blk.down is not None:
            sites[pre + "downsample.1"] = bn(blk.down, pre + "downsample.1")
            assert blk.down.saved[2] is not None
            skip = written[pre + "downsample.1"] = _cpu(blk.down.saved[2])
        sites[pre + "out"] = bn(blk.c2, pre + "bn2") + skip
        assert blk.c2.saved[2] is not None, "a block output is always written (the next skip connection reads it)"
        h = written[pre + "out"] = _cpu(blk.c2.saved[2])
    return sites, written, co, stats


def _check_forward(S, tag, x, out, r64, r32):
    """A training forward: the sign margin of the reference, then every site, written activation, convolution output and batch
    statistic of the GPU against it."""
    case, tau = S.case, S.tau
    margin = sign_margin(r64["sites"])
    print("trunk-err block | %s %s sign margin min|pre|/max|pre| %.3g | tau %.3g" % (case, tag, margin, tau))
    assert margin >= tau, "%s %s: the seed does not qualify (margin %g < tau %g), see tools/trunk_test_seeds.py" % (case, tag, margin, tau)
    sites, written, co, stats = _gpu_forward_state(S, x)
    for k, ref in r64["sites"].items():
        scale = ref.abs().max().item()
        _close(case, "%s pre-activation %s" % (tag, k), sites[k], ref, tau)
        assert (r32["sites"][k] - ref).abs().max().item() <= tau * scale, "the fp32 yardstick must not have flipped a sign either"
        if written[k] is not None:
            act = ref if k.endswith("downsample.1") else torch.relu(ref)
            _close(case, "%s written activation %s" % (tag, k), written[k], act, tau, scale)
    _close(case, "%s output" % tag, _cpu(out), r64["out"], tau, r64["sites"]["%d.out" % (len(S.blocks) - 1)].abs().max().item())
    for k, (mean, rstd) in r64["stats"].items():
        cmax = r64["co"][k].abs().max().item()
        _close(case, "%s conv output %s" % (tag, k), co[k], r64["co"][k], tau)
        _close(case, "%s batch mean %s" % (tag, k), stats[k][0], mean, tau, cmax)
        rel = ((stats[k][1] / rstd - 1.0).abs() / (cmax * rstd)).max().item()
        print("trunk-err block | %s %s batch rstd %s | rel err / (max|co| * rstd) %.3g | tol %.3g" % (case, tag, k, rel, tau))
        assert rel <= tau


def _check_running(S, tag, steps):
    ref_bn = dict(S.ref64.named_modules())
    for k, cb in S.bn_modules().items():
        _close(S.case, "%s running_mean %s" % (tag, k), _cpu(cb.bn.running_mean), ref_bn[k].running_mean, 1e-5)
        _close(S.case, "%s running_var %s" % (tag, k), _cpu(cb.bn.running_var), ref_bn[k].running_var, 1e-5)
        assert int(cb.bn.num_batches_tracked.item()) == steps == int(ref_bn[k].num_batches_tracked.item())


def _check_grads(S, tag, dx, r64, r32):
    g64, g32 = r64["grads"], r32["grads"]
    got = {"x": _cpu(dx)}
    for n in g64:
        if n != "x":
            got[n] = _cpu(S.lay.gr["layer1." + n])
    assert set(S.lay.gr) == {"layer1." + n for n in g64 if n != "x"}
    names = [n for n in g64 if g64[n].norm().item() > 0]
    assert len(names) == len(g64)
    rel_cpu = sorted((g32[n] - g64[n]).norm().item() / g64[n].norm().item() for n in names)
    med_cpu = rel_cpu[len(rel_cpu) // 2]
    bad = []
    for n, t in g64.items():
        assert tuple(got[n].shape) == tuple(t.shape), n
        assert not torch.isnan(got[n]).any(), "%s %s: NaN left in the gradient of %s" % (S.case, tag, n)
        norm = t.norm().item()
        e_gpu, e_cpu = (got[n] - t).norm().item(), (g32[n] - t).norm().item()
        bound = 12.0 * max(e_cpu, med_cpu * norm) + 2e-5 * norm
        print("trunk-err block | %s %s grad %s | e_gpu %.3g | e_cpu %.3g | ratio %.3g | |g64| %.3g | e_gpu/|g64| %.3g | bound/|g64| %.3g"
              % (S.case, tag, n, e_gpu, e_cpu, e_gpu / max(e_cpu, 1e-300), norm, e_gpu / norm, bound / norm))
        if not e_gpu <= bound:
            bad.append((n, e_gpu, e_cpu, norm))
    assert not bad, "%s %s gradient error (name, |gpu-f64|, |cpu32-f64|, |f64|): %s" % (S.case, tag, bad)


def _train_step(S, tag, x, gout, steps):
    S.lay.poison()
    S.spy.clear()
    r64, r32 = run_ref(S.ref64, x, gout), run_ref(S.ref32, x, gout)
    out = S.trunk.layer_fwd(S.ctx, 1, x.to(DEV))
    dx = S.trunk.layer_bwd(S.ctx, 1, gout.to(DEV))
    torch.cuda.synchronize()
    _check_forward(S, tag, x, out, r64, r32)
    _check_running(S, tag, steps)
    _check_grads(S, tag, dx, r64, r32)


# ------------------------------------------------------------------ which kernels a case must reach
def _ints(args, n):
    return tuple(args[-1 - n:-1])     # the n integers before the stream argument


def _paths_f4(S, shapes, written_bn1=False):
    """The lazy F(4x4) path: statistics out of the output transform, both forms of the BatchNorm-applying input transform, the
    BatchNorm backward inside the output-gradient transform with the mask read and recomputed, the adjoint with the skip gradient."""
    spy = S.spy
    assert {_ints(a, 4) for a in spy.named("mmfn_wino_output_stats_f32")} == shapes
    assert len(spy.named("mmfn_bn_finalize_stats_f32")) == len(spy.named("mmfn_wino_output_stats_f32"))
    in_bn = spy.named("mmfn_wino_input_bn_f32")       # (x, res, mean, rstd, weight, bias, relu, y, V, B, H, W, C, stream)
    assert any(a[7] is None and a[1] is None for a in in_bn), "bn1 + ReLU applied in c2's transform, never written"
    if len(S.blocks) > 1:
        assert any(a[7] is not None and a[1] is not None for a in in_bn), "block output (bn2 + skip + ReLU) written by the next c1"
    assert {_ints(a, 4) for a in in_bn} <= shapes
    assert all(blk.c1.saved[2] is None for blk in S.blocks), "no bn1 activation was written"
    n3 = sum(1 for blk in S.blocks for cb in (blk.c1, blk.c2) if cb.w.shape[1] == 3 and cb.stride == 1)
    assert len(spy.named("mmfn_bn_bwd_reduce_f32")) == n3
    og = spy.named("mmfn_wino_outgrad_bn_f32")        # (g, y, x, mean, rstd, weight, relu_bias, means, ge_out, dMt, B, H, W, C, stream)
    assert len(og) == n3
    assert any(a[1] is not None and a[6] is None and a[8] is not None for a in og), "mask read from y, ge_out written"
    assert any(a[1] is None and a[6] is not None and a[8] is None for a in og), "mask recomputed from the convolution output"
    adj = spy.named("mmfn_wino_input_adjoint_f32")    # (dV, res, dx, B, H, W, C, stream)
    assert any(a[1] is not None for a in adj) and any(a[1] is None for a in adj)
    assert len(spy.named("mmfn_bn_apply_f32")) == 1 + sum(1 for blk in S.blocks if blk.down is not None), "only the chain's output"


def _paths(S):
    from mmfn_amd._lib import A_COLMAJOR, A_DGRAD, A_IM2COL, B_DGRADW, B_IM2COL, B_NK
    spy, case = S.spy, S.case
    names = spy.names()
    if case in ("A", "C", "D", "G"):
        B, H, W = CASES[case]["x"]
        _paths_f4(S, {(B, H, W, CASES[case]["blocks"][0][1])})
        assert "mmfn_bn_train_stats_f32" not in names and "mmfn_bn_bwd_f32" not in names
        assert {a[4] for a in spy.named("mmfn_wino_weight_f32")} == {4}
    elif case == "B":
        fwd = spy.convs(A_IM2COL, B_NK)
        assert (8, 8, 64, 4, 4, 128, 3, 3, 2, 1) in fwd and (8, 8, 64, 4, 4, 128, 1, 1, 2, 0) in fwd, "strided 3x3 and 1x1 downsample"
        assert len(spy.named("mmfn_bn_train_stats_f32")) == 2 and len(spy.named("mmfn_bn_bwd_f32")) == 2
        assert (8, 8, 64, 4, 4, 128, 3, 3, 2, 1) in spy.convs(A_COLMAJOR, B_IM2COL), "direct weight gradient"
        assert (8, 8, 64, 4, 4, 128, 1, 1, 2, 0) in spy.convs(A_COLMAJOR, B_IM2COL)
        dg = spy.convs(A_DGRAD, B_DGRADW)
        assert (8, 8, 64, 4, 4, 128, 3, 3, 2, 1) in dg and (8, 8, 64, 4, 4, 128, 1, 1, 2, 0) in dg, "direct data gradients"
        _paths_f4(S, {(4, 4, 4, 128)})      # T = B: one tile per image
    elif case == "E":
        assert {a[4] for a in spy.named("mmfn_wino_weight_f32")} == {2} and {a[6] for a in spy.named("mmfn_wino_input_f32")} == {2}
        assert not names & {"mmfn_wino_input_bn_f32", "mmfn_wino_outgrad_bn_f32", "mmfn_wino_input_adjoint_f32", "mmfn_wino_output_stats_f32",
                            "mmfn_bn_bwd_reduce_f32", "mmfn_wino_outgrad_f32"}
        assert len(spy.named("mmfn_bn_apply_f32")) == 4 and len(spy.named("mmfn_bn_train_stats_f32")) == 4, "eager apply"
        assert len(spy.named("mmfn_bn_bwd_f32")) == 4 and len(spy.convs(A_COLMAJOR, B_IM2COL)) == 4, "direct backward"
        assert all(blk.c1.saved[2] is not None for blk in S.blocks)
    elif case == "F":
        assert not [n for n in names if n.startswith("mmfn_wino_")], "odd sides: no Winograd anywhere"
        assert len(spy.convs(A_IM2COL, B_NK)) >= 4 and len(spy.convs(A_COLMAJOR, B_IM2COL)) == 4
        assert len(spy.named("mmfn_bn_apply_f32")) == 4 and len(spy.named("mmfn_bn_bwd_f32")) == 4


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", sorted(CASES))
def test_block_chain_training_step_against_fp64(case, monkeypatch):
    """One training step: chain output, every pre-activation, convolution output and batch statistic, the running statistics,
    the input gradient and every parameter gradient; the kernels the case exists for are asserted to have run."""
    S = _Setup(case, monkeypatch)
    _train_step(S, "step1", S.x, S.gout, 1)
    _paths(S)


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if CASES[c]["seed2"] is not None])
def test_second_step_through_the_grouped_filter_transform(case, monkeypatch):
    """After step one every filter is perturbed and all Winograd filter transforms come from one mmfn_wino_weight_group_f32 launch
    (ctx.wino_ready): step two must match float64 with the NEW filters, without a single per-layer filter transform."""
    from mmfn_amd import ops
    S = _Setup(case, monkeypatch)
    _train_step(S, "step1", S.x, S.gout, 1)
    delta, x2, g2 = draw_step_two(case, S.seq, CASES[case]["seed2"])
    for m in (S.seq, S.ref64, S.ref32):
        perturb(m, delta)
    S.lay.load(S.seq)
    assert len(S.stub.wino_layers) == 2 * len(S.blocks), "every 3x3 convolution registered its kept filter transform"
    for w, u in S.stub.wino_layers.values():
        u.fill_(NAN)       # a layer the grouped launch missed would leave NaN behind
    table = ops.make_wino_group_table(list(S.stub.wino_layers.values()), DEV)
    ops.wino_weight_group(*table)
    S.ctx.wino_ready = True
    S.ctx.wino_names = frozenset(S.stub.wino_layers)
    _train_step(S, "step2", x2, g2, 2)
    registered = {w.data_ptr() for w, _ in S.stub.wino_layers.values()}
    assert not [a for a in S.spy.named("mmfn_wino_weight_f32") if a[0] in registered]
    _paths_f4(S, {CASES[case]["x"] + (CASES[case]["blocks"][0][1],)})


@pytest.mark.parametrize("case", ["A", "B"])
def test_eval_forward_plain_and_folded_against_fp64(case, monkeypatch):
    """Eval over random running statistics: the lazy path (BatchNorm from the running statistics inside the input transform) and
    the BatchNorm-folded single-launch convolution + shift + skip + ReLU path, both against the float64 eval forward."""
    from mmfn_amd import ops
    S = _Setup(case, monkeypatch)
    g = _gen(77)
    ref_bn = dict(S.ref64.named_modules())
    with torch.no_grad():
        for k, cb in S.bn_modules().items():
            rm = torch.randn(cb.cout, generator=g) * 0.1
            rv = torch.rand(cb.cout, generator=g) + 0.5
            cb.bn.running_mean.copy_(rm)
            cb.bn.running_var.copy_(rv)
            ref_bn[k].running_mean.copy_(rm)
            ref_bn[k].running_var.copy_(rv)
    S.ref64.eval()
    r64 = run_ref(S.ref64, S.x)
    scale = r64["sites"]["%d.out" % (len(S.blocks) - 1)].abs().max().item()
    S.ctx.training = False
    out = S.trunk.layer_fwd(S.ctx, 1, S.x.to(DEV))
    torch.cuda.synchronize()
    assert "mmfn_wino_input_bn_f32" in S.spy.names() and "mmfn_bn_eval_prepare_f32" in S.spy.names()
    assert not S.stub.wino_layers, "eval keeps no filter transform"
    sites, written, co, stats = _gpu_forward_state(S, S.x)
    for k, ref in r64["sites"].items():
        _close(case, "eval pre-activation %s" % k, sites[k], ref, S.tau)
        if written[k] is not None:
            act = ref if k.endswith("downsample.1") else torch.relu(ref)
            _close(case, "eval written activation %s" % k, written[k], act, S.tau, ref.abs().max().item())
    for k, (mean, rstd) in r64["stats"].items():
        _close(case, "eval conv output %s" % k, co[k], r64["co"][k], S.tau)
        _close(case, "eval mean %s" % k, stats[k][0], mean, 1e-6)
        _close(case, "eval rstd %s" % k, stats[k][1], rstd, 1e-6)
    _close(case, "eval output", _cpu(out), r64["out"], S.tau, scale)
    for cb in S.trunk.convbns():
        wf, bf = torch.full_like(cb.w, NAN), torch.full((cb.cout,), NAN, device=DEV)
        ops.bn_fold(cb.w, cb.bn_w, cb.bn_b, cb.bn.running_mean, cb.bn.running_var, cb.bn.eps, wf, bf)
        S.stub.folded[cb.name] = (wf, bf)
    S.ctx.folded = True
    S.spy.clear()
    out = S.trunk.layer_fwd(S.ctx, 1, S.x.to(DEV))
    torch.cuda.synchronize()
    n_conv = sum(1 for _ in S.trunk.convbns())
    assert S.spy.names() == {"gemm"} and len(S.spy.calls) == n_conv, "one launch per convolution, nothing else"
    _close(case, "folded eval output", _cpu(out), r64["out"], S.tau, scale)
    for k, cb in S.bn_modules().items():
        if k.endswith("bn1"):       # the written bn1 activation of the folded path
            y = _cpu(S.ctx.bufs.get(cb.name + ".out", tuple(r64["sites"][k].shape)))
            _close(case, "folded eval activation %s" % k, y, torch.relu(r64["sites"][k]), S.tau, r64["sites"][k].abs().max().item())
    for n in S.lay.gr:
        assert torch.isnan(S.lay.gr[n]).all(), "an eval forward writes no gradient"
