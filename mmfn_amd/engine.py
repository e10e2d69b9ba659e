"""Static execution plan of the MMFN training step on one MI355X.

There is no autograd tape and no tracing compiler: forward and backward of every layer are
written out explicitly as sequences of HIP launches (mmfn_amd.ops -> libmmfn_hip.so) over
buffers that are allocated once per batch size.  Nothing allocates or synchronises during a
step, so a whole step can be captured into a hipGraph and replayed (mmfn_amd.model).

Data layout: feature maps are NHWC [B,H,W,C]; transformer tokens are rows of a [B*T, C] matrix,
which is the same memory as an 8x8 NHWC map, so the reference's permute/contiguous copies
around each GPT (model_vec.py:228,240-244) do not exist here.

Backward conventions: `bwd` methods receive dL/d(output) buffers and write parameter gradients
straight into the flat gradient buffer (each parameter has exactly one writer per step).
"""
import contextlib
import math

import os

import torch

from . import ops
from .ops import ACT_GELU, ACT_NONE, ACT_RELU


class Buffers(object):
    """Named, shape-keyed activation buffers: allocated on first use, reused on every later step."""

    def __init__(self, device):
        self.device = device
        self._bufs = {}

    def get(self, name, shape, dtype=torch.float32):
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("buffer %s%s first used during graph capture; run one eager step first" % (name, tuple(shape)))
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._bufs.values())


class Ctx(object):
    """Per-call execution context."""

    def __init__(self, bufs, training, drop_p, rng_state, side=None, engine=None):
        self.bufs = bufs
        self.engine = engine
        self.wino_ready = False   # True: the filters of the registered Winograd layers were transformed by the grouped launch
        self.wino_names = frozenset()   # ... and the layers that launch covered
        self.training = training
        self.drop = drop_p if training else (0.0, 0.0, 0.0)  # (embd, attn, resid)
        self.rng_state = rng_state
        self.side = side  # side stream for work that is off the critical path (weight gradients), or None
        self.side2 = None  # a second one (lane 2's stream): the launch-bound transformers split their side work over both (GPT._offload_side)
        self.side2_used = False
        self.adt = engine.act_dtype if engine is not None else torch.float32   # dtype of activation / activation-gradient buffers
        self.bf16 = self.adt == torch.bfloat16
        self.folded = False  # eval forward over BatchNorm-folded filters (Engine.fold_batchnorm)
        # fz(*gradient views): every one of them belongs to a frozen parameter, so a launch that only writes them is not issued
        self.fz = engine.fz if engine is not None else (lambda *g: False)

    def wino_u(self, name, w):
        """Engine-wide buffer for a layer's transformed filter U [36][Co][Ci]; registers the layer for the grouped transform."""
        eng = self.engine
        u = eng.wino_layers.get(name)
        if u is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Winograd filter buffer %s first used during graph capture; run one eager step first" % name)
            u = (w, torch.empty(36 * w.shape[0] * w.shape[3], dtype=torch.float32, device=w.device))
            eng.wino_layers[name] = u
            eng.wino_table = None   # rebuilt before the next forward; THIS forward transforms the new layer's filter itself
        return u[1]

    def wino_in_table(self, name):
        """True when the grouped launch at the head of this forward transformed this layer's filter (the layer was registered
        when the table was built - a layer that registers later, e.g. for a new image size, is not)."""
        return self.wino_ready and name in self.wino_names

    def offload(self, fn):
        """Run fn (launches that only produce parameter gradients) on the side stream, ordered after everything
        enqueued so far on the current stream.  Inline when no side stream is configured."""
        if self.side is None:
            return fn()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side), ops.lane(1):
            fn()

    def fork_point(self):
        """An event at the current point of the current stream, for offload_at()."""
        if self.side is None:
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ev

    def offload_at(self, ev, fn, second=False):
        """Like offload(), but ordered after the earlier fork_point() `ev` instead of after everything enqueued so far.
        Used to enqueue side work AFTER the chain's next kernel: when a captured graph is replayed, the first-captured child
        of a node stays on the node's hardware queue and later children move to other queues; capturing the chain's
        continuation first keeps the dependent chain on one queue (a queue hop costs 10-16 us of idle time)."""
        if self.side is None or ev is None:
            return fn()
        st, ln = (self.side2, 2) if (second and self.side2 is not None) else (self.side, 1)
        st.wait_event(ev)
        with torch.cuda.stream(st), ops.lane(ln):
            fn()
        if st is self.side2:
            self.side2_used = True

    def rejoin(self):
        """Current stream waits for all offloaded work (before its input buffers are reused)."""
        if self.side is None:
            return
        ev = torch.cuda.Event()
        ev.record(self.side)
        torch.cuda.current_stream().wait_event(ev)
        if self.side2_used:
            ev2 = torch.cuda.Event()
            ev2.record(self.side2)
            torch.cuda.current_stream().wait_event(ev2)
            self.side2_used = False


# ----------------------------------------------------------------------------- conv + BN
# fp32: a BatchNorm apply (+ residual + ReLU) whose consumer is an F(4x4) Winograd convolution runs inside that convolution's input
# transform (PendingBN).  A/B switch; 0 = every BatchNorm apply is its own launch (the round-3 step).
LAZY_BN_APPLY = os.environ.get("MMFN_LAZY_BN", "1") == "1"


# bf16 mode: the same laziness - a 3x3 stride-1 convolution whose input is the PendingBN of its producer runs as
# mmfn_conv3x3_halo_bf16 (csrc/conv16_halo.hip), which applies the producer's BatchNorm (+ skip + ReLU) while it stages its halo
# patch and writes the activation for the pixels it owns.  Measured per shape (tools/halo_bench.py, B = 32): 64 / 128 contraction
# channels 1.3-1.4 x the apply + implicit-GEMM pair; 256 / 512 channels are bound by the filter stream per 64-pixel tile and stay on
# the implicit GEMM (256 channels on the halo kernel measured slower: 16.59 vs 16.25 ms per step).  The same kernel is the data
# gradient of those layers (ConvBN.bwd16).
HALO_MAX_K = 128


class PendingBN(object):
    """The output of a ConvBN whose BatchNorm apply (+ residual) (+ ReLU) has not run: the convolution output and the batch
    statistics are in HBM, the activation y = [relu](bn(co) [+ res]) is not.  Two ways out:
      * consume(...) by an F(4x4) Winograd convolution - the apply runs inside its input transform (ops.conv2d_winograd(x_bn=...),
        csrc/winograd.hip wino4_input_bn_kernel); with want_y the transform also writes y (a block output, which the next
        block's skip connection and the backward's ReLU mask read), otherwise y never exists and the producer's backward
        recomputes the ReLU sign from co;
      * tensor(ctx): the plain apply launch (any other consumer: pooling, token kernels, a strided convolution)."""

    def __init__(self, owner, co, res, relu):
        self.owner, self.co, self.res, self.relu = owner, co, res, relu
        self.shape, self.dtype = co.shape, co.dtype
        self.y = None

    def _out(self, ctx):
        return ctx.bufs.get(self.owner.name + ".out", self.shape, ctx.adt if ctx.bf16 else torch.float32)

    def tensor(self, ctx):
        if self.y is None:
            o = self.owner
            M = self.co.numel() // o.cout
            self.y = self._out(ctx)
            ops.bn_apply(self.co.view(M, o.cout), self.y.view(M, o.cout), o.saved[3], o.saved[4], o.bn_w, o.bn_b, self.relu,
                         res=None if self.res is None else self.res.view(M, o.cout))
            o.saved[2] = self.y
        return self.y

    def consume(self, ctx, want_y):
        """-> the x_bn tuple of ops.conv2d_winograd; afterwards self.y is the written activation (want_y) or stays None."""
        o = self.owner
        if want_y and self.y is None:
            self.y = self._out(ctx)
            o.saved[2] = self.y
            y_out = self.y
        else:
            y_out = None
        return (self.res, o.saved[3], o.saved[4], o.bn_w, o.bn_b, self.relu, y_out)


def as_tensor(ctx, x):
    return x.tensor(ctx) if isinstance(x, PendingBN) else x


class ConvBN(object):
    """conv (bias-free) -> BatchNorm2d -> [+ residual] -> [ReLU]."""

    def __init__(self, name, layout, conv_name, bn_name, bn_mod, stride, pad):
        self.name = name
        self.w = layout.w(conv_name + ".weight")
        self.gw = layout.g(conv_name + ".weight")
        self.bn_w, self.bn_b = layout.w(bn_name + ".weight"), layout.w(bn_name + ".bias")
        self.g_bn_w, self.g_bn_b = layout.g(bn_name + ".weight"), layout.g(bn_name + ".bias")
        self.bn = bn_mod
        self.stride, self.pad = stride, pad
        self.cout = self.w.shape[0]
        self.conv_name = conv_name
        self.w16 = self.w16t = None   # bf16 shadows [Cout,KH,KW,Cin] / [Cin,KH,KW,Cout] (Engine._build_shadows, bf16 mode)

    # ---- the 7x7 stems (3 / 2 input channels) as explicit im2col + plain GEMM (csrc/misc.hip: mmfn_im2col_small)
    def is_stem(self):
        return self.w.shape[3] <= 4

    def stem_conv(self, ctx, x, co, stats=None, w=None, bias=None, relu=False):
        """co [B,OH,OW,Cout] = conv(x) through the patch matrix, which is kept for the weight gradient (stem_wgrad).
        w / bias / relu: the BatchNorm-folded filter and shift of an eval forward (Engine.fold_batchnorm)."""
        Co, KH, KW, Ci = self.w.shape
        K = KH * KW * Ci
        M = co.numel() // Co
        tile = 64 if co.dtype == torch.bfloat16 else 16
        KP = (K + tile - 1) // tile * tile
        col = ctx.bufs.get(self.name + ".col", (M, KP), co.dtype)
        wp = ctx.bufs.get(self.name + ".wpad", (Co, KP), co.dtype)
        ops.im2col_small(x, col, KH, KW, self.stride, self.pad)
        ops.repitch_rows(self.w if w is None else w, wp, Co, K, K, KP)
        if stats is not None:
            ops.linear_fwd(col, wp, None, out=co.view(M, Co), stats=stats)
        elif bias is not None:
            ops.linear_fwd(col, wp, bias, out=co.view(M, Co), relu=relu)
        else:
            ops.linear_fwd(col, wp, None, out=co.view(M, Co))
        self.saved_col = col
        return co

    def stem_wgrad(self, ctx, dco):
        Co, KH, KW, Ci = self.w.shape
        K = KH * KW * Ci
        col = self.saved_col
        KP = col.shape[1]
        if ctx.fz(self.gw):   # frozen filter: no weight gradient
            return
        dwp = ctx.bufs.get(self.name + ".dwpad", (Co, KP))
        ops.linear_dw(dco.view(-1, Co), col, out=dwp)
        ops.repitch_rows(dwp, self.gw, Co, K, KP, K)

    def bwd_pooled(self, ctx, g, idx):
        """Backward of a stem whose BatchNorm + ReLU ran inside the pooling pass (ResNetTrunk.stem_fwd): g = dL/d(pooled), idx
        the pooling's argmax taps.  Neither dL/d(activation) nor the activation exists; no data gradient."""
        x, co, y, mean, rstd, relu = self.saved
        assert relu and y is None
        dco = ctx.bufs.get(self.name + ".dconv", co.shape)
        ops.stem_bn_bwd_pooled(g, idx, co, mean, rstd, self.bn_w, self.bn_b, dco, self.g_bn_w, self.g_bn_b)
        if self.is_stem():
            self.stem_wgrad(ctx, dco)
        elif not ctx.fz(self.gw):
            ops.conv2d_wgrad(dco, x, tuple(self.w.shape), self.stride, self.pad, out=self.gw, v=getattr(self, "saved_v", None))

    def fwd16(self, ctx, x, relu=True, res=None, lazy=False):
        """bf16 mode.  A trunk convolution (bf16 input): direct implicit GEMM on the bf16 MFMA pipe whose epilogue also emits
        the BatchNorm batch-statistics partial sums of its fp32 accumulators (no statistics pass over the output); a stem (fp32
        input from the ingest kernels, 3 / 2 channels): the fp32 convolution, fp32 output, and the BatchNorm apply is where the
        activation becomes bf16.  x may be the PendingBN of the producing ConvBN: a 3x3 stride-1 convolution of up to HALO_MAX_K
        channels then runs as mmfn_conv3x3_halo_bf16 and applies that BatchNorm (+ skip + ReLU) in its loader; lazy: return this
        layer's own PendingBN instead of launching the apply."""
        from . import ops16
        # the LDS-resident-patch kernel (3x3 stride 1): takes the producer's PendingBN as it is and applies it in its loader (pro 1)
        pend = x if isinstance(x, PendingBN) and x.y is None and LAZY_BN_APPLY and not ctx.folded else None
        halo = x.dtype == torch.bfloat16 and x.shape[-1] <= HALO_MAX_K and \
            ops16.halo_ok(tuple(x.shape), tuple(self.w.shape), self.stride, self.pad, pro=1 if pend is not None else 0) > 0
        x_bn = None
        if isinstance(x, PendingBN):
            if halo and pend is not None:
                x_bn = pend.consume(ctx, True)    # (res, mean, rstd, weight, bias, relu, y_out): y is written by this convolution
                xin, x = pend.co, pend.y
            else:
                x = xin = x.tensor(ctx)
        else:
            xin = x
        _, oshape = ops.conv_geom(x.shape, self.w.shape, self.stride, self.pad)
        M = oshape[0] * oshape[1] * oshape[2]
        stem = x.dtype == torch.float32
        if not ctx.training and ctx.folded and (not stem or self.is_stem()):
            # eval over BatchNorm-folded filters (Engine.fold_batchnorm; the closed-loop session): convolution + shift + skip + ReLU
            # in ONE launch of the implicit GEMM, the folded filter as a bf16 shadow
            assert x_bn is None
            wf, bf, wf16 = ctx.engine.folded[self.name]
            y = ctx.bufs.get(self.name + ".out", oshape, ctx.adt)
            if stem:
                self.stem_conv(ctx, x, y, w=wf, bias=bf, relu=relu)
            elif res is None:
                ops16.conv2d_fwd(x, wf16, self.stride, self.pad, y, bias=bf, relu=relu)
            else:
                ops16.conv2d_fwd(x, wf16, self.stride, self.pad, y, bias=bf, res=res.view(M, self.cout), ldr=self.cout, relu_last=relu)
            return y
        col_stem = stem and self.is_stem()   # patch-matrix form: the stem joins the bf16 pipeline (bf16 conv output, statistics from the epilogue)
        co = ctx.bufs.get(self.name + ".conv", oshape, torch.float32 if (stem and not col_stem) else ctx.adt)
        mean = ctx.bufs.get(self.name + ".mean", (self.cout,))
        rstd = ctx.bufs.get(self.name + ".rstd", (self.cout,))
        bn = self.bn
        if col_stem:
            if ctx.training:
                ws = ops.norm_workspace(x.device, 2 * ((M + 63) // 64) * 2 * self.cout * 8)
                self.stem_conv(ctx, x, co, stats=ws)
                rows = ops16.gemm_stats_rows(ops16.G16_NT, M, self.cout, self.saved_col.shape[1])
                ops.bn_finalize_stats(ws, rows, M, self.cout, mean, rstd, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                      bn.eps, bn.momentum)
            else:
                self.stem_conv(ctx, x, co)
        elif stem:
            if ctx.training:
                ops.conv2d_fwd_bn_stats(x, self.w, self.stride, self.pad, co, mean, rstd, bn.running_mean, bn.running_var,
                                        bn.num_batches_tracked, bn.eps, bn.momentum)
            else:
                ops.conv2d_fwd(x, self.w, self.stride, self.pad, out=co)
        elif halo:
            ws = ops.norm_workspace(x.device, 2 * ((M + 63) // 64) * 2 * self.cout * 8) if ctx.training else None
            bn_apply = None if x_bn is None else (x_bn[1], x_bn[2], x_bn[3], x_bn[4], x_bn[0], x_bn[5], x_bn[6])
            rows = ops16.conv3x3_halo(xin, self.w16, co, stats=ws, bn_apply=bn_apply)
            if ctx.training:
                ops.bn_finalize_stats(ws, rows, M, self.cout, mean, rstd, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                      bn.eps, bn.momentum)
        elif ctx.training:
            ws = ops.norm_workspace(x.device, 2 * ((M + 63) // 64) * 2 * self.cout * 8)   # sized for the smallest tile
            ops16.conv2d_fwd(x, self.w16, self.stride, self.pad, co, stats=ws)
            rows = ops16.conv_stats_rows(x.shape, self.w.shape, self.stride, self.pad)   # AFTER the launch: autotune may add the entry
            ops.bn_finalize_stats(ws, rows, M, self.cout, mean, rstd, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                  bn.eps, bn.momentum)
        else:
            ops16.conv2d_fwd(x, self.w16, self.stride, self.pad, co)
        if not ctx.training:
            ops.bn_eval_prepare(bn.running_mean, bn.running_var, mean, rstd, bn.eps)
        self.saved = [x, co, None, mean, rstd, relu]   # saved[2]: the activation, written by PendingBN.tensor() or by the consumer's loader
        pend = PendingBN(self, co, res, relu)
        if lazy and LAZY_BN_APPLY:
            return pend
        return pend.tensor(ctx)

    def bwd16(self, ctx, g, need_dx=True, ge_out=None, dx_res=None, mask_y=None, emit=None):
        """emit: the ConvBN whose BatchNorm receives THIS call's data gradient as its output gradient (the layer below on the
        dependent chain): the data-gradient GEMM's epilogue then also forms the two reductions of that BatchNorm's backward
        (sum ge, sum ge * xhat) from the tile it is storing, so the consumer skips its reduction pass over g, y and x."""
        from . import ops16
        x, co, y, mean, rstd, relu = self.saved
        M = co.numel() // self.cout
        dco = ctx.bufs.get(self.name + ".dconv", co.shape, co.dtype)
        ymask = (y if mask_y is None else mask_y).view(M, self.cout) if relu else None
        pre, self._pre = getattr(self, "_pre", None), None
        if pre is not None and mask_y is None and co.dtype == torch.bfloat16:
            ops16.bn_bwd_partials(pre[0], pre[1], g.view(M, self.cout), ymask, co.view(M, self.cout), mean, rstd, self.bn_w,
                                  dco.view(M, self.cout), self.g_bn_w, self.g_bn_b,
                                  ge_out=None if ge_out is None else ge_out.view(M, self.cout))
        else:
            ops.bn_bwd(g.view(M, self.cout), ymask, co.view(M, self.cout), mean, rstd, self.bn_w, dco.view(M, self.cout),
                       self.g_bn_w, self.g_bn_b, ge_out=None if ge_out is None else ge_out.view(M, self.cout))
        if x.dtype == torch.float32:   # stem: no data gradient
            if self.is_stem():
                self.stem_wgrad(ctx, dco)
            elif not ctx.fz(self.gw):
                ops.conv2d_wgrad(dco, x, tuple(self.w.shape), self.stride, self.pad, out=self.gw)
            return None
        if not ctx.fz(self.gw):
            ops16.conv2d_wgrad(dco, x, tuple(self.w.shape), self.stride, self.pad, self.gw)
        if not need_dx:
            return None
        dx = ctx.bufs.get(self.name + ".dx", x.shape, ctx.adt)
        cin = x.shape[-1]
        extra = {}
        if emit is not None and emit.saved[1].dtype == torch.bfloat16:
            ex, eco, ey, emean, erstd, erelu = emit.saved
            Mx = x.shape[0] * x.shape[1] * x.shape[2]
            part = ctx.bufs.get(emit.name + ".bnpart", (ops16.max_stats_rows(Mx), 2, cin), torch.float64)
            extra = dict(stats=part, stats_mode=2, bn=(ey if erelu else None, eco, emean, erstd))
        # data gradient through the LDS-resident-patch kernel (3x3 stride 1, contraction = this layer's output channels)
        if co.dtype == torch.bfloat16 and self.cout <= HALO_MAX_K and \
                ops16.halo_ok(tuple(co.shape), tuple(self.w16t.shape), self.stride, self.pad) > 0:
            rows = ops16.conv3x3_halo(dco, self.w16t, dx, flip=True, out_res=dx_res, stats=extra.get("stats"), stats_mode=2,
                                      bn2=extra.get("bn"))
            if "stats" in extra:
                emit._pre = (extra["stats"], rows)
            return dx
        if dx_res is not None:
            extra.update(res=dx_res.view(-1, cin), ldr=cin)
        ops16.conv2d_dgrad(dco, self.w16t, tuple(x.shape), tuple(self.w.shape), self.stride, self.pad, dx, **extra)
        if "stats" in extra:   # (after the launch: the autotuner may just have added the shape's table entry)
            g_, _ = ops.conv_geom(tuple(x.shape), tuple(self.w.shape), self.stride, self.pad)
            emit._pre = (extra["stats"], ops16.gemm_stats_rows(ops16.G16_CONV_DGRAD, Mx, cin, g_[6] * g_[7] * g_[5], g_))
        return dx

    def fwd(self, ctx, x, relu=True, res=None, lazy=False, want_x=True):
        """x: an NHWC tensor or the PendingBN of the producing ConvBN.  lazy: return a PendingBN instead of applying the BatchNorm
        (the caller hands it to the next convolution, or calls .tensor()).  want_x (x pending): the producer's activation is
        needed as a tensor as well (it is a block output)."""
        if ctx.bf16:
            return self.fwd16(ctx, x, relu, res, lazy)
        x_bn = None
        if isinstance(x, PendingBN):
            # the producer's BatchNorm apply inside this convolution's input transform: F(4x4) forward, and - when training - a
            # backward that never reads x (transformed input kept, adjoint data gradient)
            wshape, xs = self.w.shape, x.shape
            ok = LAZY_BN_APPLY and not ctx.folded and ops.winograd_f4_ok(xs, wshape, self.stride, self.pad) and x.y is None
            if ok and ctx.training:
                ok = ops.winograd_wgrad_ok(xs, wshape, self.stride, self.pad) and ops.winograd_adjoint_ok(xs, wshape, self.stride, self.pad)
            if ok:
                pend = x
                x_bn = pend.consume(ctx, want_x)
                x = pend.co      # what the transform reads; same shape as the activation
            else:
                x = x.tensor(ctx)
        B = x.shape[0]
        _, oshape = ops.conv_geom(x.shape, self.w.shape, self.stride, self.pad)
        co = ctx.bufs.get(self.name + ".conv", oshape)
        keep_v = keep_u = None
        if ctx.training and ops.winograd_ok(x.shape, self.w.shape, self.stride, self.pad, {}) and \
                ops.winograd_wgrad_ok(x.shape, self.w.shape, self.stride, self.pad):
            # the transformed input of the Winograd path is what the weight gradient needs again: keep it per layer
            keep_v = ctx.bufs.get(self.name + ".winoV", (ops.winograd_v_numel(x.shape),))
            if ops.winograd_adjoint_ok(x.shape, self.w.shape, self.stride, self.pad):
                # ... and the transformed filter is what the data gradient (adjoint of this forward) needs again.  The
                # buffer is engine-wide (it does not depend on the batch): Engine.forward transforms all of them in one launch
                keep_u = ctx.wino_u(self.name, self.w)
        M = oshape[0] * oshape[1] * oshape[2]
        if not ctx.training and ctx.folded:
            assert x_bn is None
            # eval with BatchNorm folded into the filter (Engine.fold_batchnorm): convolution + shift + skip + ReLU in ONE launch,
            # as a direct implicit GEMM (at batch 1 the Winograd form - transform, 36-batch GEMM, transform - measured slower: 4.99 vs
            # 4.59 ms per tick)
            wf, bf = ctx.engine.folded[self.name][:2]
            y = ctx.bufs.get(self.name + ".out", oshape)
            if res is None:
                ops.conv2d_fwd(x, wf, self.stride, self.pad, out=y, bias=bf, relu=relu)
            else:
                ops.conv2d_fwd(x, wf, self.stride, self.pad, out=y, bias=bf, res=res.view(M, self.cout), ldr=self.cout, relu_last=relu)
            return y
        co2 = co.view(M, self.cout)
        mean = ctx.bufs.get(self.name + ".mean", (self.cout,))
        rstd = ctx.bufs.get(self.name + ".rstd", (self.cout,))
        if self.is_stem():
            self.stem_conv(ctx, x, co)
            if ctx.training:
                ops.bn_train_stats(co2, mean, rstd, self.bn.running_mean, self.bn.running_var, self.bn.num_batches_tracked, self.bn.eps,
                                   self.bn.momentum)
            else:
                ops.bn_eval_prepare(self.bn.running_mean, self.bn.running_var, mean, rstd, self.bn.eps)
        elif ctx.training:
            ops.conv2d_fwd_bn_stats(x, self.w, self.stride, self.pad, co, mean, rstd, self.bn.running_mean, self.bn.running_var,
                                    self.bn.num_batches_tracked, self.bn.eps, self.bn.momentum, keep_v=keep_v, keep_u=keep_u,
                                    u_ready=keep_u is not None and ctx.wino_in_table(self.name), x_bn=x_bn)
        else:
            ops.conv2d_fwd(x, self.w, self.stride, self.pad, out=co, x_bn=x_bn)
            ops.bn_eval_prepare(self.bn.running_mean, self.bn.running_var, mean, rstd, self.bn.eps)
        # saved[0]: the input - with x_bn the producer's convolution output stands in: only its SHAPE is read by the backward
        # (the Winograd weight gradient uses the kept transformed input); saved[2]: the activation, None until / unless written
        self.saved = [x, co, None, mean, rstd, relu]
        self.saved_v = keep_v
        self.saved_u = keep_u
        self.x_is_standin = x_bn is not None
        pend = PendingBN(self, co, res, relu)
        if lazy and LAZY_BN_APPLY:
            return pend
        return pend.tensor(ctx)

    def bwd(self, ctx, g, need_dx=True, ge_out=None, dx_res=None, mask_y=None, emit=None):
        """g: dL/dy.  ge_out receives the ReLU-masked g (the residual branch's gradient).
        dx_res is added to dx (gradient arriving at x from another branch).
        mask_y overrides the tensor whose sign gates the ReLU (when y was further modified).
        emit (bf16 mode): see bwd16."""
        if ctx.bf16:
            return self.bwd16(ctx, g, need_dx, ge_out, dx_res, mask_y, emit)
        x, co, y, mean, rstd, relu = self.saved
        M = co.numel() // self.cout
        dco = ctx.bufs.get(self.name + ".dconv", co.shape)
        ymask = relu_bias = None
        if relu:
            ym = y if mask_y is None else mask_y
            if ym is not None:
                ymask = ym.view(M, self.cout)
            else:
                # the forward applied this BatchNorm + ReLU inside the next convolution's input transform and never wrote its
                # output (PendingBN): the backward kernels recompute the sign of bn(co) from co
                relu_bias = self.bn_b
        u = getattr(self, "saved_u", None)
        if need_dx and u is not None:
            # weight and data gradient together in the Winograd domain (shared A dy A^T), and dy = the BatchNorm backward of g
            # is formed inside that transform: only the two reductions run as kernels of their own, dy never goes to HBM
            means = ctx.bufs.get(self.name + ".bnmeans", (2, self.cout))
            ops.bn_bwd_reduce(g.view(M, self.cout), ymask, co.view(M, self.cout), mean, rstd, self.g_bn_w, self.g_bn_b, means,
                              relu_wb=None if relu_bias is None else (self.bn_w, relu_bias))
            dx = ctx.bufs.get(self.name + ".dx", x.shape)
            ops.conv2d_bwd_winograd(dco, x, u, None if ctx.fz(self.gw) else self.gw, dx, v=getattr(self, "saved_v", None), res=dx_res,
                                    bn=(g, None if ymask is None else ymask.view(g.shape), co, mean, rstd, self.bn_w, relu_bias, means,
                                        ge_out))
            return dx
        assert not getattr(self, "x_is_standin", False), "%s: the direct backward needs the input activation" % self.name
        ops.bn_bwd(g.view(M, self.cout), ymask, co.view(M, self.cout), mean, rstd, self.bn_w, dco.view(M, self.cout),
                   self.g_bn_w, self.g_bn_b, ge_out=None if ge_out is None else ge_out.view(M, self.cout), relu_bias=relu_bias)
        if self.is_stem() and not need_dx:
            self.stem_wgrad(ctx, dco)
            return None
        if not ctx.fz(self.gw):
            ops.conv2d_wgrad(dco, x, tuple(self.w.shape), self.stride, self.pad, out=self.gw, v=getattr(self, "saved_v", None))
        if not need_dx:
            return None
        dx = ctx.bufs.get(self.name + ".dx", x.shape)
        if dx_res is None:
            ops.conv2d_dgrad(dco, self.w, tuple(x.shape), self.stride, self.pad, out=dx)
        else:
            cin = x.shape[-1]
            ops.conv2d_dgrad(dco, self.w, tuple(x.shape), self.stride, self.pad, out=dx, res=dx_res, ldr=cin)
        return dx


class BasicBlock(object):
    def __init__(self, name, layout, prefix, mod):
        self.name = name
        s = mod.stride
        self.c1 = ConvBN(name + ".c1", layout, prefix + ".conv1", prefix + ".bn1", mod.bn1, s, 1)
        self.c2 = ConvBN(name + ".c2", layout, prefix + ".conv2", prefix + ".bn2", mod.bn2, 1, 1)
        self.down = None
        if mod.downsample is not None:
            self.down = ConvBN(name + ".down", layout, prefix + ".downsample.0", prefix + ".downsample.1",
                               mod.downsample[1], s, 0)

    def fwd(self, ctx, x):
        """x: tensor, or the PendingBN of the previous block's output.  Returns the PendingBN of this block's output (fp32 path;
        the bf16 mode applies every BatchNorm eagerly): the first BatchNorm + ReLU is applied inside the second convolution's
        input transform and its output is never written; the second BatchNorm + skip + ReLU inside the NEXT block's first
        convolution, which also writes the block output (its own skip connection reads it)."""
        y1 = self.c1.fwd(ctx, x, relu=True, lazy=True, want_x=True)
        x = as_tensor(ctx, x)     # written by c1's input transform if it was pending, else by the apply launch
        skip = x if self.down is None else self.down.fwd(ctx, x, relu=False)
        return self.c2.fwd(ctx, y1, relu=True, res=skip, lazy=True, want_x=False)

    def bwd(self, ctx, g, mask_y=None, emit=None):
        """emit: the ConvBN (the previous block's second convolution) whose BatchNorm this block's input gradient enters."""
        ge = ctx.bufs.get(self.name + ".ge", g.shape, g.dtype)
        g_y1 = self.c2.bwd(ctx, g, ge_out=ge, mask_y=mask_y, emit=self.c1)
        if self.down is None:
            return self.c1.bwd(ctx, g_y1, dx_res=ge, emit=emit)
        dx_skip = self.down.bwd(ctx, ge)
        return self.c1.bwd(ctx, g_y1, dx_res=dx_skip, emit=emit)


class ResNetTrunk(object):
    def __init__(self, name, layout, prefix, mod, with_stem=True, first_layer=1):
        self.name = name
        self.stem = ConvBN(name + ".stem", layout, prefix + ".conv1", prefix + ".bn1", mod.bn1, 2, 3) if with_stem else None
        self.layers = {}
        for li in range(first_layer, 5):
            seq = getattr(mod, "layer%d" % li)
            self.layers[li] = [BasicBlock("%s.l%d.%d" % (name, li, j), layout, "%s.layer%d.%d" % (prefix, li, j), blk)
                               for j, blk in enumerate(seq)]

    def convbns(self):
        if self.stem is not None:
            yield self.stem
        for li in sorted(self.layers):
            for blk in self.layers[li]:
                yield blk.c1
                yield blk.c2
                if blk.down is not None:
                    yield blk.down

    def stem_fwd(self, ctx, x):
        """conv1 -> bn1 -> relu -> maxpool.  fp32 path: the BatchNorm + ReLU are applied inside the pooling pass
        (ops.stem_bn_relu_maxpool) and the stem-resolution activation is never written; a shape ops.stem_pool_ok refuses, the
        bf16 mode and the BatchNorm-folded eval forward keep the apply and the pooling as two launches."""
        y = self.stem.fwd(ctx, x, relu=True, lazy=not ctx.bf16)
        B, H, W, C = y.shape
        fused = isinstance(y, PendingBN) and ops.stem_pool_ok(y.shape, y.dtype)
        p = ctx.bufs.get(self.name + ".pool", (B, (H + 1) // 2, (W + 1) // 2, C), y.dtype)
        idx = ctx.bufs.get(self.name + ".poolidx", p.shape, torch.uint8)
        if fused:
            st = self.stem
            ops.stem_bn_relu_maxpool(y.co, st.saved[3], st.saved[4], st.bn_w, st.bn_b, p, idx)
            self.pool_saved = (None, idx)
            return p
        y = as_tensor(ctx, y)
        ops.maxpool_fwd(y, p, idx)
        self.pool_saved = (y, idx)
        return p

    def stem_bwd(self, ctx, g):
        y, idx = self.pool_saved
        if y is None:   # fused forward: the pooling's backward and the ReLU mask happen in the BatchNorm backward's loaders
            self.stem.bwd_pooled(ctx, g, idx)
            return
        gy = ctx.bufs.get(self.name + ".dpool", y.shape, y.dtype)
        ops.maxpool_bwd(g, idx, gy)
        self.stem.bwd(ctx, gy, need_dx=False)

    def layer_fwd(self, ctx, li, x):
        for blk in self.layers[li]:
            x = blk.fwd(ctx, x)
        return as_tensor(ctx, x)

    def layer_bwd(self, ctx, li, g, mask_y=None):
        blocks = self.layers[li]
        for i in range(len(blocks) - 1, -1, -1):
            g = blocks[i].bwd(ctx, g, mask_y=mask_y if i == len(blocks) - 1 else None, emit=blocks[i - 1].c2 if i > 0 else None)
        return g


# ----------------------------------------------------------------------------- Linear helper
class Linear(object):
    def __init__(self, layout, prefix, bias=True):
        self.w, self.gw = layout.w(prefix + ".weight"), layout.g(prefix + ".weight")
        self.b = layout.w(prefix + ".bias") if bias else None
        self.gb = layout.g(prefix + ".bias") if bias else None
        self.name = prefix + ".weight"
        self.w16 = self.w16t = None   # bf16 shadows [out, in] / [in, out] (Engine._build_shadows, bf16 mode)


class LayerNorm(object):
    def __init__(self, name, layout, prefix):
        self.name = name
        self.w, self.b = layout.w(prefix + ".weight"), layout.w(prefix + ".bias")
        self.gw, self.gb = layout.g(prefix + ".weight"), layout.g(prefix + ".bias")

    def fwd(self, ctx, x, act=ACT_NONE, out=None):
        M, C = x.shape
        y = ctx.bufs.get(self.name + ".y", (M, C), x.dtype) if out is None else out
        mean, rstd = ctx.bufs.get(self.name + ".mu", (M,)), ctx.bufs.get(self.name + ".rs", (M,))
        ops.layernorm_fwd(x, self.w, self.b, y, mean, rstd, act)
        self.saved = (x, mean, rstd, act)
        return y

    def bwd(self, ctx, g, dres=None, out=None, dropped=None, drop_p=0.0, rng_stream=0, colsum=None, defer=False, collect=None):
        """defer: the caller rejoins the side stream before the gradients are consumed (GPT.bwd).  dropped: buffer that receives dx with the dropout mask (p, stream) of the branch consuming dx applied.
        colsum: [C] gradient buffer that receives the column sums of that tensor (the consuming Linear's bias gradient)."""
        x, mean, rstd, act = self.saved
        dx = ctx.bufs.get(self.name + ".dx", x.shape, x.dtype) if out is None else out
        rng = ctx.rng_state if dropped is not None else None
        if (defer is True or isinstance(defer, list)) and ctx.side is not None:
            # the chain only needs dx: the reduction of the per-block partial rows into the weight / bias gradients (and the
            # consuming Linear's bias gradient) goes to the side stream, like the weight-gradient GEMMs (0.8 ms of ~11 us
            # launches per step off the transformers' dependent chain); own partial buffer, it must outlive this call
            M, C = x.shape
            rows = ops.layernorm_bwd_rows(M)
            part = ctx.bufs.get(self.name + ".part", (rows, 3 if colsum is not None else 2, C))
            ops.layernorm_bwd_partial(g, x, self.w, self.b, mean, rstd, dx, part, act, dres=dres, dx_dropped=dropped, drop_p=drop_p,
                                      rng_state=rng, rng_stream=rng_stream, want_colsum=colsum is not None)
            fin = lambda: _ln_finalize(ctx, part, rows, C, self.gw, self.gb, colsum)
            if collect is not None:
                collect.append((part, self.gw, self.gb, colsum, rows, C))   # GPT.bwd: one batched launch for all of them at its end
            elif isinstance(defer, list):
                defer.append(fin)      # the caller decides where the reductions run (GPT.bwd: one fork per block / none)
            else:
                ctx.offload(fin)
            return dx
        ops.layernorm_bwd(g, x, self.w, self.b, mean, rstd, dx, self.gw, self.gb, act, dres=dres, dx_dropped=dropped,
                          drop_p=drop_p, rng_state=rng, rng_stream=rng_stream, dx_colsum=colsum)
        return dx


# ----------------------------------------------------------------------------- GPT fusion transformer
# fp32 eval-mode forwards: ln1 -> key/query/value and ln2 -> mlp.0 as ONE launch each (MMFN_EPI_LN_FOLD: the LayerNorm folded into
# the GEMM, include/mmfn_hip.h mmfn_gemm_desc.ln_c1) - validation and the batch-1 closed-loop tick, where 64 launches less on a
# dependent chain of ~330 are worth 4 % (4.05 vs 4.22 ms per tick).  Such a forward keeps no normalised tensor, so no backward can
# follow it.  Folding in training steps too was measured slower (32.01 vs 31.74 ms per step, tools/experiments/NOTES.md) and removed.
# Side work of the transformers up to this width alternates between TWO side streams (GPT._offload_side): their blocks are
# launch-bound on the chain AND on the side stream (8 against ~14 launches of 5-8 us per block), so the join at the end of the
# transformer waited for the side stream.  Measured (3 interleaved runs each): bf16 step 17.55 -> 17.16 ms, fp32 31.62 -> 31.37;
# C = 512 included: 17.33 / 31.50 (its side work is chip-filling GEMMs); three or four streams: 17.57 / 18.02 and 31.95 (every
# further fork is a queue hop).
SIDE_SPLIT_MAX_C = 256
# The narrow transformers (n_embd 64 / 128, fp32): a block is 2 forward launches (ln1 + q/k/v + attention per (sample, head, half);
# proj + ln2 + mlp per 32-row block) and 3 backward launches (dQ, dK/dV, the row-local rest) instead of 8 and 9 on the dependent
# chain (ops.gpt_block_*, csrc/gpt_block.hip): step 31.00 -> 29.98 ms.


def _dw_db(ctx, dy, x, gw, gb):
    """A Linear's weight AND bias gradient: one GEMM in fp32 (the bias gradient = the column sums of dy, formed from the operand
    fragments of dW = dy^T x: MMFN_EPI_COLSUM_A), column sums + GEMM in the bf16 mode.  Both frozen: no launch; one of them: the
    launch runs as it is and the frozen range is zeroed behind it (Engine._ready)."""
    if ctx.fz(gw, gb):
        return None
    if dy.dtype == torch.bfloat16:
        ops.colsum(dy, gb)
        return ops.linear_dw(dy, x, out=gw)
    return ops.linear_dw(dy, x, out=gw, db=gb)


def _dw(ctx, dy, x, gw):
    """A Linear's weight gradient alone (its bias gradient comes out of a LayerNorm backward); none for a frozen weight."""
    if not ctx.fz(gw):
        ops.linear_dw(dy, x, out=gw)


def _ln_finalize(ctx, part, rows, C, gw, gb, colsum):
    """The row reduction of a LayerNorm backward's partials into its weight / bias gradient (+ the consuming Linear's bias
    gradient); not issued when all of them are frozen."""
    if not ctx.fz(*[t for t in (gw, gb, colsum) if t is not None]):
        ops.layernorm_bwd_finalize(part, rows, C, gw, gb, colsum)


class GPT(object):
    """model_vec.py:136-246 (GPT), :112-133 (Block), :73-109 (SelfAttention)."""

    def __init__(self, name, layout, prefix, mod, cfg, stream_base):
        self.name, self.mod = name, mod
        self.C = mod.n_embd
        self.nh = cfg.n_head
        self.hs = self.C // self.nh
        self.T = mod.pos_emb.shape[1]
        self.n_modal = mod.n_modal
        self.pos, self.g_pos = layout.w(prefix + ".pos_emb"), layout.g(prefix + ".pos_emb")
        self.vel = Linear(layout, prefix + ".vel_emb")
        self.stream_base = stream_base
        self.blocks = []
        C = self.C
        for i in range(len(mod.blocks)):
            bp = "%s.blocks.%d" % (prefix, i)
            blk = {
                "ln1": LayerNorm("%s.b%d.ln1" % (name, i), layout, bp + ".ln1"),
                "ln2": LayerNorm("%s.b%d.ln2" % (name, i), layout, bp + ".ln2"),
                "proj": Linear(layout, bp + ".attn.proj"),
                "fc1": Linear(layout, bp + ".mlp.0"),
                "fc2": Linear(layout, bp + ".mlp.2"),
            }
            blk["wqkv"], blk["g_wqkv"] = layout.packed(bp + ".attn.key.weight", 3 * C, C)
            blk["wqkv_name"] = bp + ".attn.key.weight"
            blk["wqkv16"] = blk["wqkv16t"] = None   # bf16 shadows (Engine._build_shadows)
            blk["bqkv"], blk["g_bqkv"] = layout.packed(bp + ".attn.key.bias", 3 * C)
            blk["fold"] = None   # (wqkv * gamma1, c1, c2, fc1.w * gamma2, c1, c2): Engine._build_ln_fold
            self.blocks.append(blk)
        self.ln_f = LayerNorm(name + ".ln_f", layout, prefix + ".ln_f")
        self._fin_tables = {}   # device pointer tables of the batched LayerNorm finalize, per buffer set

    def fwd(self, ctx, feats, velocity):
        B = velocity.shape[0]
        T, C, nh, hs = self.T, self.C, self.nh, self.hs
        M = B * T
        bufs, nm = ctx.bufs, self.name
        p_embd, p_attn, p_resid = ctx.drop
        adt = ctx.adt
        # The residual stream x (and, in bwd, its gradient) is fp32 in BOTH modes: in the bf16 mode the LayerNorm outputs, q / k / v,
        # the attention output and the MLP hidden - every GEMM operand - are bf16, the sums x + proj(.) and x + mlp(.) are not
        # (what torch.autocast does to model_vec.py:124-132; rounding the stream alone costs 0.03-0.04 of gradient cosine per
        # backward stage, tools/experiments/bf16_where.py)
        sdt = torch.float32
        Wf = (lambda lin: lin.w16) if ctx.bf16 else (lambda lin: lin.w)      # forward operand of a Linear
        x = bufs.get(nm + ".x0", (B, T, C), sdt)
        ops.tokens_fwd(feats, self.pos.view(T, C), self.vel.w.view(C), self.vel.b, velocity, x, p_embd, ctx.rng_state,
                       self.stream_base, frames=self.frames)
        self.velocity = velocity
        x = x.view(M, C)
        self.acts = []
        scale = 1.0 / math.sqrt(hs)
        nb = len(self.blocks)
        # the activations the weight gradients read again, one slab per block (the side stream may lag by several blocks)
        S_a, S_a2 = bufs.get(nm + ".S.a", (nb, M, C), adt), bufs.get(nm + ".S.a2", (nb, M, C), adt)
        S_o, S_h = bufs.get(nm + ".S.att", (nb, M, C), adt), bufs.get(nm + ".S.h", (nb, M, 4 * C), adt)
        self.stacks = (S_a, S_a2, S_o, S_h)
        # the path of this pass, which GPT.bwd follows: "fold" (eval only), "fused" (fp32: both fused launches; bf16 mode: the
        # row-block launch after attention16) or "plain" (the per-op launches)
        if (not ctx.bf16) and ops.current_precision() == "f32" and self.blocks[0]["fold"] is not None and M % 64 == 0 \
                and ctx.engine.ln_fold_now(ctx.training):
            self.path = "fold"
        else:
            self.path = "fused" if self.fused_now(ctx) else "plain"
        fold = self.path == "fold"
        for i, blk in enumerate(self.blocks):
            sb = self.stream_base + 1 + 3 * i
            qkv = bufs.get("%s.b%d.qkv" % (nm, i), (M, 3 * C), adt)
            if self.path == "fused":
                ln1, ln2 = blk["ln1"], blk["ln2"]
                mu1, rs1 = bufs.get(ln1.name + ".mu", (M,)), bufs.get(ln1.name + ".rs", (M,))
                mu2, rs2 = bufs.get(ln2.name + ".mu", (M,)), bufs.get(ln2.name + ".rs", (M,))
                lse = bufs.get("%s.b%d.lse" % (nm, i), (B, nh, T))
                x1 = bufs.get("%s.b%d.x1" % (nm, i), (M, C), sdt)
                x2 = bufs.get("%s.b%d.x2" % (nm, i), (M, C), sdt)
                a, o, a2, h = S_a[i], S_o[i], S_a2[i], S_h[i]
                if not self.fused_attn_now(ctx):   # bf16 mode, or a token count the fused attention launch is not shaped for (rad: 256)
                    ln1.fwd(ctx, x, out=a)
                    ops.linear_fwd(a, blk["wqkv16"] if ctx.bf16 else blk["wqkv"], blk["bqkv"], out=qkv)
                    ops.attention_fwd(qkv[:, C:], qkv, qkv[:, 2 * C:], 3 * C, o, C, lse, B, T, nh, hs, scale, drop_p=p_attn,
                                      rng_state=ctx.rng_state, rng_stream=sb)
                    d = self._desc(blk, B, ctx, sb, weights="fwd16" if ctx.bf16 else "f32", x=x, o=o, x1=x1, a2=a2, mu2=mu2, rs2=rs2,
                                   h=h, x2=x2)
                else:
                    d = self._desc(blk, B, ctx, sb, x=x, a=a, mu1=mu1, rs1=rs1, qkv=qkv, o=o, lse=lse, x1=x1, a2=a2, mu2=mu2,
                                   rs2=rs2, h=h, x2=x2)
                    ops.gpt_block_attn_fwd(d)
                    ln1.saved = (x, mu1, rs1, ACT_NONE)
                ops.gpt_block_mlp_fwd(d)
                ln2.saved = (x1, mu2, rs2, ACT_NONE)
                self.acts.append((x, a, qkv, o, lse, x1, a2, h))
                x = x2
                continue
            if fold:
                # LN(x) . Wqkv^T + b in one launch; a = LN(x) is never formed
                ln = blk["ln1"]
                mu, rs = bufs.get(ln.name + ".mu", (M,)), bufs.get(ln.name + ".rs", (M,))
                wf, c1, c2 = blk["fold"][:3]
                ops.linear_fwd(x, wf, c2, out=qkv, ln_fold=(c1, mu, rs, 1e-5))
                ln.saved = (x, mu, rs, ACT_NONE)
                a = S_a[i]
            else:
                a = blk["ln1"].fwd(ctx, x, out=S_a[i])
                ops.linear_fwd(a, blk["wqkv16"] if ctx.bf16 else blk["wqkv"], blk["bqkv"], out=qkv)
            o = S_o[i]
            lse = bufs.get("%s.b%d.lse" % (nm, i), (B, nh, T))
            # packed columns: [key | query | value]  (reference registration order, model_vec.py:82-84)
            ops.attention_fwd(qkv[:, C:], qkv, qkv[:, 2 * C:], 3 * C, o, C, lse, B, T, nh, hs, scale, drop_p=p_attn,
                              rng_state=ctx.rng_state, rng_stream=sb)
            x1 = bufs.get("%s.b%d.x1" % (nm, i), (M, C), sdt)
            ops.linear_fwd(o, Wf(blk["proj"]), blk["proj"].b, out=x1, res=x, ldr=C, drop_p=p_resid, rng_state=ctx.rng_state,
                           rng_stream=sb + 1)
            h = S_h[i]
            if fold:
                ln = blk["ln2"]
                mu, rs = bufs.get(ln.name + ".mu", (M,)), bufs.get(ln.name + ".rs", (M,))
                wf, c1, c2 = blk["fold"][3:]
                ops.linear_fwd(x1, wf, c2, out=h, relu=True, ln_fold=(c1, mu, rs, 1e-5))
                ln.saved = (x1, mu, rs, ACT_NONE)
                a2 = S_a2[i]
            else:
                a2 = blk["ln2"].fwd(ctx, x1, out=S_a2[i])
                ops.linear_fwd(a2, Wf(blk["fc1"]), blk["fc1"].b, out=h, relu=True)
            x2 = bufs.get("%s.b%d.x2" % (nm, i), (M, C), sdt)
            ops.linear_fwd(h, Wf(blk["fc2"]), blk["fc2"].b, out=x2, res=x1, ldr=C, drop_p=p_resid, rng_state=ctx.rng_state,
                           rng_stream=sb + 2)
            self.acts.append((x, a, qkv, o, lse, x1, a2, h))
            x = x2
        y = self.ln_f.fwd(ctx, x, out=bufs.get(nm + ".ln_f.out", (M, C), adt))
        return y.view(B, T, C)

    def fused_now(self, ctx):
        """The fused block kernels serve this transformer in this pass: fp32 mode and arithmetic, n_embd 64 / 128, 4 heads, T = 192."""
        return (ctx.bf16 or ops.current_precision() == "f32") and ops.gpt_block_rows_supported(self.C, self.T)

    def fused_attn_now(self, ctx):
        """... and the attention launch with the projections as its prologue too (fp32, 4 heads, 192 tokens)."""
        return not ctx.bf16 and ops.gpt_block_supported(self.C, self.nh, self.T)

    def _desc(self, blk, B, ctx, sb, sb_below=0, below_colsum=False, weights="f32", **tensors):
        """weights: "f32" the master weights; "fwd16" / "bwd16" the bf16 mode's [out][in] / transposed [in][out] shadows."""
        p_embd, p_attn, p_resid = ctx.drop
        if weights == "f32":
            w = dict(wqkv=blk["wqkv"], wproj=blk["proj"].w, w1=blk["fc1"].w, w2=blk["fc2"].w)
        elif weights == "fwd16":
            w = dict(wqkv=blk["wqkv16"], wproj=blk["proj"].w16, w1=blk["fc1"].w16, w2=blk["fc2"].w16)
        else:
            w = dict(wqkv=blk["wqkv16t"], wproj=blk["proj"].w16t, w1=blk["fc1"].w16t, w2=blk["fc2"].w16t)
        return ops.gpt_block_desc(
            B, self.T, self.C, self.nh, eps=1e-5, attn_pdrop=p_attn, resid_pdrop=p_resid, rng_state=ctx.rng_state, rng_stream=sb,
            rng_stream_below=sb_below, below_colsum=below_colsum,
            ln1_w=blk["ln1"].w, ln1_b=blk["ln1"].b, bqkv=blk["bqkv"], bproj=blk["proj"].b,
            ln2_w=blk["ln2"].w, ln2_b=blk["ln2"].b, b1=blk["fc1"].b, b2=blk["fc2"].b, **w, **tensors)

    def _bwd_fused(self, ctx, g_y):
        """GPT.bwd with the row-local chain of every block in one launch (csrc/gpt_block.hip gpt_bwd_rows_kernel): per block the chain is
        dQ -> dK/dV -> rows(this block's qkv dgrad + ln1 backward | the block below's mlp / ln2 / proj dgrads)."""
        B = g_y.shape[0]
        T, C, nh, hs = self.T, self.C, self.nh, self.hs
        M = B * T
        bufs, nm = ctx.bufs, self.name
        p_embd, p_attn, p_resid = ctx.drop
        scale = 1.0 / math.sqrt(hs)
        nblk = len(self.blocks)
        # bf16 mode: the "dropped copy" is also where the stream gradient becomes a bf16 GEMM operand, so it exists without dropout too
        drop = p_resid > 0.0 or ctx.bf16
        sb_of = lambda i: self.stream_base + 1 + 3 * i
        f32, adt = torch.float32, ctx.adt   # the residual stream's gradient (G, G1) is fp32 in both modes
        G = bufs.get(nm + ".S.g", (nblk, M, C), f32)
        GD = bufs.get(nm + ".S.gdrop", (nblk, M, C), adt) if drop else None
        G1 = bufs.get(nm + ".S.g1", (nblk, M, C), f32)
        GD2 = bufs.get(nm + ".S.gdrop2", (nblk, M, C), adt) if drop else None
        GH = bufs.get(nm + ".S.gh", (nblk, M, 4 * C), adt)
        DQKV = bufs.get(nm + ".S.dqkv", (nblk, M, 3 * C), adt)
        nrow = M // ops.GPT_ROWS
        P1 = bufs.get(nm + ".S.part1", (nblk, nrow, 3, C), f32)
        P2 = bufs.get(nm + ".S.part2", (nblk, nrow, 3, C), f32)
        go = bufs.get(nm + ".go", (M, C), adt)
        g_tok = bufs.get(nm + ".g_tok", (M, C), f32)
        delta = bufs.get(nm + ".delta", (B, nh, T))
        side = []
        self.ln_f.bwd(ctx, g_y.view(M, C), out=G[nblk - 1], dropped=GD[nblk - 1] if drop else None, drop_p=p_resid,
                      rng_stream=sb_of(nblk - 1) + 2, colsum=self.blocks[nblk - 1]["fc2"].gb, defer=side)
        descs = []
        for i, blk in enumerate(self.blocks):
            x, a, qkv, o, lse, x1, a2, h = self.acts[i]
            descs.append(self._desc(
                blk, B, ctx, sb_of(i), sb_below=sb_of(i - 1) if i > 0 else 0, below_colsum=i > 0,
                weights="bwd16" if ctx.bf16 else "f32", x=x, mu1=blk["ln1"].saved[1], rs1=blk["ln1"].saved[2], x1=x1, mu2=blk["ln2"].saved[1], rs2=blk["ln2"].saved[2], h=h,
                g=G[i], gd=GD[i] if drop else None, gh=GH[i], g1=G1[i], gd2=GD2[i] if drop else None, go=go, dqkv=DQKV[i],
                g_below=G[i - 1] if i > 0 else g_tok, gd_below=GD[i - 1] if (drop and i > 0) else None, part_ln1=P1[i], part_ln2=P2[i]))
        ops.gpt_block_bwd_rows(None, descs[nblk - 1])
        pending = None
        for i in range(nblk - 1, -1, -1):
            blk = self.blocks[i]
            x, a, qkv, o, lse, x1, a2, h = self.acts[i]
            dqkv = DQKV[i]
            ops.attention_bwd(qkv[:, C:], qkv, qkv[:, 2 * C:], 3 * C, o, go, C, lse, delta, dqkv[:, C:], dqkv, dqkv[:, 2 * C:],
                              3 * C, B, T, nh, hs, scale, drop_p=p_attn, rng_state=ctx.rng_state, rng_stream=sb_of(i))
            if pending is not None:   # the block above's side work, now that this block's first chain kernel is captured
                self._offload_side(ctx, pending)
                pending = None
            ops.gpt_block_bwd_rows(descs[i], descs[i - 1] if i > 0 else None)
            gp, gp2 = (GD[i] if drop else G[i]), (GD2[i] if drop else G1[i])
            below_gb = self.blocks[i - 1]["fc2"].gb if i > 0 else None
            side += [
                lambda gp=gp, blk=blk, h=h: _dw(ctx, gp, h, blk["fc2"].gw),
                lambda gh=GH[i], blk=blk, a2=a2: _dw_db(ctx, gh, a2, blk["fc1"].gw, blk["fc1"].gb),
                lambda p=P2[i], blk=blk: _ln_finalize(ctx, p, nrow, C, blk["ln2"].gw, blk["ln2"].gb, blk["proj"].gb),
                lambda gp2=gp2, blk=blk, o=o: _dw(ctx, gp2, o, blk["proj"].gw),
                lambda dqkv=dqkv, blk=blk, a=a: _dw_db(ctx, dqkv, a, blk["g_wqkv"], blk["g_bqkv"]),
                lambda p=(P1[i] if i > 0 else P1[i].view(-1)[:nrow * 2 * C].view(nrow, 2, C)), blk=blk, cs=below_gb:
                    _ln_finalize(ctx, p, nrow, C, blk["ln1"].gw, blk["ln1"].gb, cs),
            ]
            work, side = side, []
            pending = (ctx.fork_point(), work)
        if pending is not None:
            self._offload_side(ctx, pending)
        ctx.rejoin()
        gtok = g_tok.view(B, T, C)
        ops.tokens_bwd(gtok, self.velocity, self.g_pos.view(T, C), self.vel.gw.view(C), self.vel.gb, p_embd, ctx.rng_state,
                       self.stream_base)
        return gtok

    def _offload_side(self, ctx, pending):
        """A block's side work (fork point, launch closures).  The narrow transformers are launch-bound on BOTH streams - per block
        8 kernels on the chain and ~14 on the side stream, 5-8 us each - so there the closures alternate between two side streams."""
        ev, work = pending
        if self.C <= SIDE_SPLIT_MAX_C and ctx.side2 is not None and len(work) > 1:
            ctx.offload_at(ev, lambda: [f() for f in work[0::2]])
            ctx.offload_at(ev, lambda: [f() for f in work[1::2]], second=True)
        else:
            ctx.offload_at(ev, lambda: [f() for f in work])

    def bwd(self, ctx, g_y):
        """g_y: [B,T,C] gradient of the GPT output.  Returns the token gradient (masked by the
        embedding dropout) to be spread back over the feature maps; writes all parameter grads.  Follows the path of the forward."""
        if self.path == "fold":
            raise RuntimeError("%s: no backward after a LayerNorm-folded (eval-mode) forward: it keeps no normalised tensor" % self.name)
        if self.path == "fused":
            return self._bwd_fused(ctx, g_y)
        B = g_y.shape[0]
        T, C, nh, hs = self.T, self.C, self.nh, self.hs
        M = B * T
        bufs, nm = ctx.bufs, self.name
        p_embd, p_attn, p_resid = ctx.drop
        scale = 1.0 / math.sqrt(hs)
        nblk = len(self.blocks)
        drop = p_resid > 0.0
        # the LayerNorm backward that produces a block's incoming gradient also writes its dropped copy (the residual
        # dropouts of the forward sit in GEMM epilogues; their masks are re-applied here without an extra pass)
        sb_of = lambda i: self.stream_base + 1 + 3 * i
        # Per-block gradient tensors, stacked over the blocks: G[i] = gradient arriving at block i's output, GD[i] its dropped copy
        # (what enters the MLP branch), G1 / GD2 the same for the attention branch, GH / DQKV the gradients of the hidden / qkv
        # activations.  The side stream reads them for the weight gradients, so they are per block and it may lag by any number
        # of blocks: one rejoin at the end of the transformer.
        adt, sdt = ctx.adt, torch.float32   # sdt: the residual stream's gradient is fp32 in both modes (see fwd)
        # bf16 mode: the "dropped copy" is also where the stream gradient becomes a bf16 GEMM operand, so it exists without dropout too
        drop = drop or ctx.bf16
        Wb = (lambda lin: lin.w16t) if ctx.bf16 else (lambda lin: lin.w)     # data-gradient operand of a Linear (bf16: the transposed shadow)
        G = bufs.get(nm + ".S.g", (nblk, M, C), sdt)
        GD = bufs.get(nm + ".S.gdrop", (nblk, M, C), adt) if drop else None
        G1 = bufs.get(nm + ".S.g1", (nblk, M, C), sdt)
        GD2 = bufs.get(nm + ".S.gdrop2", (nblk, M, C), adt) if drop else None
        GH = bufs.get(nm + ".S.gh", (nblk, M, 4 * C), adt)
        DQKV = bufs.get(nm + ".S.dqkv", (nblk, M, 3 * C), adt)
        # Side work - everything that only feeds the optimizer: weight / bias gradients, column sums, the LayerNorm row
        # reductions - is collected per block and forked to the side stream ONCE per block, and the fork is captured AFTER the
        # chain's next kernel (Ctx.offload_at): in a replayed graph every fork moves the continuation of the chain to another
        # hardware queue, and each such hop costs 10-16 us of idle time (profiles/r02c_graph_timeline.txt) - with a fork per
        # weight gradient and per LayerNorm reduction (7 per block) that was 0.3 ms per transformer.
        side = []
        pending = None
        # bf16 mode: the 17 LayerNorm backward passes leave their row reductions (weight / bias gradient, the consuming Linear's bias
        # gradient) to ONE launch at the end of this transformer (mmfn_layernorm_bwd_finalize_batched_f32) instead of one each on the
        # side streams.  Bit-identical either way; measured (3 interleaved runs each): bf16 step 17.14 -> 17.09 ms, fp32 31.40 -> 31.49
        # (there the launch at the tail costs more than the side streams gain) - hence by mode.
        fins = [] if (ctx.bf16 and ctx.side is not None) else None
        g = self.ln_f.bwd(ctx, g_y.view(M, C), out=G[nblk - 1], dropped=GD[nblk - 1] if drop else None, drop_p=p_resid,
                          rng_stream=sb_of(nblk - 1) + 2, colsum=self.blocks[nblk - 1]["fc2"].gb, defer=side, collect=fins)
        for i in range(nblk - 1, -1, -1):
            blk = self.blocks[i]
            sb = sb_of(i)
            x, a, qkv, o, lse, x1, a2, h = self.acts[i]
            # ---- MLP branch: x2 = x1 + drop(fc2(relu(fc1(ln2(x1)))))
            gp = GD[i] if drop else g
            side.append(lambda gp=gp, blk=blk, h=h: _dw(ctx, gp, h, blk["fc2"].gw))   # fc2.gb: from the LayerNorm backward
            gh = GH[i]
            ghpart = None
            if ctx.bf16:
                # the column sums of gh (= mlp.0's bias gradient) come out of this GEMM's epilogue as partial rows
                from . import ops16
                ghpart = bufs.get("%s.b%d.ghpart" % (nm, i), (ops16.max_stats_rows(M), 2, 4 * C), torch.float64)
                ops.linear_dx(gp, Wb(blk["fc2"]), out=gh, aux=h, ldaux=4 * C, stats=ghpart, stats_mode=1)
                ghrows = ops16.gemm_stats_rows(ops16.G16_NT, M, 4 * C, C)
            else:
                ops.linear_dx(gp, Wb(blk["fc2"]), out=gh, aux=h, ldaux=4 * C)
            if pending is not None:   # the previous block's side work, now that this block's first chain kernel is captured
                self._offload_side(ctx, pending)
                pending = None
            if ghpart is not None:
                side.append(lambda gh=gh, blk=blk, a2=a2, p=ghpart, r=ghrows: (ops16.colsum_partials(p, r, 4 * C, blk["fc1"].gb),
                                                                               _dw(ctx, gh, a2, blk["fc1"].gw)))
            else:
                side.append(lambda gh=gh, blk=blk, a2=a2: _dw_db(ctx, gh, a2, blk["fc1"].gw, blk["fc1"].gb))
            ga2 = bufs.get(nm + ".ga", (M, C), adt)
            ops.linear_dx(gh, Wb(blk["fc1"]), out=ga2)
            g1 = blk["ln2"].bwd(ctx, ga2, dres=g, out=G1[i], dropped=GD2[i] if drop else None, drop_p=p_resid,
                                rng_stream=sb + 1, colsum=blk["proj"].gb, defer=side, collect=fins)
            # ---- attention branch: x1 = x + drop(proj(att(ln1(x))))
            gp = GD2[i] if drop else g1
            side.append(lambda gp=gp, blk=blk, o=o: _dw(ctx, gp, o, blk["proj"].gw))   # proj.gb: from ln2's backward
            go = bufs.get(nm + ".go", (M, C), adt)
            ops.linear_dx(gp, Wb(blk["proj"]), out=go)
            dqkv = DQKV[i]
            delta = bufs.get(nm + ".delta", (B, nh, T))
            ops.attention_bwd(qkv[:, C:], qkv, qkv[:, 2 * C:], 3 * C, o, go, C, lse, delta, dqkv[:, C:], dqkv, dqkv[:, 2 * C:],
                              3 * C, B, T, nh, hs, scale, drop_p=p_attn, rng_state=ctx.rng_state, rng_stream=sb)
            side.append(lambda dqkv=dqkv, blk=blk, a=a: _dw_db(ctx, dqkv, a, blk["g_wqkv"], blk["g_bqkv"]))
            ga = bufs.get(nm + ".ga2", (M, C), adt)
            ops.linear_dx(dqkv, blk["wqkv16t"] if ctx.bf16 else blk["wqkv"], out=ga)
            g = blk["ln1"].bwd(ctx, ga, dres=g1, out=G[i - 1] if i > 0 else bufs.get(nm + ".g_tok", (M, C), sdt),
                               dropped=GD[i - 1] if (drop and i > 0) else None, drop_p=p_resid,
                               rng_stream=sb_of(i - 1) + 2, colsum=self.blocks[i - 1]["fc2"].gb if i > 0 else None, defer=side,
                               collect=fins)
            work, side = side, []
            pending = (ctx.fork_point(), work)   # enqueued after the next block's first kernel (Ctx.offload_at)
        if pending is not None:
            self._offload_side(ctx, pending)
        if fins:
            # keyed by the addresses the table holds (not by id(bufs): a dropped Buffers object's id can be reused, and a
            # reallocated gradient buffer moves the targets) - a stale table would write through dangling pointers
            key = tuple(0 if t is None else t.data_ptr() for f in fins for t in f[:4])
            tab = self._fin_tables.get(key)
            if tab is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("LayerNorm finalize table of %s first built during graph capture; run one eager step first" % nm)
                tab = self._fin_tables[key] = ops.layernorm_finalize_table([f[:4] for f in fins], g.device)
            ctx.offload(lambda: ops.layernorm_bwd_finalize_batched(tab, len(fins), fins[0][4], fins[0][5]))
        ctx.rejoin()
        gtok = g.view(B, T, C)
        ops.tokens_bwd(gtok, self.velocity, self.g_pos.view(T, C), self.vel.gw.view(C), self.vel.gb, p_embd, ctx.rng_state,
                       self.stream_base)
        return gtok


# ----------------------------------------------------------------------------- VectorNet
class VectorNet(object):
    """model_vec.py:326-416.  Only lane 0's fused token feeds the generator (:412), so everything
    after the lane attention runs on B rows; the constant pos_emb branch (fed zeros, :408) runs on
    a single row."""

    def __init__(self, name, layout, prefix, mod):
        self.name = name
        self.sub = []
        for i in range(3):
            p = "%s.lane_subgraph.layers.mlp_%d.mlp" % (prefix, i)
            self.sub.append((Linear(layout, p + ".0"), LayerNorm("%s.sub%d.ln" % (name, i), layout, p + ".1")))
        self.pe0, self.pe_ln, self.pe3 = (Linear(layout, prefix + ".pos_emb.0"), LayerNorm(name + ".pe.ln", layout, prefix + ".pos_emb.1"),
                                          Linear(layout, prefix + ".pos_emb.3"))
        self.qkv = Linear(layout, prefix + ".L2L.to_qkv", bias=False)
        self.to_out = Linear(layout, prefix + ".L2L.to_out.0")
        self.af0, self.af_ln, self.af3 = (Linear(layout, prefix + ".agent_fusion.0"), LayerNorm(name + ".af.ln", layout, prefix + ".agent_fusion.1"),
                                          Linear(layout, prefix + ".agent_fusion.3"))
        self.gen0, self.gen_ln, self.gen3 = (Linear(layout, prefix + ".generator.0"), LayerNorm(name + ".gen.ln", layout, prefix + ".generator.1"),
                                             Linear(layout, prefix + ".generator.3"))
        self.heads = mod.L2L.heads

    def fwd(self, ctx, lane, lane_num):
        """lane [B,L,n,5] f32 nodes (reference format) or pre-vectorised polylines [B,L,V,lane_channels] (perf-only
        64x19x8 variant, config.lane_channels = 8), lane_num int32 [B]  ->  map features NHWC [B,64,64,64]."""
        bufs, nm = ctx.bufs, self.name
        B, L, n, F = lane.shape
        cin = self.sub[0][0].w.shape[1]
        if F == 5 and cin == 7:
            V = n - 1
            R = B * L
            x = ops.lane_to_vector(lane, bufs.get(nm + ".vec", (R * V, 7)))
        elif F == cin:
            V, R = n, B * L
            x = lane.view(R * V, cin)
        else:
            raise ValueError("lane tensor [..., %d, %d] does not fit a VectorNet with lane_channels=%d" % (n, F, cin))
        self.sub_saved = []
        for i, (lin, ln) in enumerate(self.sub):
            pre = bufs.get("%s.sub%d.pre" % (nm, i), (R * V, 64))
            ops.linear_fwd(x, lin.w, lin.b, out=pre)
            y = ln.fwd(ctx, pre, ACT_RELU)
            last = i == len(self.sub) - 1
            out = bufs.get("%s.sub%d.cat" % (nm, i), (R, 128) if last else (R * V, 128))
            arg = bufs.get("%s.sub%d.arg" % (nm, i), (R, 64), torch.uint8)
            ops.polyline_pool_fwd(y, out, arg, R, V, 64, last)
            self.sub_saved.append((x, arg))
            x = out
        tok = x  # [R,128] lane tokens
        qkv = bufs.get(nm + ".qkv", (R, 384))
        ops.linear_fwd(tok, self.qkv.w, None, out=qkv)
        # Only lane 0's attended token feeds the encoder output (model_vec.py:412), so the lane attention runs for query 0
        # alone: O(L) instead of O(L^2), and any number of lanes (the fused attention kernels stop at 256 tokens)
        hd = 128 // self.heads
        att0 = bufs.get(nm + ".att0", (B, 128))
        prob = bufs.get(nm + ".prob", (B, self.heads, L))
        ops.lane0_attention_fwd(qkv, lane_num, B, L, self.heads, hd, hd ** -0.5, att0, prob)
        t0 = bufs.get(nm + ".t0", (B, 128))
        ops.gemm(att0, self.to_out.w, t0, B, 128, 128, 128, 128, 128, bias=self.to_out.b)
        # constant positional branch: pos_emb(zeros) = Linear(GELU(LN(bias0)))
        pe_pre = bufs.get(nm + ".pe.pre", (1, 64))
        zero2 = bufs.get(nm + ".zero2", (1, 2))
        ops.fill(zero2, 0.0)
        ops.linear_fwd(zero2, self.pe0.w, self.pe0.b, out=pe_pre)
        pe_act = self.pe_ln.fwd(ctx, pe_pre, ACT_GELU)
        pe = bufs.get(nm + ".pe", (1, 64))
        ops.linear_fwd(pe_act, self.pe3.w, self.pe3.b, out=pe)
        # agent_fusion.0 over cat([t0, pe]): split the [128,192] weight into its two column blocks
        cbias = bufs.get(nm + ".af.cbias", (1, 128))
        ops.gemm(pe, self.af0.w[:, 128:], cbias, 1, 128, 64, 64, 192, 128, bias=self.af0.b)
        af_pre = bufs.get(nm + ".af.pre", (B, 128))
        ops.gemm(t0, self.af0.w, af_pre, B, 128, 128, 128, 192, 128, bias=cbias.view(128))
        af_act = self.af_ln.fwd(ctx, af_pre, ACT_GELU)
        fused = bufs.get(nm + ".fused", (B, 128))
        ops.linear_fwd(af_act, self.af3.w, self.af3.b, out=fused)
        gen_pre = bufs.get(nm + ".gen.pre", (B, 64))
        ops.linear_fwd(fused, self.gen0.w, self.gen0.b, out=gen_pre)
        gen_act = self.gen_ln.fwd(ctx, gen_pre, ACT_GELU)
        nchw = bufs.get(nm + ".nchw", (B, 64 * 64 * 64))
        ops.linear_fwd(gen_act, self.gen3.w, self.gen3.b, out=nchw)
        out = bufs.get(nm + ".out", (B, 64, 64, 64), ctx.adt)   # (bf16 mode: VectorNet is fp32 inside, its map feature is an activation)
        ops.transpose(nchw, out, B, 64, 4096)  # "b (n d a)" -> NHWC [b, d, a, n]
        self.saved = (B, L, V, tok, qkv, att0, prob, lane_num, t0, pe, pe_act, af_act, fused, gen_act)
        return out

    def bwd(self, ctx, g_out):
        bufs, nm = ctx.bufs, self.name
        B, L, V, tok, qkv, att0, prob, lane_num, t0, pe, pe_act, af_act, fused, gen_act = self.saved
        R = B * L
        g_nchw = bufs.get(nm + ".g.nchw", (B, 64 * 64 * 64))
        ops.transpose(g_out.view(B, 4096, 64), g_nchw, B, 4096, 64)
        if not ctx.fz(self.gen3.gb):
            ops.colsum(g_nchw, self.gen3.gb)
        _dw(ctx, g_nchw, gen_act, self.gen3.gw)
        g_gen_act = ops.linear_dx(g_nchw, self.gen3.w, out=bufs.get(nm + ".g.gen_act", (B, 64)))
        g_gen_pre = self.gen_ln.bwd(ctx, g_gen_act)
        if not ctx.fz(self.gen0.gb):
            ops.colsum(g_gen_pre, self.gen0.gb)
        _dw(ctx, g_gen_pre, fused, self.gen0.gw)
        g_fused = ops.linear_dx(g_gen_pre, self.gen0.w, out=bufs.get(nm + ".g.fused", (B, 128)))
        if not ctx.fz(self.af3.gb):
            ops.colsum(g_fused, self.af3.gb)
        _dw(ctx, g_fused, af_act, self.af3.gw)
        g_af_act = ops.linear_dx(g_fused, self.af3.w, out=bufs.get(nm + ".g.af_act", (B, 128)))
        g_af_pre = self.af_ln.bwd(ctx, g_af_act)
        # agent_fusion.0: columns 0:128 act on t0, columns 128:192 on the constant pe row
        gsum = ops.colsum(g_af_pre, bufs.get(nm + ".g.afsum", (1, 128)).view(128)).view(1, 128)
        ops.axpby(self.af0.gb, gsum.view(128), 1.0, 0.0)
        ops.gemm(g_af_pre, t0, self.af0.gw, 128, 128, B, 128, 128, 192, a_mode=ops.A_COLMAJOR, b_mode=ops.B_KN)
        ops.gemm(gsum, pe, self.af0.gw[:, 128:], 128, 64, 1, 128, 64, 192, a_mode=ops.A_COLMAJOR, b_mode=ops.B_KN)
        g_t0 = bufs.get(nm + ".g.t0", (B, 128))
        ops.gemm(g_af_pre, self.af0.w, g_t0, B, 128, 128, 128, 192, 128, b_mode=ops.B_KN)
        g_pe = bufs.get(nm + ".g.pe", (1, 64))
        ops.gemm(gsum, self.af0.w[:, 128:], g_pe, 1, 64, 128, 128, 192, 64, b_mode=ops.B_KN)
        # pos_emb branch (single row; its first Linear sees a zero input -> exactly-zero weight grad)
        ops.axpby(self.pe3.gb, g_pe.view(64), 1.0, 0.0)
        _dw(ctx, g_pe, pe_act, self.pe3.gw)
        g_pe_act = ops.linear_dx(g_pe, self.pe3.w, out=bufs.get(nm + ".g.pe_act", (1, 64)))
        g_pe_pre = self.pe_ln.bwd(ctx, g_pe_act)
        ops.axpby(self.pe0.gb, g_pe_pre.view(64), 1.0, 0.0)
        ops.fill(self.pe0.gw, 0.0)
        # to_out on lane 0 only
        if not ctx.fz(self.to_out.gb):
            ops.colsum(g_t0, self.to_out.gb)
        ops.gemm(g_t0, att0, self.to_out.gw, 128, 128, B, 128, 128, 128, a_mode=ops.A_COLMAJOR, b_mode=ops.B_KN)
        g_att0 = bufs.get(nm + ".g.att0", (B, 128))
        ops.gemm(g_t0, self.to_out.w, g_att0, B, 128, 128, 128, 128, 128, b_mode=ops.B_KN)
        dqkv = bufs.get(nm + ".g.qkv", (R, 384))
        hd = 128 // self.heads
        ops.lane0_attention_bwd(qkv, prob, g_att0, lane_num, B, L, self.heads, hd, hd ** -0.5, dqkv)
        _dw(ctx, dqkv, tok, self.qkv.gw)
        g = ops.linear_dx(dqkv, self.qkv.w, out=bufs.get(nm + ".g.tok", (R, 128)))
        for i in range(len(self.sub) - 1, -1, -1):
            lin, ln = self.sub[i]
            x_in, arg = self.sub_saved[i]
            last = i == len(self.sub) - 1
            gy = ops.polyline_pool_bwd(g, arg, bufs.get("%s.g.sub%d.y" % (nm, i), (R * V, 64)), R, V, 64, last)
            g_pre = ln.bwd(ctx, gy)
            if not ctx.fz(lin.gb):
                ops.colsum(g_pre, lin.gb)
            _dw(ctx, g_pre, x_in, lin.gw)
            if i > 0:
                g = ops.linear_dx(g_pre, lin.w, out=bufs.get("%s.g.sub%d.x" % (nm, i), (R * V, 128)))



# ----------------------------------------------------------------------------- radar GAT
class RadarGAT(object):
    """model_rad.py:853-884 (SpGAT) with its two SpGraphAttentionLayer heads (:778-847).

    radar [B,81,5], adj [B,81,81] -> NHWC map [B,8,8,512] (log-softmax over channels).  Matrix products
    run on the (batched) MFMA GEMM; the (nhid == N == 81) coincidence that makes `Wh @ a` an [81,81]
    score matrix (config.py:53) is kept as is."""

    def __init__(self, name, layout, prefix, mod):
        self.name = name
        self.nh = mod.nheads
        if self.nh > 3:
            # head h draws its attention mask from stream_base + 1 + h; the sites after the heads use stream_base + 4, 5 and 6
            raise ValueError("RadarGAT numbers its dropout streams 901 + head and 904..906 for the later sites: nheads = %d would "
                             "give a head the mask stream of a later site (at most 3 heads)" % self.nh)
        self.alpha = mod.alpha
        self.p = mod.dropout
        self.W = [layout.w("%s.attention_%d.W" % (prefix, i)) for i in range(self.nh)]
        self.gW = [layout.g("%s.attention_%d.W" % (prefix, i)) for i in range(self.nh)]
        self.a = [layout.w("%s.attention_%d.a" % (prefix, i)) for i in range(self.nh)]
        self.ga = [layout.g("%s.attention_%d.a" % (prefix, i)) for i in range(self.nh)]
        self.m1 = Linear(layout, prefix + ".mlp_1.0")
        self.m2 = Linear(layout, prefix + ".mlp_2.0")
        self.stream_base = 900

    def _drop(self, ctx, t, tag, sid):
        p = self.p if ctx.training else 0.0
        if p <= 0.0:
            return t
        return ops.dropout_apply(t, ctx.bufs.get("%s.%s" % (self.name, tag), t.shape), p, ctx.rng_state, self.stream_base + sid)

    def fwd(self, ctx, radar, adj):
        bufs, nm = ctx.bufs, self.name
        B, N, Fin = radar.shape  # 81 nodes, 5 features
        H2 = self.W[0].shape[1]  # 162
        R = B * N
        p = self.p if ctx.training else 0.0
        x = self._drop(ctx, radar.view(R, Fin), "xd", 0)
        cat = bufs.get(nm + ".cat", (B, self.nh * N, H2))
        self.heads = []
        adj2 = adj.view(R, N)
        for h in range(self.nh):
            wh = bufs.get("%s.wh%d" % (nm, h), (R, H2))
            ops.gemm(x, self.W[h], wh, R, H2, Fin, Fin, H2, H2, b_mode=ops.B_KN)
            epre = bufs.get("%s.epre%d" % (nm, h), (R, N))
            ops.gemm(wh, self.a[h], epre, R, N, H2, H2, N, N, b_mode=ops.B_KN)
            prob = bufs.get("%s.p%d" % (nm, h), (R, N))
            att = bufs.get("%s.att%d" % (nm, h), (R, N))
            ops.gat_softmax_fwd(epre, adj2, self.alpha, prob, att, p, ctx.rng_state, self.stream_base + 1 + h)
            # h' = att @ Wh per sample, written into rows [h*81, (h+1)*81) of the concatenated tensor
            ops.gemm(att, wh, cat[:, h * N:], N, H2, N, N, H2, H2, b_mode=ops.B_KN, batch=B, strideA=N * N,
                     strideB=N * H2, strideC=self.nh * N * H2)
            self.heads.append((wh, epre, prob, att))
        n_cat = B * self.nh * N
        y1 = ops.elu_fwd(cat, bufs.get(nm + ".y1", cat.shape))                 # F.elu inside each head
        y1d = self._drop(ctx, y1, "y1d", 4)
        y2 = ops.elu_fwd(y1d, bufs.get(nm + ".y2", cat.shape))                # F.elu before mlp_1
        m1 = bufs.get(nm + ".m1", (n_cat, 256))
        ops.linear_fwd(y2.view(n_cat, H2), self.m1.w, self.m1.b, out=m1)
        m1d = self._drop(ctx, m1, "m1d", 5)
        m1t = bufs.get(nm + ".m1t", (B * 256, self.nh * N))
        ops.transpose(m1d, m1t, B, self.nh * N, 256)
        m2 = bufs.get(nm + ".m2", (B * 256, 128))
        ops.linear_fwd(m1t, self.m2.w, self.m2.b, out=m2)
        m2d = self._drop(ctx, m2, "m2d", 6)
        out = bufs.get(nm + ".out", (B, 8, 8, 512))
        ops.log_softmax_fwd(m2d, out, B * 64, 512, True)
        self.saved = (B, N, Fin, H2, x, adj2, y1, y2, m1t, out)
        if ctx.bf16:   # fp32 inside (81 points x 7 heads: nothing for the bf16 pipe), the radar feature joins the fusion as a bf16 activation
            return ops.cast_to_bf16(out, bufs.get(nm + ".out16", out.shape, ctx.adt))
        return out

    def bwd(self, ctx, g_out):
        bufs, nm = ctx.bufs, self.name
        B, N, Fin, H2, x, adj2, y1, y2, m1t, out = self.saved
        R = B * N
        n_cat = B * self.nh * N
        p = self.p if ctx.training else 0.0
        if g_out.dtype != torch.float32:
            g_out = ops.cast_to_f32(g_out, bufs.get(nm + ".g.out32", g_out.shape))
        g_m2 = ops.log_softmax_bwd(g_out, out, bufs.get(nm + ".g.m2", (B * 256, 128)), B * 64, 512, True)
        if p > 0.0:
            ops.dropout_apply(g_m2, g_m2, p, ctx.rng_state, self.stream_base + 6)
        if not ctx.fz(self.m2.gb):
            ops.colsum(g_m2, self.m2.gb)
        _dw(ctx, g_m2, m1t, self.m2.gw)
        g_m1t = ops.linear_dx(g_m2, self.m2.w, out=bufs.get(nm + ".g.m1t", m1t.shape))
        g_m1 = ops.transpose(g_m1t, bufs.get(nm + ".g.m1", (n_cat, 256)), B, 256, self.nh * N)
        if p > 0.0:
            ops.dropout_apply(g_m1, g_m1, p, ctx.rng_state, self.stream_base + 5)
        if not ctx.fz(self.m1.gb):
            ops.colsum(g_m1, self.m1.gb)
        _dw(ctx, g_m1, y2.view(n_cat, H2), self.m1.gw)
        g_y2 = ops.linear_dx(g_m1, self.m1.w, out=bufs.get(nm + ".g.y2", (n_cat, H2)))
        g_y1d = ops.elu_bwd(g_y2, y2, bufs.get(nm + ".g.y1d", (n_cat, H2)))
        if p > 0.0:
            ops.dropout_apply(g_y1d, g_y1d, p, ctx.rng_state, self.stream_base + 4)
        g_cat = ops.elu_bwd(g_y1d, y1, bufs.get(nm + ".g.cat", (B, self.nh * N, H2)))
        for h in range(self.nh):
            wh, epre, prob, att = self.heads[h]
            gh = g_cat[:, h * N:]  # [B, 81, 162] view, batch stride nh*N*H2
            # h' = att @ Wh:  d_att = g h'  Wh^T   ;   d_Wh = att^T g h'
            g_att = bufs.get("%s.g.att%d" % (nm, h), (R, N))
            ops.gemm(gh, wh, g_att, N, N, H2, H2, H2, N, b_mode=ops.B_NK, batch=B, strideA=self.nh * N * H2, strideB=N * H2,
                     strideC=N * N)
            g_wh = bufs.get("%s.g.wh%d" % (nm, h), (R, H2))
            ops.gemm(att, gh, g_wh, N, H2, N, N, H2, H2, a_mode=ops.A_COLMAJOR, b_mode=ops.B_KN, batch=B, strideA=N * N,
                     strideB=self.nh * N * H2, strideC=N * H2)
            g_epre = bufs.get("%s.g.epre%d" % (nm, h), (R, N))
            ops.gat_softmax_bwd(g_att, prob, epre, adj2, self.alpha, g_epre, p, ctx.rng_state, self.stream_base + 1 + h)
            # e_pre = Wh @ a
            ops.gemm(wh, g_epre, self.ga[h], H2, N, R, H2, N, N, a_mode=ops.A_COLMAJOR, b_mode=ops.B_KN)
            ops.gemm(g_epre, self.a[h], g_wh, R, H2, N, N, N, H2, b_mode=ops.B_NK, accum=True)
            # Wh = x @ W
            ops.gemm(x, g_wh, self.gW[h], Fin, H2, R, Fin, H2, H2, a_mode=ops.A_COLMAJOR, b_mode=ops.B_KN)


# ----------------------------------------------------------------------------- waypoint head
class Head(object):
    """model_vec.py:642-651,664-680: join MLP 512-256-128-64 (ReLU), GRUCell x pred_len, Linear(64,2)."""

    def __init__(self, layout, pred_len):
        self.join = [Linear(layout, "join.0"), Linear(layout, "join.2"), Linear(layout, "join.4")]
        self.w_ih, self.w_hh = layout.w("decoder.weight_ih"), layout.w("decoder.weight_hh")
        self.b_ih, self.b_hh = layout.w("decoder.bias_ih"), layout.w("decoder.bias_hh")
        self.out = Linear(layout, "output")
        self.grads = [layout.g("decoder.weight_ih"), layout.g("decoder.weight_hh"), layout.g("decoder.bias_ih"),
                      layout.g("decoder.bias_hh"), self.out.gw, self.out.gb]
        self.steps = pred_len
        # the objective of the training forwards (Engine.set_loss): MMFN_LOSS_* and the 16 device floats the launches with the
        # objective as a parameter read (None until a loss or a sample weight first needs them)
        self.loss_kind = 0
        self.loss_table = None
        self.plain = True      # L1 without horizon weights: the original launches, unless the batch carries sample weights
        self.lossy = False     # the last training forward with a loss ran the launches with the objective as a parameter

    def fwd(self, ctx, fused, target, gt=None, sample_weight=None):
        bufs = ctx.bufs
        B = fused.shape[0]
        self.xs = [fused]
        x = fused
        for i, lin in enumerate(self.join):
            y = bufs.get("head.j%d" % i, (B, lin.w.shape[0]))
            ops.linear_fwd(x, lin.w, lin.b, out=y, relu=True)
            self.xs.append(y)
            x = y
        S = self.steps
        pred = bufs.get("head.pred", (B, S, 2))
        train = ctx.training
        hs = bufs.get("head.hs", (B, S + 1, 64)) if train else None
        gates = bufs.get("head.gates", (B, S, 4, 64)) if train else None
        xin = bufs.get("head.xin", (B, S, 2)) if train else None
        lt = bufs.get("head.lt", (B,)) if gt is not None else None
        loss = bufs.get("head.loss", (1,)) if gt is not None else None
        # the objective applies to training forwards only: an eval forward's loss stays the mean L1 (validation keeps its meaning)
        lossy = train and gt is not None and (sample_weight is not None or not self.plain)
        if lossy:
            if self.loss_table is None:
                raise RuntimeError("the loss table is not allocated (Engine.set_loss / Engine._loss_table)")
            l1 = bufs.get("head.l1", (B,))
            ops.gru_head_fwd_loss(x, target, self.w_ih, self.w_hh, self.b_ih, self.b_hh, self.out.w, self.out.b, gt, pred, hs, gates,
                                  xin, lt, loss, self.loss_kind, self.loss_table, sample_weight, l1, S)
        else:
            ops.gru_head_fwd(x, target, self.w_ih, self.w_hh, self.b_ih, self.b_hh, self.out.w, self.out.b, gt, pred, hs, gates, xin,
                             lt, loss, S)
        if train and gt is not None:
            self.lossy = lossy
        self.saved = (pred, gt, hs, gates, xin, sample_weight if lossy else None, lossy)
        return pred, loss

    def bwd(self, ctx, dpred=None, gscale=None):
        bufs = ctx.bufs
        pred, gt, hs, gates, xin, sample_weight, lossy = self.saved
        B, S = pred.shape[0], self.steps
        if gscale is None:
            gscale = 1.0 / (B * S * 2)
        npart = ops.lib().mmfn_gru_head_part_floats()
        part = bufs.get("head.part", (B, npart))
        dz = bufs.get("head.dz", (B, 64))
        if lossy and dpred is None:   # (an external gradient - the autograd entry - takes the original launch)
            ops.gru_head_bwd_loss(pred, gt, gscale, self.w_ih, self.w_hh, self.out.w, hs, gates, xin, dz, part, self.loss_kind,
                                  self.loss_table, sample_weight, S)
        else:
            ops.gru_head_bwd(pred, gt, dpred, gscale, self.w_ih, self.w_hh, self.out.w, hs, gates, xin, dz, part, S)
        tot = ops.colsum(part, bufs.get("head.partsum", (npart,)))
        o = 0
        for gbuf in self.grads:
            n = gbuf.numel()
            if not ctx.fz(gbuf):
                ops.axpby(gbuf, tot[o:o + n], 1.0, 0.0)
            o += n
        # z0 = relu(join.4(.)): mask the GRU's gradient, then walk the MLP back; each dX GEMM applies
        # the ReLU mask of the layer below in its epilogue
        g = ops.relu_mask(dz, self.xs[-1], out=bufs.get("head.gz", dz.shape))
        for i in range(len(self.join) - 1, -1, -1):
            lin, x = self.join[i], self.xs[i]
            if not ctx.fz(lin.gb):
                ops.colsum(g, lin.gb)
            _dw(ctx, g, x, lin.gw)
            gx = bufs.get("head.gx%d" % i, x.shape)
            if i > 0:
                g = ops.linear_dx(g, lin.w, out=gx, aux=x, ldaux=x.shape[1])
            else:
                g = ops.linear_dx(g, lin.w, out=gx)
        return g


# ----------------------------------------------------------------------------- whole network
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _in_precision(fn):
    """Run an Engine method with its plain GEMMs in the engine's arithmetic (ops.precision)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        with ops.precision(self.gemm_dtype):
            return fn(self, *args, **kwargs)
    return wrapped


class Engine(object):
    """Forward / backward / optimizer step of one MMFN replica on one GPU.

    Orchestration restates Encoder.forward (model_vec.py:488-598; model_img.py:310-423) and
    MMFN.forward (model_vec.py:653-682).  seq_len = 1, n_views = 1 is the reference's configuration (config.py:6,11) and the
    tuned one; other values run the same kernels with more frames per sample: a sample's n_views * seq_len camera frames,
    seq_len LiDAR frames and seq_len map frames are batch entries of their branch and token groups of one sequence
    (self.frames / self.group_base; model_img.py:211-246, :410-423)."""

    def __init__(self, module, layout, variant):
        cfg = module.config
        self.module, self.layout, self.variant, self.cfg = module, layout, variant, cfg
        self.device = layout.device
        self.act_dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[getattr(cfg, "act_dtype", "f32")]
        S, V = int(cfg.seq_len), int(cfg.n_views)
        if S < 1 or V < 1:
            raise ValueError("seq_len and n_views must be >= 1, got %d and %d" % (S, V))
        if variant != "img" and S != 1:
            # the reference cannot either: its VectorNet / radar encoders emit one feature map per SAMPLE, which
            # GPT.forward's view(bz, seq_len, ...) rejects for seq_len > 1 (model_vec.py:223-229)
            raise NotImplementedError("seq_len > 1 exists for the image-map model only (the vector-map and radar encoders produce one "
                                      "frame per sample, as in the reference)")
        # frames per sample of each fused modality, in token order, and each modality's first 64-token group
        self.frames = [V * S, S, S]
        self.group_base = [0, V * S, (V + 1) * S]
        tokens = 64 * ((V + 2) * S + (1 if variant == "rad" else 0))
        if tokens > 384:
            raise NotImplementedError("(n_views + 2) * seq_len * 64%s = %d tokens: the attention kernels hold at most 384 keys" % (
                " + 64" if variant == "rad" else "", tokens))
        if self.act_dtype == torch.bfloat16 and tokens > 256:
            raise NotImplementedError("the bf16 training mode's attention kernels stage K and V of one head in LDS: at most 256 tokens, got %d" % tokens)
        if self.device.type != "cuda":
            raise ops._lib.MMFNLibraryError("the MMFN HIP path needs a GPU device (got %s); there is no CPU fallback" % self.device)
        enc = module.encoder
        self.img = ResNetTrunk("img", layout, "encoder.image_encoder.features", enc.image_encoder.features)
        self.lid = ResNetTrunk("lid", layout, "encoder.lidar_encoder._model", enc.lidar_encoder._model)
        if variant == "img":
            self.map = ResNetTrunk("map", layout, "encoder.img_map_encoder.features", enc.img_map_encoder.features)
            self.vec = None
        else:
            self.map = ResNetTrunk("map", layout, "encoder.img_map_encoder.features", enc.img_map_encoder.features,
                                   with_stem=False, first_layer=2)
            self.vec = VectorNet("vec", layout, "encoder.vectornet_encoder", enc.vectornet_encoder)
        self.rad = RadarGAT("rad", layout, "encoder.radar_encoder", enc.radar_encoder) if variant == "rad" else None
        self.gpts = [GPT("gpt%d" % (i + 1), layout, "encoder.transformer%d" % (i + 1), getattr(enc, "transformer%d" % (i + 1)),
                         cfg, 100 * (i + 1)) for i in range(4)]
        for i, g in enumerate(self.gpts):
            g.frames = self.frames + ([1] if (variant == "rad" and i == 3) else [])
            if g.T != 64 * sum(g.frames):
                raise ValueError("%s.pos_emb holds %d tokens; seq_len %d / n_views %d need %d (config changed after the module was built?)"
                                 % (g.name, g.T, S, V, 64 * sum(g.frames)))
        self.head = Head(layout, cfg.pred_len)
        self.bufs = {}
        dev = self.device
        self.rng_state = torch.tensor([0x5EED, 0], dtype=torch.int64, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.norm_mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=dev)
        self.norm_inv_std = torch.tensor([1.0 / s for s in IMAGENET_STD], dtype=torch.float32, device=dev)
        ops.norm_workspace(dev)
        ops.workspace(64 << 20, dev)
        # The three encoder branches (camera ResNet-34, LiDAR ResNet-18, map branch) only meet at the four
        # fusion transformers.  Between those points they run on separate HIP streams, so the many small
        # kernels of the deep stages (M = 2048..8192 rows at B = 32) overlap each other's tails and launch
        # gaps; captured into the hipGraph this becomes a fork/join DAG.
        self.side = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        self.multi_stream = True
        self._recorder = None   # mmfn_amd.graphs.Recorder while a capture is running
        self.folded = {}        # ConvBN name -> (BatchNorm-folded filter, shift), see fold_batchnorm()
        # "f32" (parity path) or "bf16": bf16 MFMA operands with fp32 accumulation for the Linear / Winograd GEMMs
        self.gemm_dtype = getattr(cfg, "gemm_dtype", "f32")
        if self.act_dtype == torch.bfloat16:
            self.gemm_dtype = "f32"   # the fp32 islands of the bf16 mode (stems, VectorNet, head) are plain fp32
            self._build_shadows()
        self.ln_fold_table = None   # the LayerNorm fold of the fp32 eval forwards (GPT.fwd); None = never fold
        if self.act_dtype == torch.float32:
            self._build_ln_fold()
        self.wino_layers = {}     # ConvBN name -> (filter storage, transformed-filter buffer): filled by the first training forward
        self.wino_table = None
        self.opt_group_of = None
        self.opt_hyper = torch.zeros(16, 8, dtype=torch.float32, device=dev)
        self._hyper_host = None
        self._hyper_pinned, self._hyper_slot = None, 0
        self.opt_amsgrad = ()       # per optimizer group: amsgrad (set_amsgrad); the flags travel in the last column of opt_hyper
        self._hyper_flags = ()      # ... as set_hyper last wrote them: the AdamW launch follows the table
        self.opt_kind = "adamw"     # the update rule of the optimizer launch (set_optimizer): "adamw" | "sgd"
        self.loss = None            # the objective of the training forwards (set_loss): None = the reference's mean L1
        # gradient accumulation (accumulate_step) and global-norm clipping: allocated on first use only
        self.grad_acc = None        # fp32 [0, tail): the sum of the pending micro-steps' gradients
        self.accum_pending = 0      # micro-steps in grad_acc (host count: it picks the 1 / (k * world) of the final step)
        self._norm = None           # partials table, its slots, and the device (norm, coef) pair
        self._tiling_checked = False
        self.average = None         # averaging.AveragedMMFN updated inside every optimizer step's AdamW launch (attach_average)
        self.nonfinite_guard = False   # set_nonfinite_guard: skip an optimizer step whose gradient norm is not finite
        self._guard = None          # its device flag, skip counter and BatchNorm shadows (allocated when first armed)
        self._stats_tab = None      # tensor_stats: the device table of the layout's tensors
        # frozen parameters (requires_grad = False), see trainable_mask()
        self._mask_flags = None     # the tuple of flags the state below was built for
        self._mask_held = 0         # > 0 inside mask_held(): the flags were read at the entry of the running step
        self.frozen = frozenset()   # frozen names of the trained range
        self._fz = frozenset()      # data pointers of their gradient views (a packed k/q/v window: all three frozen)
        self._plan = None           # which sub-backwards still run (None: everything, nothing is frozen)
        self._fill_tabs = {}        # readiness group -> fill_ranges table of the frozen ranges a launch may still write
        self._filled = set()        # ... and the groups zeroed so far in the running backward
        self._mask_table = None     # (optimizer group table it was built from, effective table with 255 over frozen float4s)
        self.never_stepped = None   # names frozen at every optimizer step so far (None: no step yet): FusedAdamW.state_dict
        # per-tensor AdamW step counts (params.StepClasses): one device counter per step class, read by the AdamW launch with
        # step classes once a class that steps no longer carries step_count; until then step_count serves everybody
        self.classes = layout.step_classes
        n_trained = max(len(self.classes.names), 1)   # (a class holds at least one tensor)
        self._class_steps = torch.zeros(n_trained, dtype=torch.int64, device=dev)
        self._class_active = torch.ones(n_trained, dtype=torch.uint8, device=dev)
        self._row_table = None      # (optimizer group table, classes.epoch, device row table, host rows)
        self._class_index = None    # (classes.epoch, device class index per trained tensor): tensor_steps
        if not self.classes.stepped and any(self.classes.values):   # counts loaded before the engine existed
            self.set_tensor_steps(self.classes.host_steps(), step_count=max(self.classes.values))
        self.n_lanes = int(os.environ.get("MMFN_BRANCH_LANES", "3"))
        self.offload_wgrad = True   # transformer weight / bias gradients on the side stream (worth 3.9 ms per step)

    # ------------------------------------------------------------------ frozen parameters
    def trainable_mask(self):
        """The parameters' requires_grad flags (a tuple, named_parameters() order), read at the entry of every step, backward and
        optimizer step, by the autograd bridge and at every capture and replay.  The flags are the only source: when they differ
        from the last read, the state derived from them is rebuilt (_install_mask) - outside a capture, and not while micro-steps
        are pending."""
        if self._mask_held:   # read at the entry of the running step (mask_held): one read of all flags per step
            return self._mask_flags
        flags = self.layout.trainable_flags()
        if flags != self._mask_flags:
            self._install_mask(flags)
        return flags

    @contextlib.contextmanager
    def mask_held(self):
        """Read the flags once and hold them for the block: the entry points inside (backward, optimizer_step, a replay) then
        use this read instead of one each.  train_step / accumulate_step and the trainer's step wrap themselves in it."""
        flags = self.trainable_mask()
        self._mask_held += 1
        try:
            yield flags
        finally:
            self._mask_held -= 1

    def fz(self, *grads):
        """True when every one of these gradient views belongs to a frozen parameter."""
        f = self._fz
        if not f:
            return False
        for g in grads:
            if g.data_ptr() not in f:
                return False
        return True

    def _install_mask(self, flags):
        L = self.layout
        frozen = L.frozen_names(flags)
        if frozen == self.frozen:   # (the first read with nothing frozen, or only never-trained tail tensors changed)
            self._mask_flags = flags
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("requires_grad flags changed inside a hipGraph capture")
        if self.accum_pending:
            raise RuntimeError("requires_grad flags changed while %d accumulated micro-step(s) are pending: finish them with "
                               "train_step() or drop them with discard_accumulated() first" % self.accum_pending)
        self._mask_flags, self.frozen = flags, frozen
        L.frozen = frozen
        self._mask_table = None
        self._fill_tabs = {}
        self._install_classes(self.classes.install(frozen))
        if not frozen:
            self._fz, self._plan = frozenset(), None
            return
        # gradient views by pointer; the packed k / q / v windows start at key.*: frozen as a window only when all three are
        ptrs = set()
        for n in frozen:
            if ".attn.key." in n and not all(n.replace(".key.", k) in frozen for k in (".query.", ".value.")):
                continue
            ptrs.add(L.g(n).data_ptr())
        self._fz = frozenset(ptrs)
        live = [n for n in L.offsets if n not in L.unused and n not in frozen]
        has = lambda *keys: any(all(k in n for k in keys) for n in live)
        trunk_keys = ("image_encoder.", "lidar_encoder.", "img_map_encoder.")
        layer = [[has(t, ".layer%d." % li) for li in range(5)] for t in trunk_keys]           # [m][li], li 1..4
        first = [any(t in n and ".layer" not in n for n in live) or layer[m][1] for m, t in enumerate(trunk_keys)]   # stem + layer1
        vec, rad = has("vectornet_encoder."), has("radar_encoder.")
        if self.variant != "img":
            first[2] = vec
        gpt = [has("transformer%d." % (i + 1)) for i in range(4)]
        act, below = [], False    # act[s]: something trainable in transformer s+1 or anywhere below it in the backward
        for s in range(4):
            below = below or gpt[s] or (s == 3 and rad) or any(first[m] if s == 0 else layer[m][s + 1] for m in range(3))
            act.append(below)
        self._plan = {"gpt": act, "rad": rad, "tail": first,
                      "layer": [[s > 0 and (act[s - 1] or layer[m][s + 1]) for m in range(3)] for s in range(4)]}
        # frozen ranges inside a sub-backward that this plan skips as a whole are written by no launch any more: zeroed once, here.
        # Every other frozen range is zeroed once per backward, per readiness group, in front of the group's hook (_ready):
        # byproducts of launches that run unchanged (BatchNorm / LayerNorm sums, one of a packed window, ...) and, deliberately,
        # also the ranges whose single launch is pruned (ctx.fz) - which launch writes which tensor is known only where the
        # launch is issued, and a second list of it here could go stale without any test noticing
        skipped = []
        for s in range(4):
            if not act[s]:
                skipped.append(("transformer%d." % (s + 1),))
            for m, t in enumerate(trunk_keys):
                if s > 0 and not self._plan["layer"][s][m]:
                    skipped.append((t, ".layer%d." % (s + 1)))
        for m, t in enumerate(trunk_keys):
            if not first[m] and not (m == 2 and self.variant != "img"):
                skipped += [(t, ".layer1."), (t, "stem")]
        if self.vec is not None and not vec:
            skipped.append(("vectornet_encoder.",))
        if self.rad is not None and not rad:
            skipped.append(("radar_encoder.",))

        def clean(n):
            for keys in skipped:
                if keys[-1] == "stem":
                    if keys[0] in n and ".layer" not in n:
                        return True
                elif all(k in n for k in keys):
                    return True
            return False

        dirty = {}
        for n in frozen:
            if not clean(n):
                dirty.setdefault((L.stage_of(n), L.GROUPS[L.group_of(n)]), []).append(n)
        self._fill_tabs = {key: ops.fill_ranges_table(L.merged_ranges(names), self.device) for key, names in dirty.items()}
        ops.fill_ranges(L.grads, ops.fill_ranges_table(L.merged_ranges(frozen), self.device))

    def _group_table(self, n_groups):
        """The AdamW launch's group table while something is frozen: 255 over frozen float4s, elsewhere what the unmasked launch
        reads - the optimizer's ids when the step has several hyper rows, zeros when it has one (a step with one row runs
        everything as group 0 whatever table an optimizer installed earlier)."""
        ids = self.opt_group_of if n_groups > 1 else None
        if self._mask_table is None or self._mask_table[0] is not ids:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the optimizer's group table changed inside a hipGraph capture")
            self._mask_table = (ids, self.layout.group_table(self.frozen, ids).to(self.device))
        return self._mask_table[1]

    # ------------------------------------------------------------------ per-tensor step counts (params.StepClasses)
    def _install_classes(self, splits=()):
        """The device side of a change of the step classes (new flags, set_tensor_steps), outside a capture: a class split off
        another one gets a copy of its counter, every class that still carries step_count gets that value (its slot is not
        advanced while the shared counter serves all classes that step), and the active bytes follow the flags."""
        C = self.classes
        dev = self.device
        if splits:
            new, src = (torch.tensor(x, dtype=torch.int64, device=dev) for x in zip(*splits))
            self._class_steps[new] = self._class_steps[src]
        synced = [c for c in range(C.n_classes) if C.synced[c]]
        if synced:
            self._class_steps[torch.tensor(synced, dtype=torch.int64, device=dev)] = self.step_count
        active = torch.zeros(self._class_active.numel(), dtype=torch.uint8)
        active[:C.n_classes] = torch.tensor(C.active, dtype=torch.uint8)
        self._class_active.copy_(active)
        self._row_table = None

    def _rows(self, n_groups):
        """(device row table, host rows) of the AdamW launch with step classes for the installed flags and the optimizer's groups
        (one row of hyper-parameters: everything is group 0, as in _group_table).  Built outside a capture."""
        ids = self.opt_group_of if n_groups > 1 else None
        C = self.classes
        if self._row_table is None or self._row_table[0] is not ids or self._row_table[1] != C.epoch:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the optimizer's group table or the step classes changed inside a hipGraph capture")
            tab, rows = C.row_table(self.layout, self.frozen, ids)
            self._row_table = (ids, C.epoch, tab.to(self.device), rows)
        return self._row_table[2], self._row_table[3]

    def _advance_steps(self, ok=None):
        """step_count += 1, and every active class counter with it once the classes have their own (behind the guard's flag)."""
        ops.step_advance(self.step_count, ok=ok)
        if not self.classes.uniform():
            ops.class_steps_advance(self._class_steps, self._class_active, self.classes.n_classes, ok=ok)

    def tensor_steps(self):
        """int64 CPU tensor: the AdamW step count of every trained tensor, in layout order (classes.names) - what
        torch.optim.AdamW holds in state[p]["step"].  One small device-to-host copy."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("tensor_steps() inside a hipGraph capture")
        C = self.classes
        if self._class_index is None or self._class_index[0] != (C.epoch, tuple(C.synced)):
            self._class_index = ((C.epoch, tuple(C.synced)), torch.tensor(C.cls, dtype=torch.int64, device=self.device),
                                 torch.tensor(C.synced, dtype=torch.bool, device=self.device))
        _, cls, synced = self._class_index
        per_class = torch.where(synced, self.step_count, self._class_steps[:C.n_classes])
        return per_class[cls].cpu()

    def set_tensor_steps(self, steps, step_count=None):
        """Set every trained tensor's step count (layout order, as tensor_steps() returns them); the classes are rebuilt from the
        distinct values.  step_count: the count of optimizer steps taken (None: it stays what it is)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_tensor_steps() inside a hipGraph capture")
        steps = [int(s) for s in (steps.tolist() if isinstance(steps, torch.Tensor) else steps)]
        if step_count is None:
            step_count = int(self.step_count.item())
        C = self.classes
        C.set_steps(steps, step_count)
        self.step_count.fill_(int(step_count))
        self._class_steps.zero_()
        self._class_steps[:C.n_classes] = torch.tensor(C.values, dtype=torch.int64, device=self.device)
        self._install_classes(C.install(self.frozen))
        self._class_index = None

    # ------------------------------------------------------------------ LayerNorm folded into the Linear behind it (fp32 path)
    def ln_fold_now(self, training):
        return self.ln_fold_table is not None and not training

    def _build_ln_fold(self):
        """Per transformer block: (Wqkv . diag(gamma1), c1, c2) and (W_mlp0 . diag(gamma2), c1, c2) for MMFN_EPI_LN_FOLD, refreshed by
        one grouped launch per forward (ops.ln_fold_weights): the weights change at every optimizer step."""
        dev, entries = self.device, []
        for gpt in self.gpts:
            C = gpt.C
            for blk in gpt.blocks:
                mk = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
                f = (mk(3 * C, C), mk(3 * C), mk(3 * C), mk(4 * C, C), mk(4 * C), mk(4 * C))
                blk["fold"] = f
                entries.append((blk["wqkv"], blk["ln1"].w, blk["ln1"].b, blk["bqkv"], f[0], f[1], f[2]))
                entries.append((blk["fc1"].w, blk["ln2"].w, blk["ln2"].b, blk["fc1"].b, f[3], f[4], f[5]))
        self.ln_fold_table = ops.make_ln_fold_table(entries, dev)

    # ------------------------------------------------------------------ bf16 weight shadows
    def _build_shadows(self):
        """bf16 mode: every GEMM weight has a bf16 shadow at the same offset of layout.params16 (forward operand) and, where a
        data gradient reads it, a transposed shadow ([in, out] / [Cin, taps, Cout]) in one extra flat buffer; both are
        re-derived from the fp32 master weights once per step (refresh_shadows: two launches)."""
        L = self.layout
        L.make_shadows()
        entries = []

        def want(src, shape_t):
            n = src.numel()
            entries.append((src, n, shape_t))

        trunks = [self.img, self.lid, self.map]
        convs = [cb for t in trunks for cb in t.convbns() if cb.w.shape[3] % 64 == 0]   # all but the 7x7 stems
        for cb in convs:
            cb.w16 = L.w16(cb.conv_name + ".weight")
            Co, KH, KW, Ci = cb.w.shape
            want(cb.w.view(Co, KH * KW, Ci), (Ci, KH, KW, Co))
        lins = []
        for gpt in self.gpts:
            for blk in gpt.blocks:
                C = gpt.C
                blk["wqkv16"] = L.packed16(blk["wqkv_name"], 3 * C, C)
                want(blk["wqkv"], (C, 3 * C))
                for k in ("proj", "fc1", "fc2"):
                    lin = blk[k]
                    lin.w16 = L.w16(lin.name)
                    want(lin.w, (lin.w.shape[1], lin.w.shape[0]))
                    lins.append(lin)
        total = sum((n + 7) // 8 * 8 for _, n, _ in entries)
        self.shadow_t = torch.zeros(total, dtype=torch.bfloat16, device=self.device)
        off, pairs, views = 0, [], []
        for src, n, shape_t in entries:
            dst = self.shadow_t[off:off + n]
            pairs.append((src, dst))
            views.append(dst.view(shape_t))
            off += (n + 7) // 8 * 8
        it = iter(views)
        for cb in convs:
            cb.w16t = next(it)
        for gpt in self.gpts:
            for blk in gpt.blocks:
                blk["wqkv16t"] = next(it)
                for k in ("proj", "fc1", "fc2"):
                    blk[k].w16t = next(it)
        self.shadow_table = ops.make_shadow_table(pairs, self.device)
        self.refresh_shadows()

    def refresh_shadows(self):
        """fp32 master weights -> bf16 operands (same offsets) + transposed copies.  Part of every bf16-mode forward: the weights
        change at every optimizer step, and a captured step must not depend on host-side bookkeeping."""
        L = self.layout
        ops.cast_to_bf16(L.params, L.params16)
        ops.shadow_transpose(*self.shadow_table)

    # ------------------------------------------------------------------ inputs
    def _bufs_for(self, B):
        b = self.bufs.get(B)
        if b is None:
            b = Buffers(self.device)
            self.bufs[B] = b
        return b

    def _ctx(self, B, training):
        cfg = self.cfg
        side = self.side[0] if (self.multi_stream and self.offload_wgrad and training) else None
        ctx = Ctx(self._bufs_for(B), training, (cfg.embd_pdrop, cfg.attn_pdrop, cfg.resid_pdrop), self.rng_state, side, engine=self)
        ctx.side2 = self.side[1] if side is not None else None
        return ctx

    def _ingest(self, ctx, inp):
        """inp: dict of device tensors -> NHWC network inputs."""
        bufs = ctx.bufs
        if "rgb_u8" in inp:
            rgb = inp["rgb_u8"]
            B = rgb.shape[0]
            img = ops.ingest_rgb_u8(rgb, bufs.get("in.img", (B, 256, 256, 3)))
        else:
            x = inp["image"]
            B = x.shape[0]
            img = ops.nchw_to_nhwc(x, bufs.get("in.img", (B, x.shape[2], x.shape[3], 3)), self.norm_mean, self.norm_inv_std)
        if "lidar_pts" in inp:
            lid = ops.lidar_splat(inp["lidar_pts"], bufs.get("in.lid", (inp["lidar_pts"].shape[0], 256, 256, 2)),
                                  flip_y=bool(inp.get("lidar_flip_y", False)))
        else:
            x = inp["lidar"]
            lid = ops.nchw_to_nhwc(x, bufs.get("in.lid", (x.shape[0], x.shape[2], x.shape[3], x.shape[1])))
        mp = None
        if self.variant == "img":
            x = inp["map"]
            mp = ops.nchw_to_nhwc(x, bufs.get("in.map", (x.shape[0], x.shape[2], x.shape[3], 3)))  # NOT normalised (model_img.py:337)
        return img, lid, mp

    # ------------------------------------------------------------------ branch concurrency
    def _branches(self, fns):
        """Run fns[0] on the current stream and fns[1:] on the side streams, fork/join with events."""
        if not self.multi_stream:
            return [f() for f in fns]
        main = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(main)
        outs = [None] * len(fns)
        if self.n_lanes == 2:
            # two lanes: the camera ResNet-34 alone on the main stream, LiDAR ResNet-18 + map branch back to back on
            # the side stream.  Which lane count wins depends on the kernel mix: with the implicit-GEMM convolutions
            # (few, chip-filling launches) two lanes beat three by 3 %; with the Winograd path (many small streaming
            # transforms between the GEMMs) three lanes beat two by 3 %
            st = self.side[0]
            st.wait_event(fork)
            with torch.cuda.stream(st), ops.lane(1):
                for i in range(1, len(fns)):
                    outs[i] = fns[i]()
            outs[0] = fns[0]()
            done = torch.cuda.Event()
            done.record(st)
            main.wait_event(done)
            return outs
        for i, f in enumerate(fns[1:]):
            st = self.side[i]
            st.wait_event(fork)
            with torch.cuda.stream(st), ops.lane(i + 1):
                outs[i + 1] = f()
        outs[0] = fns[0]()
        for i in range(len(fns) - 1):
            done = torch.cuda.Event()
            done.record(self.side[i])
            main.wait_event(done)
        return outs

    # ------------------------------------------------------------------ forward / backward
    def fold_batchnorm(self):
        """(Re)compute the BatchNorm-folded filters / shifts of every convolution from the current weights and running
        statistics, for eval forwards with folded=True.  The caller owns freshness: call it again after the weights or the
        running statistics change (DrivingSession does at construction and in refresh())."""
        for trunk in (self.img, self.lid, self.map):
            for cb in trunk.convbns():
                ent = self.folded.get(cb.name)
                if ent is None:
                    ent = (torch.empty_like(cb.w), torch.empty(cb.cout, dtype=torch.float32, device=self.device),
                           torch.empty(cb.w.shape, dtype=torch.bfloat16, device=self.device) if self.act_dtype == torch.bfloat16 else None)
                    self.folded[cb.name] = ent
                ops.bn_fold(cb.w, cb.bn_w, cb.bn_b, cb.bn.running_mean, cb.bn.running_var, cb.bn.eps, ent[0], ent[1])
                if ent[2] is not None:   # bf16 mode: the folded filter's shadow (the fold itself stays fp32: w * s is rounded once)
                    ops.cast_to_bf16(ent[0], ent[2])

    @_in_precision
    def forward(self, inp, training, gt=None, folded=False):
        B = inp["target_point"].shape[0]
        ctx = self._ctx(B, training)
        if folded:
            if training or not self.folded:
                raise ValueError("folded=True is an eval-mode option and needs Engine.fold_batchnorm() first")
            ctx.folded = True
        self._last = (ctx, B)
        if ctx.bf16:
            self.refresh_shadows()
        if self.ln_fold_now(training) and ops.current_precision() == "f32":
            ops.ln_fold_weights(*self.ln_fold_table)
        img, lid, mp = self._ingest(ctx, inp)
        vel = inp["velocity"]
        trunks = [self.img, self.lid, self.map]

        if training and self.wino_layers:
            # every Winograd filter transform of the step in one launch (the layers registered themselves in an earlier
            # forward); it runs at the head of the shortest branch, the consumers (layer2 and deeper) come after the first
            # fusion transformer, where all branches have joined
            if self.wino_table is None and not torch.cuda.is_current_stream_capturing():
                # two launches: the filters of layer1 (consumed inside the first fork, by lanes that run beside the lane that
                # would transform them: they go first, on the main stream, a few microseconds) and all the others
                early = [v for k, v in self.wino_layers.items() if ".l1." in k]
                late = [v for k, v in self.wino_layers.items() if ".l1." not in k]
                self.wino_table = (ops.make_wino_group_table(early, self.device) if early else None,
                                   ops.make_wino_group_table(late, self.device) if late else None, frozenset(self.wino_layers))
            table = self.wino_table   # a layer registering during this forward resets self.wino_table: keep using this one
            ctx.wino_ready = table is not None
            if ctx.wino_ready:
                ctx.wino_names = table[2]
                if table[0] is not None:
                    ops.wino_weight_group(*table[0])
        else:
            table = None

        def map_stage1():
            if ctx.wino_ready and table[1] is not None:
                ops.wino_weight_group(*table[1])
            if self.variant == "img":
                return self.map.layer_fwd(ctx, 1, self.map.stem_fwd(ctx, mp))
            return self.vec.fwd(ctx, inp["lane"], inp["lane_num"])

        feats = self._branches([lambda: self.img.layer_fwd(ctx, 1, self.img.stem_fwd(ctx, img)),
                                lambda: self.lid.layer_fwd(ctx, 1, self.lid.stem_fwd(ctx, lid)),
                                map_stage1])
        self.taps = {"stage1": tuple(feats)}
        self.pre_add = []
        tok = None
        # token groups: the modality's first 64-token group and its frames per sample (radar: one frame after the others)
        frames, base = self.frames + [1], self.group_base + [sum(self.frames)]
        for s in range(4):
            if s > 0:
                # per branch: add the previous scale's fusion output, then the next ResNet stage
                prev, ptok = feats, tok

                def stage(m, prev=prev, ptok=ptok, s=s):
                    f = ops.upsample_add_fwd(prev[m], ptok, ctx.bufs.get("fuse%d.%d" % (s - 1, m), prev[m].shape, prev[m].dtype),
                                             base[m], frames[m])
                    return trunks[m].layer_fwd(ctx, s + 1, f)

                feats = self._branches([lambda m=m: stage(m) for m in range(3)])
            if s == 3 and self.rad is not None:  # radar joins only the deepest fusion (model_rad.py:585-593)
                feats = feats + [self.rad.fwd(ctx, inp["radar"], inp["radar_adj"])]
            tok = self.gpts[s].fwd(ctx, feats, vel)
            self.taps["gpt%d" % (s + 1)] = tok
            self.pre_add.append(feats)
        feats = [ops.upsample_add_fwd(f, tok, ctx.bufs.get("fuse3.%d" % m, f.shape, f.dtype), base[m], frames[m]) for m, f in enumerate(feats)]
        fused = ops.gap_sum_fwd(feats, ctx.bufs.get("fused", (B, 512)), frames=frames[:len(feats)])
        self.taps["fused"] = fused
        sw = inp.get("sample_weight") if training and gt is not None else None
        if sw is not None:
            if sw.dtype != torch.float32 or tuple(sw.shape) != (B,) or not sw.is_contiguous():
                raise ValueError("inp['sample_weight'] must be a contiguous float32 tensor of shape [%d], got %s %s" % (
                    B, sw.dtype, tuple(sw.shape)))
            self._loss_table()
        pred, loss = self.head.fwd(ctx, fused, inp["target_point"], gt, sw)
        return pred, loss

    def backward(self, dpred=None, gscale=None, on_stage=None, on_ready=None):
        """Backward of the last training forward.  dpred None => gradient of the forward's own loss (the mean L1, or what set_loss chose).
        on_stage(i) is called as soon as every gradient of backward stage i (params.FlatLayout.stage_of)
        has been written, so a data-parallel wrapper can start reducing that bucket.
        on_ready((stage, group)) is the finer hook: called - ON THE STREAM THAT WROTE THEM, which inside the branch lanes is a
        side stream - as soon as the gradients of one readiness group of a stage (params.FlatLayout.group_ranges: "head",
        "gpt", "vec", "img", "lid", "map") are complete.  With frozen parameters the hooks fire as always, in the same order; a
        sub-backward nothing trainable needs is not issued (_install_mask) and the frozen ranges of a group hold +0.0 when its
        hook fires."""
        self.trainable_mask()
        self.backward_begin(dpred, gscale, on_ready=on_ready)
        for s in range(3, -1, -1):
            self.backward_scale(s, on_ready=on_ready)
            if on_stage is not None:
                on_stage(3 - s)

    def _ready(self, hook, stage, group):
        key = (stage, group)
        tab = self._fill_tabs.get(key)
        if tab is not None and key not in self._filled:
            # gradients of frozen tensors that launches of this group wrote as a byproduct: back to +0.0, on the stream that
            # wrote them, before anything reads the group
            ops.fill_ranges(self.layout.grads, tab)
            self._filled.add(key)
        if hook is not None and key in self.layout.group_ranges:
            hook(key)

    @_in_precision
    def backward_begin(self, dpred=None, gscale=None, on_ready=None):
        """Head backward + gradient of the global-average-pool/sum: seeds the per-branch gradients."""
        ctx, B = self._last
        bufs = ctx.bufs
        self._adj_done = False
        self._filled = set()
        g_fused = self.head.bwd(ctx, dpred, gscale)
        if self.rad is None:   # (rad: the "head" group also holds the radar encoder, complete after the deepest transformer)
            self._ready(on_ready, 0, "head")
        shapes = [f.shape for f in self.pre_add[3]]
        self._G = [bufs.get("G3.%d" % m, shp, ctx.adt) for m, shp in enumerate(shapes)]
        ops.gap_sum_bwd(g_fused, self._G, frames=(self.frames + [1])[:len(self._G)])

    @_in_precision
    def backward_scale(self, s, on_ready=None):
        """Backward of fusion scale s (3 = deepest): GPT_s, then ResNet stage s+1 of the three branches
        (s = 0: layer1 + stems + VectorNet).  After it returns (enqueues), backward stage 3-s is complete."""
        ctx, B = self._last
        st = 3 - s
        names = ("img", "lid", "map")
        bufs = ctx.bufs
        trunks = [self.img, self.lid, self.map]
        G = self._G
        gpt = self.gpts[s]
        frames, base = self.frames + [1], self.group_base + [sum(self.frames)]
        plan = self._plan
        if plan is not None and not plan["gpt"][s]:
            # nothing trainable in this transformer or anywhere below it: no launch, the groups are reported as always
            self._ready(on_ready, st, "gpt")
            if s == 3 and self.rad is not None:
                self._ready(on_ready, 0, "head")
            group = lambda m: "vec" if (s == 0 and m == 2 and self.variant != "img") else names[m]
            self._branches([lambda m=m: self._ready(on_ready, st, group(m)) for m in range(3)])   # (the lanes' own order and streams)
            if s == 0:
                self._fill_rest()
            return
        gtok = bufs.get("gtok%d" % s, (B, gpt.T, gpt.C), ctx.adt)
        for m, g in enumerate(G):
            if not (self._adj_done and m < 3):   # the three branch lanes of the previous scale already spread their gradient
                ops.upsample_adj(g, gtok, base[m], frames[m])
        gin = gpt.bwd(ctx, gtok)
        self._ready(on_ready, st, "gpt")
        if s == 3 and self.rad is not None:
            if plan is None or plan["rad"]:
                dF3 = ops.pool_bcast_add(G[3], gin, bufs.get("dF3.3", G[3].shape, G[3].dtype), base[3], 1)
                self.rad.bwd(ctx, dF3)
            self._ready(on_ready, 0, "head")
        if s > 0:
            nxt = self.gpts[s - 1]
            gtok_next = bufs.get("gtok%d" % (s - 1), (B, nxt.T, nxt.C), ctx.adt)

            def stage(m):
                if plan is not None and not plan["layer"][s][m]:   # this stage of the trunk and everything below it is frozen
                    self._ready(on_ready, st, names[m])
                    return None
                d = ops.pool_bcast_add(G[m], gin, bufs.get("dF%d.%d" % (s, m), G[m].shape, G[m].dtype), base[m], frames[m])
                g = trunks[m].layer_bwd(ctx, s + 1, d)
                self._ready(on_ready, st, names[m])
                # the adjoint of the next scale's upsample-add for this branch (its own 64 token rows of gtok) at the tail of
                # the lane, beside the other lanes, instead of three launches on the main stream ahead of the transformer
                if plan is None or plan["gpt"][s - 1]:
                    ops.upsample_adj(g, gtok_next, base[m], frames[m])
                return g

            self._G = self._branches([lambda m=m: stage(m) for m in range(3)])
            self._adj_done = True
            return

        tail = (True, True, True) if plan is None else plan["tail"]   # False: the stem, layer1 (or VectorNet) are all frozen

        def img_tail():
            if tail[0]:
                d = ops.pool_bcast_add(G[0], gin, bufs.get("dF0.0", G[0].shape, G[0].dtype), base[0], frames[0])
                self.img.stem_bwd(ctx, self.img.layer_bwd(ctx, 1, d))
            self._ready(on_ready, st, "img")

        def lid_tail():
            if tail[1]:
                d = ops.pool_bcast_add(G[1], gin, bufs.get("dF0.1", G[1].shape, G[1].dtype), base[1], frames[1])
                self.lid.stem_bwd(ctx, self.lid.layer_bwd(ctx, 1, d))
            self._ready(on_ready, st, "lid")

        def map_tail():
            if tail[2]:
                d = ops.pool_bcast_add(G[2], gin, bufs.get("dF0.2", G[2].shape, G[2].dtype), base[2], frames[2])
                if self.variant == "img":
                    self.map.stem_bwd(ctx, self.map.layer_bwd(ctx, 1, d))
                else:
                    self.vec.bwd(ctx, d)
            self._ready(on_ready, st, "map" if self.variant == "img" else "vec")

        self._branches([img_tail, lid_tail, map_tail])
        self._fill_rest()

    def _fill_rest(self):
        """After the last scale: the frozen ranges of a group the backward did not report (none in the variants as built)."""
        for key, tab in self._fill_tabs.items():
            if key not in self._filled:
                ops.fill_ranges(self.layout.grads, tab)
                self._filled.add(key)

    # ------------------------------------------------------------------ optimizer
    def set_param_groups(self, group_of):
        """group_of: uint8 device tensor with one optimizer-group id per 4 consecutive floats of the flat buffer
        (optim.FusedAdamW builds it from torch-style param_groups), or None = one group."""
        self.opt_group_of = group_of

    def set_amsgrad(self, flags):
        """flags: one bool per optimizer group, torch.optim.AdamW's amsgrad (optim.FusedAdamW hands them over beside its hyper
        rows).  The first set flag allocates layout.max_exp_avg_sq (zeros, a fifth flat buffer); with none set nothing is
        allocated and every step issues the launches it always issued.  The flags reach the kernel through the last column of
        the hyper table (set_hyper).  Steps with a set flag run eagerly: parallel.GraphedStep refuses to capture them, and to
        replay a step captured before a flag was set."""
        flags = tuple(bool(f) for f in flags)
        if flags == self.opt_amsgrad:
            return
        if len(flags) > 16:
            raise ValueError("at most 16 optimizer groups")
        if any(flags) and self.opt_kind != "adamw":
            raise ValueError("amsgrad is a flag of AdamW groups: the engine's optimizer is %r (Engine.set_optimizer)" % self.opt_kind)
        if any(flags) and self.layout.max_exp_avg_sq is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("max_exp_avg_sq must be allocated before a hipGraph capture: call Engine.set_amsgrad() before it")
            self.layout.ensure_max_exp_avg_sq()
        self.opt_amsgrad = flags

    OPTIMIZERS = ("adamw", "sgd")

    def set_optimizer(self, kind):
        """The update rule of every optimizer step: "adamw" (the default; torch.optim.AdamW) or "sgd" (torch.optim.SGD with
        momentum, optim.FusedSGD).  Everything around the launch is shared: the hyper table (an SGD row is (lr, momentum, dampening,
        nesterov, weight_decay) in the place of AdamW's five), groups, frozen masks, step classes, clipping, the guard, the
        average.  The momentum buffer is layout.exp_avg; the caller answers for what it holds when the kind changes
        (optim.FusedSGD(reset_state=True)).  A captured step records the kind and refuses to replay after it changed
        (parallel.GraphedStep).  amsgrad flags and "sgd" exclude each other."""
        if kind not in self.OPTIMIZERS:
            raise ValueError("optimizer kind must be one of %s, got %r" % (" / ".join(self.OPTIMIZERS), kind))
        if kind == self.opt_kind:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the optimizer kind changed inside a hipGraph capture")
        if self.accum_pending:
            raise RuntimeError("the optimizer kind changed while %d accumulated micro-step(s) are pending: finish them with "
                               "train_step() or drop them with discard_accumulated() first" % self.accum_pending)
        if kind != "adamw" and any(self.opt_amsgrad):
            raise ValueError("amsgrad is on in an optimizer group: clear the flags (Engine.set_amsgrad) before switching to %r" % kind)
        self.opt_kind = kind

    # ------------------------------------------------------------------ objective (mmfn_amd.losses)
    def set_loss(self, loss):
        """The objective of every TRAINING forward with a ground truth (train_step, accumulate_step, their captured forms, forward(inp,
        True, gt)): a losses.WaypointLoss, or None for the reference's mean L1.  An eval forward's loss stays the mean L1, so
        validation losses keep their meaning across runs.  A batch may also carry inp["sample_weight"] ([B] float32 on the device), with
        or without a loss object.  With a plain loss (None, or L1 without step weights) and no sample weights the head runs its
        original two launches, bit for bit; anything else runs mmfn_gru_head_fwd_loss_f32 / mmfn_gru_head_bwd_loss_f32.  beta / delta
        and the horizon weights live in a 16-float device table, written here, outside any capture: a captured step stays valid when
        they change.  The kind is a launch argument: a captured step records it and refuses to replay after it changed
        (parallel.GraphedStep).  Everything behind the head (accumulation, clipping, the guard, averaging, frozen parameters, the
        optimizer launch, data parallel: each rank the mean over its own batch, as DDP) sees only the gradient."""
        from .losses import WaypointLoss
        if loss is not None and not isinstance(loss, WaypointLoss):
            raise TypeError("set_loss takes a mmfn_amd.losses.WaypointLoss or None, got %r" % (loss,))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the loss changed inside a hipGraph capture")
        if self.accum_pending:
            raise RuntimeError("the loss changed while %d accumulated micro-step(s) are pending: finish them with "
                               "train_step() or drop them with discard_accumulated() first" % self.accum_pending)
        self._install_loss(loss)

    def _install_loss(self, loss):
        """set_loss behind its checks (Trainer.train restores the previous loss through it, also after an epoch that failed)."""
        if loss is not None:
            loss.check_steps(self.head.steps)
        self.loss = loss
        self.head.plain = loss is None or loss.is_plain()
        self.head.loss_kind = 0 if loss is None else loss.kind_code
        if self.head.loss_table is not None or not self.head.plain:
            self._loss_table(write=True)

    def _loss_table(self, write=False):
        """The device table of the head's loss launches: allocated on first need (a loss that is not plain, a batch with sample
        weights), never inside a capture; rewritten by every set_loss from then on."""
        head = self.head
        if head.loss_table is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the loss table must be allocated before a hipGraph capture: run one eager step of the batch "
                                   "(or Engine.set_loss) before it")
            head.loss_table = torch.zeros(16, dtype=torch.float32, device=self.device)
            write = True
        if write:
            from .losses import PLAIN
            head.loss_table.copy_(torch.tensor((self.loss or PLAIN).table(head.steps), dtype=torch.float32))
        return head.loss_table

    def loss_key(self):
        """What a capture records of the objective: None for a plain loss, else its kind (beta / delta / horizon weights are device
        memory and not part of a capture)."""
        return None if self.head.plain else self.loss.kind

    def sample_losses(self, batch=None):
        """Device tensor [B]: each sample's share of the last forward's loss, sw[b] * sum_t hw[t] * sum_c rho(e) / (pred_len * 2) (their
        mean is the loss).  No host sync; a view of a buffer the next forward of this batch size overwrites.  batch: the batch
        size (default: the last forward's)."""
        B = self._last[1] if batch is None else int(batch)
        return self._bufs_for(B).get("head.lt", (B,)) / float(self.head.steps * 2)

    def sample_l1(self, batch=None):
        """As sample_losses, the unweighted mean |pred - gt| of each sample - comparable with the L1 validation loss whatever the
        objective.  None when the last training forward ran the plain path (its sample_losses are these numbers)."""
        if not self.head.lossy:
            return None
        B = self._last[1] if batch is None else int(batch)
        return self._bufs_for(B).get("head.l1", (B,)) / float(self.head.steps * 2)

    def amsgrad_flags(self, n_groups):
        """The amsgrad flags of a step with n_groups hyper rows (a group without a flag has none; a step with one row runs
        everything as group 0, as in _group_table)."""
        f = self.opt_amsgrad[:n_groups]
        return f + (False,) * (n_groups - len(f))

    def set_hyper(self, rows):
        """rows: [(lr, beta1, beta2, eps, weight_decay, grad_scale), ...] one per optimizer group.  They live in a small
        device table read by the AdamW kernel, so a learning-rate schedule changes the table (one tiny host-to-device copy,
        outside any captured graph) instead of invalidating captured hipGraphs."""
        rows = tuple(tuple(float(x) for x in r) for r in rows)
        flags = self.amsgrad_flags(len(rows))
        if rows == self._hyper_host and flags == self._hyper_flags:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("optimizer hyper-parameters changed inside a hipGraph capture; call Engine.set_hyper() before it")
        if len(rows) > 16:
            raise ValueError("at most 16 optimizer groups")
        # two pinned staging slots used alternately: the copy is asynchronous on the compute stream (a per-iteration LR schedule
        # must not block the host until the previous step has drained), and a slot is only rewritten two updates later
        if self._hyper_pinned is None:
            self._hyper_pinned = [torch.zeros(16, 8, dtype=torch.float32).pin_memory() for _ in range(2)]
            self._hyper_events = [None, None]
        slot = self._hyper_slot = (self._hyper_slot + 1) % 2
        if self._hyper_events[slot] is not None:
            self._hyper_events[slot].synchronize()   # the copy issued two updates ago has long finished
        host = self._hyper_pinned[slot]
        host.zero_()
        for i, r in enumerate(rows):
            host[i, :len(r)] = torch.tensor(r, dtype=torch.float32)   # (a 7th column: max_norm of a clipped step)
            host[i, 7] = 1.0 if flags[i] else 0.0                      # (the 8th: the group's amsgrad flag)
        self.opt_hyper.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hyper_events[slot] = ev
        self._hyper_host = rows
        self._hyper_flags = flags

    @staticmethod
    def hyper_rows(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, groups=None):
        if groups is None:
            groups = [(lr, betas[0], betas[1], eps, weight_decay)]
        return [tuple(r[:5]) + (grad_scale,) for r in groups]

    def optimizer_step(self, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, groups=None):
        """torch.optim.AdamW step over the trained range of the flat buffer.  `groups`: per-group
        (lr, beta1, beta2, eps, weight_decay) rows (FusedAdamW.hyper_rows()); default one group from the scalars."""
        if self.accum_pending:
            raise RuntimeError("%d accumulated micro-step(s) are pending: finish them with train_step() or drop them with "
                               "discard_accumulated() before a direct optimizer_step()" % self.accum_pending)
        self.trainable_mask()
        groups = self.hyper_rows(lr, betas, eps, weight_decay, grad_scale, groups)
        self.set_hyper(groups)
        self.module.weights_changed()
        self._advance_steps()
        self._adamw(len(groups))

    # ------------------------------------------------------------------ weight average (mmfn_amd.averaging)
    def attach_average(self, avg):
        """From now on every optimizer step of the fused path (optimizer_step, final_adam: eager, graph-replayed, data parallel)
        also updates `avg` inside its AdamW launch; accumulate_step micro-steps do not.  A captured step records whether an
        average was attached and refuses to replay after that changed (parallel.GraphedStep)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("attach_average() inside a hipGraph capture")
        avg.check_model(self.module)
        avg.copy_tail(self.module)
        self.average = avg

    def detach_average(self):
        self.average = None

    def _adamw(self, n_groups, coef=None, ok=None):
        """The optimizer launch over the trained range - AdamW, or momentum SGD when set_optimizer("sgd") chose it - (coef: the
        clipping instance).  With an attached average it is folded into the
        launch, then come the average's BatchNorm buffers and its count: three launches (+ a counter copy) instead of one.  ok:
        the non-finite guard's flag, every one of them behind it."""
        L, a = self.layout, self.average
        avg = None if a is None else (a.module._layout.params, a.n_averaged, a.ema_weight, a.mode_code)
        # amsgrad in some group of the table as set_hyper wrote it: the launch that also carries max_exp_avg_sq (None: the plain one)
        vmax = L.max_exp_avg_sq if any(self._hyper_flags[:n_groups]) else None
        if self.opt_kind == "sgd":
            # momentum SGD: the same launches over (p, g, momentum buffer = exp_avg); a tensor's first step is the one its count
            # reads 1 at, which the step classes make per tensor
            if vmax is not None:
                raise ValueError("amsgrad flags in the hyper table of an SGD step")
            groups, rows, state = ops.sgd_groups, ops.sgd_rows, (L.exp_avg,)
            kw = dict(n=L.tail, coef=coef, avg=avg, ok=ok)
        else:
            groups, rows, state = ops.adamw_groups, ops.adamw_rows, (L.exp_avg, L.exp_avg_sq)
            kw = dict(n=L.tail, coef=coef, avg=avg, ok=ok, vmax=vmax)
        if not self.classes.uniform():
            # a tensor that steps has a count of its own: the launch whose scalars follow the step classes
            row_of, row_map = self._rows(n_groups)
            rows(L.params, L.grads, *state, self._class_steps, self.classes.n_classes, self.opt_hyper, n_groups, row_of, row_map, **kw)
        elif self.frozen:
            # the masked instance: frozen float4s keep parameter, state and decay untouched (the average still follows them)
            groups(L.params, L.grads, *state, self.step_count, self.opt_hyper, n_groups, group_of=self._group_table(n_groups),
                   mask=True, **kw)
        else:
            groups(L.params, L.grads, *state, self.step_count, self.opt_hyper, n_groups,
                   group_of=self.opt_group_of if n_groups > 1 else None, **kw)
        self.never_stepped = self.frozen if self.never_stepped is None else (self.never_stepped & self.frozen)
        self.classes.launched()
        if a is not None:
            a.update_buffers(self.module, ok=ok)
            ops.step_advance(a.n_averaged, ok=ok)
            a.module.weights_changed()

    # ------------------------------------------------------------------ non-finite guard
    def set_nonfinite_guard(self, on=True):
        """Armed: every optimizer step of the fused path (train_step, the replayed "final" step, data parallel) measures the
        global gradient norm (the clipped route, max_norm = inf unless the caller clips) and decides ON THE DEVICE whether to
        take the step: a non-finite norm leaves parameters, moments, step_count and an attached average bit-identical, restores
        the BatchNorm running statistics and counters of the start of the accumulation group, clears the accumulator and counts
        the step in skipped_steps; a finite norm gives the unguarded step bit for bit.  rng_state advances either way.  The guard
        keys on the gradient, not the loss (a non-finite label can leave the gradient finite), and does not cover a direct
        optimizer_step().  A captured step records the arming and refuses to replay after it changed (parallel.GraphedStep)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_nonfinite_guard() inside a hipGraph capture")
        if on and self._guard is None:
            L, dev = self.layout, self.device
            self._guard = {"ok": torch.ones(1, dtype=torch.int32, device=dev), "skipped": torch.zeros(1, dtype=torch.int64, device=dev),
                           "buffers": torch.zeros_like(L.buffers_flat), "counters": torch.zeros_like(L.counters_flat)}
            self._norm_state()
        self.nonfinite_guard = bool(on)

    @property
    def skipped_steps(self):
        """Device int64 [1]: optimizer steps the guard has skipped (None before it was first armed)."""
        return None if self._guard is None else self._guard["skipped"]

    def guarded_clip(self, clip_grad_norm):
        """max_norm of an optimizer step: the caller's, or inf while the guard is armed (its decision needs the norm)."""
        return float("inf") if clip_grad_norm is None and self.nonfinite_guard else clip_grad_norm

    def guard_snapshot(self):
        """BatchNorm running statistics and counters as the first micro-step of a group finds them: two device copies, issued
        in front of that step (outside a captured graph), restored by final_adam when the step is skipped."""
        if self.nonfinite_guard and self.accum_pending == 0:
            L, G = self.layout, self._guard
            G["buffers"].copy_(L.buffers_flat)
            G["counters"].copy_(L.counters_flat)

    def tensor_stats(self, which="grads"):
        """(names, float64 [n, 3] device tensor): per trained tensor, in layout order, the L2 norm over all entries (non-finite if
        any entry is), max |x| over the finite entries and the count of non-finite entries of the gradient ("grads": the
        averaged gradient the last optimizer step saw - the buffer times that step's grad_scale, without the clip coefficient,
        what last_grad_norm measures) or the parameters ("params").  One read-only pass, on demand, no host sync."""
        if which not in ("grads", "params"):
            raise ValueError("which must be 'grads' or 'params', got %r" % (which,))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("tensor_stats() inside a hipGraph capture")
        L = self.layout
        if self._stats_tab is None:
            names = [n for n in L.offsets if n not in L.unused]
            self._stats_tab = (names, ops.tensor_stats_table([L.offsets[n] for n in names], self.device))
        names, tab = self._stats_tab
        scale = 1.0
        if which == "grads" and self._hyper_host:
            scale = self._hyper_host[0][5]
        return list(names), ops.tensor_stats(L.grads if which == "grads" else L.params, tab, scale)

    def train_step(self, inp, gt, lr=1e-4, dp=None, clip_grad_norm=None, **adam):
        """One training step (see _train_step) under a single read of the requires_grad flags."""
        with self.mask_held():
            return self._train_step(inp, gt, lr, dp, clip_grad_norm, **adam)

    def _train_step(self, inp, gt, lr, dp, clip_grad_norm, **adam):
        """zero-grad (implicit: every gradient is overwritten) + forward + L1 + backward + AdamW
        (phase2_train_net.py:60-110).  `dp` (mmfn_amd.parallel.DataParallel) reduces the gradient
        buckets across ranks while the backward is still running.  `adam` may carry betas / eps /
        weight_decay.  Returns the device loss scalar.

        After accumulate_step() calls this is the last micro-step of the group: the pending sum is folded into this
        backward's gradient and AdamW sees 1 / ((pending + 1) * world) of it.  clip_grad_norm = max_norm: the step is clipped
        as torch.nn.utils.clip_grad_norm_ over every trained parameter (the norm of the averaged gradient; inf = only measure
        it), the norm is left in last_grad_norm.  With neither, the per-group pass and the norm are no launches at all and what
        is left is backward (+ the buckets' reductions), step count, AdamW: the plain step.  With the non-finite guard armed
        (set_nonfinite_guard) the step always takes the clipped route and may be skipped on the device.

        The hyper table is written (set_hyper: an asynchronous host-to-device copy on the compute stream, never part of a
        capture) in front of the backward; its only readers, the norm finalize and AdamW, come after the backward."""
        self.guard_snapshot()
        clip_grad_norm = self.guarded_clip(clip_grad_norm)
        ops.rng_advance(self.rng_state)
        _, loss = self.forward(inp, True, gt)
        pending = self.accum_pending
        self.set_hyper(self.final_rows(lr, pending, dp, clip_grad_norm, **adam))
        self.backward_groups(ops.ACCUM_FOLD if pending else ops.ACCUM_NONE, dp, clip_grad_norm is not None)
        self.final_adam(dp, clip_grad_norm is not None, len(self._hyper_host))
        return loss

    # ------------------------------------------------------------------ gradient accumulation / global-norm clipping
    def accumulate_step(self, inp, gt):
        """One accumulation micro-step (see _accumulate_step) under a single read of the requires_grad flags."""
        with self.mask_held():
            return self._accumulate_step(inp, gt)

    def _accumulate_step(self, inp, gt):
        """One micro-step of gradient accumulation: RNG advance, forward (BatchNorm running statistics update, as in the torch
        loop), L1 loss, backward, and acc += gradient per readiness group on the stream that wrote it.  No collective, no AdamW:
        the next train_step() folds the sum in.  Returns the device loss."""
        self._accum_buffer()
        self.guard_snapshot()
        ops.rng_advance(self.rng_state)
        _, loss = self.forward(inp, True, gt)
        self.backward_groups(ops.ACCUM_ADD, None, False)
        self.accum_pending += 1
        return loss

    def discard_accumulated(self):
        """Drop the pending micro-steps (acc = 0, count = 0)."""
        if self.grad_acc is not None:
            ops.fill(self.grad_acc, 0.0)
        self.accum_pending = 0

    @property
    def last_grad_norm(self):
        """Device tensor [1]: the global gradient norm of the last clipped optimizer step (None before one).  Reading it
        (.item()) is the only host sync."""
        return None if self._norm is None else self._norm["out"][0:1]

    def _check_tiling(self):
        """The per-group passes cover the trained range exactly once only if the readiness groups tile [0, tail) (DataParallel
        buckets rely on the same): checked once, loudly."""
        if self._tiling_checked:
            return
        L = self.layout
        r = sorted(L.group_ranges.values())
        ok = bool(r) and r[0][0] == 0 and r[-1][1] == L.tail and all(a[1] == b[0] for a, b in zip(r, r[1:])) and \
            all(b % 4 == 0 and e % 4 == 0 for b, e in r)
        if not ok:
            raise RuntimeError("the readiness groups of the flat gradient buffer do not tile [0, %d) in 4-float aligned ranges: "
                               "%s" % (L.tail, r))
        self._tiling_checked = True

    def _accum_buffer(self):
        if self.grad_acc is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the gradient accumulator must be allocated before a hipGraph capture")
            self._check_tiling()
            self.grad_acc = torch.zeros(self.layout.tail, dtype=torch.float32, device=self.device)
        return self.grad_acc

    def _norm_state(self):
        """fp64 partials table: the slots of every readiness group's pass (single GPU), then the slots of one pass over
        [0, tail) (data parallel: after the reduction); out = device (norm, coef)."""
        if self._norm is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the gradient-norm tables must be allocated before a hipGraph capture")
            self._check_tiling()
            L = self.layout
            slots, off = {}, 0
            for key, (b, e) in sorted(L.group_ranges.items(), key=lambda kv: kv[1][0]):
                n = ops.grad_accum_blocks(e - b)
                slots[key] = (off, n)
                off += n
            full = ops.grad_accum_blocks(L.tail)
            # (one spare slot behind each range: the guard's look at the BatchNorm statistics while parameters are frozen, final_adam)
            self._norm = {"partials": torch.zeros(off + 1 + full + 1, dtype=torch.float64, device=self.device), "groups": slots,
                          "n_group_slots": off, "full": (off + 1, full), "out": torch.zeros(2, dtype=torch.float32, device=self.device)}
        return self._norm

    def group_hooks(self, mode, partials, user=None):
        """(hook, rest) for one backward: hook(key) runs the accumulation pass `mode` over readiness group `key` (on the
        stream that reports it, the stream that wrote the group) and then the caller's hook (dp.reduce); rest() passes over
        the groups the backward never reported, after the join, before the reduction waits for them.  partials: write the
        group's sum-of-squares slots.  NONE without partials is no pass at all: (user, no-op)."""
        if mode == ops.ACCUM_NONE and not partials:
            return user, (lambda: None)
        L = self.layout
        acc = self._accum_buffer() if mode != ops.ACCUM_NONE else None
        nm = self._norm_state() if partials else None
        done = set()

        def run(key):
            if key in done:
                return
            done.add(key)
            b, e = L.group_ranges[key]
            part = None
            if nm is not None:
                o, n = nm["groups"][key]
                part = nm["partials"][o:o + n]
            ops.grad_accum(L.grads[b:e], None if acc is None else acc[b:e], mode, part)

        def hook(key):
            run(key)
            if user is not None:
                user(key)

        def rest():
            for key, _ in sorted(L.group_ranges.items(), key=lambda kv: kv[1][0]):
                run(key)

        return hook, rest

    def backward_groups(self, mode, dp, partials):
        """Backward of the last training forward with the per-group pass `mode` (accumulate_step: ADD; the final micro-step:
        FOLD, or NONE with partials for a clipped step without accumulation) in front of dp.reduce.  With dp the norm is taken
        after the reduction (final_adam), so no group partials here."""
        hook, rest = self.group_hooks(mode, partials and dp is None, dp.reduce if dp is not None else None)
        if dp is not None:
            dp.begin()
        self.backward(on_ready=hook)
        rest()
        if dp is not None:
            dp.finish()

    def final_rows(self, lr, pending, dp, clip_grad_norm, **adam):
        """Hyper-parameter rows of the optimizer step that closes an accumulation group of pending + 1 micro-steps:
        grad_scale = 1 / ((pending + 1) * world), column 6 = max_norm when clipping."""
        world = dp.world if dp is not None else 1
        rows = self.hyper_rows(lr=lr, grad_scale=1.0 / ((pending + 1) * world), **adam)
        if clip_grad_norm is not None:
            rows = [tuple(r) + (float(clip_grad_norm),) for r in rows]
        return rows

    def final_adam(self, dp, clip, n_groups):
        """AdamW after backward_groups, reading the hyper table as set (final_rows); clip: global norm of the scaled
        gradient (group partials on one GPU, one read-only pass over [0, tail) after the reduction with dp), the coefficient,
        and the coefficient AdamW.  Resets the pending count.  Guard armed: the finalize also writes the flag, and the step
        count, the BatchNorm rollback, AdamW and the average's update all sit behind it."""
        L = self.layout
        guard = self._guard if self.nonfinite_guard else None
        if guard is not None and not clip:
            raise RuntimeError("the non-finite guard decides on the gradient norm: its optimizer step is the clipped one")
        self.module.weights_changed()
        if guard is None:
            self._advance_steps()
        coef = ok = None
        if clip:
            nm = self._norm_state()
            if dp is not None:
                o, n = nm["full"]
                part = nm["partials"][o:o + n]
                ops.grad_accum(L.grads[:L.tail], None, ops.ACCUM_NONE, part)
            else:
                o, n = 0, nm["n_group_slots"]
                part = nm["partials"][:n]
            if guard is not None and self.frozen and dp is None:
                # Frozen parameters hide what the guard keys on: the backward of a frozen trunk is not run and a ReLU drops a
                # NaN, so a non-finite input can leave every TRAINABLE gradient finite while the forward has already written
                # non-finite BatchNorm running statistics.  One more partial - NaN when those statistics are not finite, else
                # 0.0 (the norm keeps its bits) - makes the step skip and roll them back, as the same step does with nothing frozen.
                # Single GPU only: the statistics are rank-local, and under data parallel every rank must reach the same
                # decision from the reduced gradient alone
                ops.nonfinite_slot(L.buffers_flat, nm["partials"][o + n:o + n + 1])
                part = nm["partials"][o:o + n + 1]
            out = nm["out"]
            coef = out[1:2]
            ok, skipped = (None, None) if guard is None else (guard["ok"], guard["skipped"])
            ops.grad_norm_finalize(part, self.opt_hyper[0, 5:6], self.opt_hyper[0, 6:7], out[0:1], coef, ok=ok, skipped=skipped)
            if guard is not None:
                self._advance_steps(ok=ok)
                ops.copy_if(L.buffers_flat, guard["buffers"], ok, when=False)    # skipped: the group's BatchNorm updates go
                ops.copy_if(L.counters_flat, guard["counters"], ok, when=False)
        self._adamw(n_groups, coef=coef, ok=ok)
        self.accum_pending = 0
