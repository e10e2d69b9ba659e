"""Thin host wrappers: torch tensors (device memory only) -> C-ABI launches.

Every function enqueues HIP kernels from libmmfn_hip.so on the current torch stream and
returns without synchronising.  Feature maps are NHWC ([B,H,W,C] contiguous); conv weights are
[Cout,KH,KW,Cin] contiguous; Linear weights are [out,in] as in the reference checkpoint.
"""
import ctypes
import json
import os

import torch

from . import _lib
from ._lib import (EPI_KEEP_SLABS, A_COLMAJOR, A_DGRAD, A_IM2COL, A_ROWMAJOR, B_DGRADW, B_IM2COL, B_KN, B_NK,
                   EPI_ACCUM, EPI_BF16_OPERANDS, EPI_BF16X3, EPI_BIAS, EPI_COLSUM_A, EPI_DROPOUT, EPI_GELU, EPI_LN_FOLD, EPI_MASK_AUX, EPI_RELU, EPI_RELU_LAST,
                   EPI_RESIDUAL,
                   GemmDesc, GptBlockDesc, check, lib, ptr, stream)

BF16 = torch.bfloat16   # activations of the bf16 training mode: the wrappers below dispatch on the tensors' dtype
_workspace = {}
_retired = []  # scratch buffers that were outgrown: never freed, captured hipGraphs may still point into them
_lane = 0  # logical execution lane (0 = main stream, 1.. = engine side streams); scratch buffers are per lane


_gemm_dtype = "f32"
# bf16 mode keeps the convolution WEIGHT gradients in fp32: measured on MI355X the bf16 kernel's pixel-contracted form (both
# operands pixel-major, transposed into k-contiguous LDS rows in registers) runs at 28-138 TF/s, slower than the fp32 Winograd-
# domain weight gradient (and than the fp32 direct one at 64 channels), and fp32 weight gradients are the more accurate anyway.
# MMFN_BF16_WGRAD=1 selects the bf16 kernel (kept for its tests and for a transpose-read rewrite).
BF16_WGRAD = False


class precision(object):
    """Context manager: arithmetic of the plain GEMMs launched inside.  "f32" (default): fp32 MFMA, the parity path.
    "bf16": operands rounded to bf16 on their way into LDS, bf16 MFMA, fp32 accumulation / outputs / master weights
    (MMFN_EPI_BF16_OPERANDS; BASELINE configs[2]).  Convolution gather forms always run in fp32."""

    def __init__(self, dtype):
        assert dtype in ("f32", "bf16", "f32x3"), dtype
        self.dtype = dtype

    def __enter__(self):
        global _gemm_dtype
        self.prev, _gemm_dtype = _gemm_dtype, self.dtype

    def __exit__(self, *exc):
        global _gemm_dtype
        _gemm_dtype = self.prev


def current_precision():
    """The arithmetic plain GEMMs launched now would run in (see `precision`)."""
    return _gemm_dtype


class lane(object):
    """Context manager: kernels launched inside use the scratch buffers of logical lane `i`.  (Keying by the
    raw stream pointer would break under hipGraph capture, where the capturing stream is a fresh one.)"""

    def __init__(self, i):
        self.i = i

    def __enter__(self):
        global _lane
        self.prev, _lane = _lane, self.i

    def __exit__(self, *exc):
        global _lane
        _lane = self.prev


def current_lane():
    return _lane


class GemmProfiler(object):
    """Brackets every GEMM / convolution of the step with HIP events on the launch stream and tallies
      * its ALGORITHMIC FLOPs: what the operation is (2*M*N*K of the matmul; output pixels x taps x Cin x Cout of the
        convolution, not the zero-inflated implicit-GEMM count) - SURVEY.md section 8d's accounting, and
      * the FLOPs the MFMA units actually EXECUTE for it, which is less when the convolution goes through the Winograd
        transforms (one record then spans filter/input/output transforms + the batched GEMM)."""

    def __init__(self):
        self.records = []   # (start, end, algorithmic flops, tag, algorithmic bytes, executed flops)
        self.suspended = 0

    def summary(self):
        torch.cuda.synchronize()
        ms = sum(r[0].elapsed_time(r[1]) for r in self.records)
        return len(self.records), float(sum(r[2] for r in self.records)), ms

    def executed_flops(self):
        return float(sum(r[5] for r in self.records))

    def algo_bytes(self):
        return float(sum(r[4] for r in self.records))

    def by_tag(self):
        torch.cuda.synchronize()
        out = {}
        for s, e, f, tag, _, _ in self.records:
            n, fl, ms = out.get(tag, (0, 0.0, 0.0))
            out[tag] = (n + 1, fl + f, ms + s.elapsed_time(e))
        return out

    def subset(self, prefix):
        """(launches, algorithmic flops, ms) of the records whose tag starts with `prefix` ("bf16 ": the launches that ran on
        the bf16-operand kernel)."""
        torch.cuda.synchronize()
        rows = [r for r in self.records if r[3].startswith(prefix)]
        return len(rows), float(sum(r[2] for r in rows)), sum(r[0].elapsed_time(r[1]) for r in rows)


class _whole_op(object):
    """Profiler bracket around a multi-kernel operation (Winograd convolution): one record with the operation's
    algorithmic FLOPs / bytes; the GEMM launched inside is not recorded a second time."""

    def __init__(self, tag, flops, abytes, executed):
        self.args = (tag, flops, abytes, executed)

    def __enter__(self):
        self.on = _profiler is not None and _profiler.suspended == 0
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        if _profiler is not None:
            _profiler.suspended += 1

    def __exit__(self, *exc):
        if _profiler is not None:
            _profiler.suspended -= 1
        if self.on:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            tag, flops, abytes, executed = self.args
            _profiler.records.append((self.e0, e1, flops, tag, abytes, executed))


_profiler = None


def set_gemm_profiler(p):
    global _profiler
    _profiler = p


# ---------------------------------------------------------------- tile / split-K selection table
# The C library picks (tile, split-K) from an analytic time model; measured on MI355X that choice is 5-20 % off the
# best on a dozen of the step's dominant shapes (tools/gemm_sweep.py).  So the host keeps a table
#   (a_mode, b_mode, M, N, K, batch, conv geometry) -> (tile, splitk)
# loaded from mmfn_amd/tuning/gfx950.json (generated by tools/tune.py on the GPU box) and, when MMFN_AUTOTUNE=1,
# extended at run time: an unknown shape is timed once over the candidate grid on a scratch output (never inside
# graph capture) and the winner cached.  Both fields are plain inputs of the C ABI (mmfn_gemm_desc.tile/.splitk).
_tuned = {}
_TUNE_FILE = os.environ.get("MMFN_TUNING_FILE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning", "gfx950.json")
AUTOTUNE = os.environ.get("MMFN_AUTOTUNE", "0") == "1"
F32X3 = os.environ.get("MMFN_F32X3", "0") == "1"  # let fp32 GEMMs use the bf16x3 emulation kernel where the table says so
USE_TABLE = os.environ.get("MMFN_TUNING_TABLE", "1") != "0"
_SK_GRID = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96)
# mmfn_gemm_desc.tile -> (rows, columns) of the fp32 kernel's block tile (include/mmfn_hip.h); 7 = 64 x 64 as two waves of 32 x 64
TILE_DIMS = {1: (128, 128), 2: (64, 64), 3: (128, 64), 4: (64, 128), 5: (192, 64), 6: (64, 192), 7: (64, 64)}
TILE_IDS = tuple(int(t) for t in os.environ.get("MMFN_TUNE_TILES", "1,2,3,4,5,6,7").split(","))


def _tune_key(a_mode, b_mode, M, N, K, batch, conv):
    return "%d,%d,%d,%d,%d,%d|%s" % (a_mode, b_mode, M, N, K, max(1, batch), ",".join(str(v) for v in conv) if conv else "")


def load_tuning(path=None):
    path = path or _TUNE_FILE
    if os.path.isfile(path):
        with open(path) as f:
            for k, v in json.load(f).items():
                _tuned[k] = tuple(int(x) for x in v)
    return len(_tuned)


def save_tuning(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({k: list(v) for k, v in sorted(_tuned.items())}, f, indent=0)


if USE_TABLE:
    load_tuning()
    if F32X3:  # entries that pick the three-term bf16 emulation kernel for fp32 GEMMs (tools/tune.py under MMFN_F32X3=1)
        load_tuning(os.path.join(os.path.dirname(_TUNE_FILE), "gfx950_f32x3.json"))


def _autotune(d, C, key, reps=3):
    """Time the (tile, split-K) grid for descriptor d on a scratch output; returns the winner or (0, 0) = library default."""
    L = lib()
    M, N, K = d.M, d.N, d.K
    nkt = max(1, K // (32 if d.flags & (EPI_BF16_OPERANDS | EPI_BF16X3) else 16))
    scratch = torch.empty(max(1, d.batch) * M * N + 16, dtype=torch.float32, device=C.device)
    saved = (d.C, d.flags, d.tile, d.splitk, d.workspace, d.strideC, d.ldc)
    # a batched GEMM can split K only if its outputs are packed and the epilogue has no per-batch operand (as in the library)
    batch_split = d.batch <= 1 or (d.strideC == M * N and d.ldc == N and not d.flags & (EPI_RESIDUAL | EPI_MASK_AUX | EPI_ACCUM))
    d.C = ptr(scratch)
    d.flags = d.flags & ~EPI_ACCUM
    if d.batch > 1:
        d.strideC = M * N
    d.ldc = N

    def run(tile, sk):
        d.tile, d.splitk = tile, sk
        need = L.mmfn_gemm_workspace_bytes(ctypes.byref(d))
        d.workspace = ptr(workspace(need, C.device)) if need > 0 else None
        st = stream()
        for _ in range(2):
            if L.mmfn_gemm_f32(ctypes.byref(d), st) != 0:
                return None
        best = None
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(4):
                L.mmfn_gemm_f32(ctypes.byref(d), st)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) / 4
            best = t if best is None else min(best, t)
        return best

    base = run(0, 0)
    results = []
    plain = d.a_mode in (A_ROWMAJOR, A_COLMAJOR) and d.b_mode in (B_NK, B_KN)
    modes = [0]
    # (not with MMFN_EPI_COLSUM_A: the column sums are formed from the fp32 operand fragments of the native kernel only)
    if F32X3 and plain and not d.flags & (EPI_BF16_OPERANDS | EPI_BF16X3 | EPI_COLSUM_A) and K % 32 == 0:
        modes.append(EPI_BF16X3)  # fp32 on the bf16 pipe (three-term split) competes with the native fp32 MFMA kernel
    if base is not None:
        for mode in modes:
            d.flags = (saved[1] & ~EPI_ACCUM) | mode
            emu = bool(d.flags & (EPI_BF16_OPERANDS | EPI_BF16X3))
            kt = max(1, K // (32 if emu else 16))
            for tile in ((1, 2) if emu else TILE_IDS):
                bm, bn = TILE_DIMS[tile]
                blocks = -(-M // bm) * -(-N // bn)
                for sk in _SK_GRID:
                    if sk > 1 and (not batch_split or sk > kt // 4):
                        break
                    if blocks * sk * max(1, d.batch) < 96 or blocks * sk > 16384:
                        continue
                    t = run(tile, sk)
                    if t is not None:
                        results.append((t, tile, sk, mode))
    d.C, d.flags, d.tile, d.splitk, d.workspace, d.strideC, d.ldc = saved
    choice = (0, 0)
    if results:
        t, tile, sk, mode = min(results)
        if t < 0.97 * base:
            choice = (tile, sk, mode) if mode else (tile, sk)
    _tuned[key] = choice
    return choice


def workspace(nbytes, device):
    """Grow-only scratch buffer (split-K slabs); never freed so captured graphs stay valid.
    One buffer per (device, lane): branches running concurrently on side streams must not share slabs."""
    key = (str(device), _lane)
    buf = _workspace.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("split-K workspace must be sized before graph capture")
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(max(nbytes // 4 + 1, 1 << 22), dtype=torch.float32, device=device)
        _workspace[key] = buf
    return buf


def _f32c(t, name):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda, name
    return t


def gemm(A, B, C, M, N, K, lda, ldb, ldc, a_mode=A_ROWMAJOR, b_mode=B_NK, bias=None, res=None, ldr=0,
         aux=None, ldaux=0, relu=False, gelu=False, accum=False, relu_last=False, drop_p=0.0, rng_state=None, rng_stream=0,
         conv=None, splitk=0, tile=0, batch=1, strideA=0, strideB=0, strideC=0, ln_fold=None, colsum=None, slab_info=None):
    """colsum ([M] fp32, TN form): also the column sums of the A operand (MMFN_EPI_COLSUM_A: a Linear's bias gradient from its
    weight-gradient GEMM).
    ln_fold = (c1 [N], mean [M] or None, rstd [M] or None, eps): C = LayerNorm(A) . B^T + bias with B / bias the folded operands
    of ln_fold_weights (MMFN_EPI_LN_FOLD, include/mmfn_hip.h); mean / rstd receive the row statistics."""
    d = GemmDesc()
    d.batch, d.strideA, d.strideB, d.strideC = batch, strideA, strideB, strideC
    d.A, d.B, d.C = ptr(A), ptr(B), ptr(C)
    d.bias, d.res, d.aux = ptr(bias), ptr(res), ptr(aux)
    d.rng_state = ptr(rng_state)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc, d.ldr, d.ldaux = lda, ldb, ldc, ldr, ldaux
    d.a_mode, d.b_mode = a_mode, b_mode
    if conv is not None:
        (d.H, d.W, d.Cin, d.OH, d.OW, d.Cout, d.KH, d.KW, d.stride, d.pad) = conv
    flags = 0
    if bias is not None:
        flags |= EPI_BIAS
    if relu:
        flags |= EPI_RELU
    if gelu:
        flags |= EPI_GELU
    if aux is not None:
        flags |= EPI_MASK_AUX
    if drop_p > 0.0:
        flags |= EPI_DROPOUT
        d.drop_p = drop_p
        d.rng_stream = rng_stream
    if res is not None:
        flags |= EPI_RESIDUAL
    if accum:
        flags |= EPI_ACCUM
    if relu_last:
        flags |= EPI_RELU_LAST
    if ln_fold is not None:
        c1, ln_mean, ln_rstd, ln_eps = ln_fold
        assert bias is not None and a_mode == A_ROWMAJOR and b_mode == B_NK and batch <= 1
        flags |= EPI_LN_FOLD
        d.ln_c1, d.ln_mean, d.ln_rstd, d.ln_eps = ptr(c1), ptr(ln_mean), ptr(ln_rstd), float(ln_eps)
        splitk = 1
    # bf16 mode: plain GEMMs and - as DIRECT convolutions - the im2col forward / flipped data gradient and the weight gradient
    # (the library falls back to the fp32 kernel for what the bf16 kernel does not cover: 7x7 stems, stride-2 data gradients)
    bf16 = _gemm_dtype != "f32" and (conv is None or (_gemm_dtype == "bf16" and (
        (a_mode, b_mode) == (A_IM2COL, B_NK) or (BF16_WGRAD and (a_mode, b_mode) == (A_COLMAJOR, B_IM2COL)))))
    if bf16:
        flags |= EPI_BF16X3 if _gemm_dtype == "f32x3" else EPI_BF16_OPERANDS
    if colsum is not None:
        assert (a_mode, b_mode) == (A_COLMAJOR, B_KN) and batch <= 1 and not bf16
        flags |= EPI_COLSUM_A
        d.colsum = ptr(colsum)
    d.flags = flags
    d.splitk = splitk
    d.tile = tile
    L = lib()
    if tile == 0 and (splitk == 0 or ln_fold is not None) and (USE_TABLE or AUTOTUNE):
        key = ((_gemm_dtype + "|") if bf16 else "") + _tune_key(a_mode, b_mode, M, N, K, batch, conv)
        cfg = _tuned.get(key)
        if cfg is None and AUTOTUNE and _profiler is None and not torch.cuda.is_current_stream_capturing() and ln_fold is None:
            cfg = _autotune(d, C, key)
        if cfg is not None and len(cfg) == 3 and colsum is not None:
            # a table entry that moves this shape to the three-term bf16 emulation kernel (MMFN_F32X3=1): that kernel cannot also
            # return the A operand's column sums (mmfn_gemm_f32 answers MMFN_EINVAL to COLSUM_A + BF16X3), and the entry's
            # (tile, split) were measured for it - the fused bias gradient keeps the native kernel at the library's default
            cfg = None
        if cfg is not None and (len(cfg) == 2 or F32X3):
            d.tile, d.splitk = cfg[0], cfg[1]
            if len(cfg) == 3 and ln_fold is None:
                d.flags |= cfg[2]
        elif cfg is not None:  # table entry wants the emulation kernel but it is switched off: library default
            pass
    if ln_fold is not None:   # the plain GEMM's tile of the same shape (table entry or the library's model); never split - a tile
        d.splitk = 1          # that does not divide M x N falls back to 64 x 64 inside the launcher
    # slab_info (a dict): a launch that splits K leaves its slices un-combined (MMFN_EPI_KEEP_SLABS) and reports them here as
    # slab_info["splits"] (> 1) and slab_info["slabs"] (the workspace tensor, [splits][batch][M][N]); with splits == 1 C holds the result
    keep = slab_info is not None and flags == 0 and not bf16 and not (d.flags & (EPI_BF16X3 | EPI_BF16_OPERANDS))
    if keep:
        d.flags |= EPI_KEEP_SLABS
    need = L.mmfn_gemm_workspace_bytes(ctypes.byref(d))
    wsbuf = None
    if need > 0:
        wsbuf = workspace(need, C.device)
        d.workspace = ptr(wsbuf)
    if slab_info is not None:
        slab_info["splits"] = L.mmfn_gemm_f32_splits(ctypes.byref(d)) if (keep and wsbuf is not None) else 1
        slab_info["slabs"] = wsbuf
        if slab_info["splits"] <= 1:
            d.flags &= ~EPI_KEEP_SLABS
    if _profiler is None or _profiler.suspended:
        check(L.mmfn_gemm_f32(ctypes.byref(d), stream()), "mmfn_gemm_f32")
        return C
    if a_mode == A_DGRAD:  # true transposed-conv FLOPs: output pixels x Cin x taps x Cout
        H, W, Cin, OH, OW, Cout, KH, KW, st, pd = conv
        flops = 2.0 * (M // (H * W)) * OH * OW * Cin * KH * KW * Cout
        tag = "dgrad %dx%d c%d->%d k%d s%d" % (H, W, Cin, Cout, KH, st)
    else:
        flops = 2.0 * M * N * K * max(1, batch)
        if conv is not None:
            H, W, Cin, OH, OW, Cout, KH, KW, st, pd = conv
            tag = "%s %dx%d c%d->%d k%d s%d" % ("conv" if a_mode == A_IM2COL else "wgrad", H, W, Cin, Cout, KH, st)
        else:
            tag = "gemm a%d b%d %dx%dx%d" % (a_mode, b_mode, M, N, K)
    # algorithmic (compulsory) bytes: every operand element read once, every output written once
    if conv is not None:
        H, W, Cin, OH, OW, Cout, KH, KW, st, pd = conv
        nb = (M // (H * W)) if a_mode == A_DGRAD else ((M // (OH * OW)) if a_mode == A_IM2COL else (K // (OH * OW)))
        abytes = 4.0 * (nb * H * W * Cin + nb * OH * OW * Cout + Cout * KH * KW * Cin)
    else:
        abytes = 4.0 * (M * K + N * K + M * N) * max(1, batch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(L.mmfn_gemm_f32(ctypes.byref(d), stream()), "mmfn_gemm_f32")
    e1.record()
    _profiler.records.append((e0, e1, flops, ("bf16 " if bf16 else "") + tag, abytes, flops))
    return C


# ---------------------------------------------------------------- Linear
def linear_fwd(x, w, bias=None, out=None, **epi):
    """out[M,N] = x[M,K] @ w[N,K]^T (+bias, epilogue)."""
    M, K = x.shape
    N = w.shape[0]
    if x.dtype == BF16:   # bf16 mode: w is the bf16 shadow of the weight
        from . import ops16
        return ops16.linear_fwd(x, w, bias, out=out, **epi)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    return gemm(x, w, out, M, N, K, x.stride(0), w.stride(0), out.stride(0), A_ROWMAJOR, B_NK, bias=bias, **epi)


def linear_dx(dy, w, out=None, **epi):
    """dx[M,K] = dy[M,N] @ w[N,K].  bf16 mode: w is the TRANSPOSED bf16 shadow [K,N]."""
    if dy.dtype == BF16:
        from . import ops16
        return ops16.linear_dx(dy, w, out=out, **epi)
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    return gemm(dy, w, out, M, K, N, dy.stride(0), w.stride(0), out.stride(0), A_ROWMAJOR, B_KN, **epi)


def linear_dw(dy, x, out=None, db=None, **epi):
    """dw[N,K] = dy[M,N]^T @ x[M,K];  db ([N], optional) = the column sums of dy = the bias gradient: formed inside the same GEMM
    where the fast TN kernel runs (fp32, 16-byte aligned operands, M a multiple of 16, N and K multiples of 4), else by colsum()."""
    if dy.dtype == BF16:
        from . import ops16
        assert db is None
        return ops16.linear_dw(dy, x, out, **epi)
    M, N = dy.shape
    K = x.shape[1]
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=dy.device)
    if db is not None:
        fusable = (_gemm_dtype == "f32" and M % 16 == 0 and N % 4 == 0 and K % 4 == 0 and N >= 4 and K >= 4
                   and dy.stride(0) % 4 == 0 and x.stride(0) % 4 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0)
        if not fusable:
            colsum(dy, db)
            db = None
    return gemm(dy, x, out, N, K, M, dy.stride(0), x.stride(0), out.stride(0), A_COLMAJOR, B_KN, colsum=db, **epi)


# ---------------------------------------------------------------- Convolution (NHWC)
def conv_geom(x_shape, w_shape, stride, pad):
    B, H, W, Cin = x_shape
    Cout, KH, KW, Cin2 = w_shape
    assert Cin == Cin2
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    return (H, W, Cin, OH, OW, Cout, KH, KW, stride, pad), (B, OH, OW, Cout)


_wino = {}
WINOGRAD_MIN_CHANNELS = int(os.environ.get("MMFN_WINOGRAD_MIN_C", "64"))  # 0 disables the Winograd path


def _wino_scratch(n, device):
    """Per-(device, lane) scratch for the transformed filter / activations / products (grow-only, sized before capture)."""
    key = (str(device), _lane)
    buf = _wino.get(key)
    if buf is None or buf.numel() < n:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Winograd scratch must be sized before graph capture")
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _wino[key] = buf
    return buf


def winograd_ok(x_shape, w_shape, stride, pad, epi, for_wgrad=False):
    Co, KH, KW, Ci = w_shape
    B, H, W, _ = x_shape
    if _gemm_dtype == "bf16" and not for_wgrad:
        # bf16 mode runs every 3x3 convolution as a direct implicit GEMM on the bf16 MFMA pipe: rounding Winograd-domain
        # operands to bf16 amplifies the error (transform gains up to ~100), and at 16x the fp32 MFMA rate the 4x FLOP saving
        # no longer pays for the 2.25x larger transformed tensors
        return False
    return (WINOGRAD_MIN_CHANNELS > 0 and KH == 3 and KW == 3 and stride == 1 and pad == 1 and H % 2 == 0 and W % 2 == 0
            and min(Ci, Co) >= WINOGRAD_MIN_CHANNELS and Ci % 16 == 0 and Co % 16 == 0 and set(epi) <= {"res", "ldr"})


WINOGRAD_F4 = True   # F(4x4,3x3) wherever the image sides are multiples of 4 (tests flip it to reach the F(2x2) kernels)


def winograd_v_numel(x_shape):
    """Elements of the transformed-input tensor V of the F(4x4,3x3) path for an NHWC input of this shape."""
    B, H, W, C = x_shape
    return 36 * B * (H // 4) * (W // 4) * C


def winograd_f4_ok(x_shape, w_shape, stride, pad):
    """The F(4x4,3x3) form of the forward (what the fused BatchNorm-apply input transform exists for)."""
    return winograd_ok(x_shape, w_shape, stride, pad, {}) and WINOGRAD_F4 and x_shape[1] % 4 == 0 and x_shape[2] % 4 == 0


def wino_weight_group(table, n_layers, total):
    """All filter transforms of the step in one launch (table: uint8 device tensor of 32-byte records, see the header)."""
    _call("mmfn_wino_weight_group_f32", ptr(table), n_layers, total, stream())


def make_wino_group_table(pairs, device):
    """pairs: [(w [Co,3,3,Ci] storage tensor, U flat tensor)] -> (device table, n, total)."""
    import struct
    blob, start = b"", 0
    for w, u in pairs:
        Co, _, _, Ci = w.shape
        blob += struct.pack("<QQiiq", w.data_ptr(), u.data_ptr(), Co, Ci, start)
        start += Co * Ci
    t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    return t, len(pairs), start


def conv2d_winograd(x, w, out, res=None, m=None, keep_v=None, bn=None, keep_u=None, u_ready=False, x_bn=None):
    """3x3 stride-1 'same' convolution as Winograd F(m x m, 3x3): streaming transforms around one (m+2)^2-batch GEMM.
    m = 4 when the image size allows (4x fewer MFMA FLOPs), else 2.  keep_v (F(4x4) only): a per-layer buffer that
    receives the transformed input, so the weight gradient can reuse it instead of transforming x again.
    x_bn = (res or None, mean, rstd, weight, bias, relu, y_out or None) (F(4x4) only): x is the PRODUCER's convolution output and
    the convolution's input is [relu](bn(x) [+ res]), applied inside the input transform (mmfn_wino_input_bn_f32); y_out also
    receives that activation as a tensor."""
    B, H, W, Ci = x.shape
    Co = w.shape[0]
    if m is None:
        m = 4 if (WINOGRAD_F4 and H % 4 == 0 and W % 4 == 0) else 2
    n = (m + 2) * (m + 2)
    T = B * (H // m) * (W // m)
    buf = _wino_scratch(n * (Co * Ci + T * Ci + T * Co), x.device)
    U = buf[:n * Co * Ci]
    V = buf[n * Co * Ci:n * (Co * Ci + T * Ci)]
    if keep_v is not None and m == 4:
        V = keep_v.view(-1)[:n * T * Ci]
    if keep_u is not None and m == 4:   # the transformed filter, kept for the adjoint data gradient (conv2d_bwd_winograd)
        U = keep_u.view(-1)[:n * Co * Ci]
    Mt = buf[n * (Co * Ci + T * Ci):n * (Co * Ci + T * Ci + T * Co)]
    st = stream()
    with _whole_op("conv %dx%d c%d->%d k3 s1 (winograd F%d)" % (H, W, Ci, Co, m), 2.0 * B * H * W * Co * 9 * Ci,
                   4.0 * (B * H * W * (Ci + Co) + 9 * Co * Ci), 2.0 * n * T * Co * Ci):
        if not (u_ready and keep_u is not None and m == 4):   # u_ready: this layer's U was written by wino_weight_group
            _call("mmfn_wino_weight_f32", ptr(w), ptr(U), Co, Ci, m, st)
        if x_bn is not None:
            assert m == 4
            xres, xmean, xrstd, xw, xb, xrelu, y_out = x_bn
            _call("mmfn_wino_input_bn_f32", ptr(x), ptr(xres), ptr(xmean), ptr(xrstd), ptr(xw), ptr(xb), 1 if xrelu else 0, ptr(y_out),
                  ptr(V), B, H, W, Ci, st)
        else:
            _call("mmfn_wino_input_f32", ptr(x), ptr(V), B, H, W, Ci, m, st)
        gemm(V, U, Mt, T, Co, Ci, Ci, Ci, Co, A_ROWMAJOR, B_NK, batch=n, strideA=T * Ci, strideB=Co * Ci, strideC=T * Co)
        if bn is not None and m == 4 and res is None and 256 % (Co // 4) == 0:
            # BatchNorm batch statistics come out of the output transform; only the tiny finalize kernel remains
            nblk = ctypes.c_int(0)
            ws = norm_workspace(x.device)
            _call("mmfn_wino_output_stats_f32", ptr(Mt), ptr(out), ptr(ws), ctypes.cast(ctypes.pointer(nblk), ctypes.c_void_p), B, H, W, Co, st)
            mean, rstd, rm, rv, nbt, eps, momentum = bn
            _call("mmfn_bn_finalize_stats_f32", ptr(ws), nblk.value, B * H * W, Co, eps, momentum, ptr(mean), ptr(rstd), ptr(rm),
                  ptr(rv), ptr(nbt), st)
            return out, True
        _call("mmfn_wino_output_f32", ptr(Mt), ptr(res), ptr(out), B, H, W, Co, m, st)
    return (out, False) if bn is not None else out


def conv2d_fwd_bn_stats(x, w, stride, pad, out, mean, rstd, running_mean, running_var, nbt, eps, momentum, keep_v=None, keep_u=None,
                        u_ready=False, x_bn=None):
    """Training-mode conv followed by the BatchNorm batch statistics of its output (model_vec.py:509-593: every conv of the
    trunks is followed by a BatchNorm2d).  On the Winograd path the statistics are a by-product of the output transform.
    x_bn: see conv2d_winograd (the caller checked winograd_f4_ok)."""
    if winograd_ok(x.shape, w.shape, stride, pad, {}):
        _, fused = conv2d_winograd(x, w, out, keep_v=keep_v, keep_u=keep_u, u_ready=u_ready, x_bn=x_bn,
                                   bn=(mean, rstd, running_mean, running_var, nbt, eps, momentum))
        if fused:
            return out
    else:
        assert x_bn is None
        conv2d_fwd(x, w, stride, pad, out=out, keep_v=keep_v, keep_u=keep_u, u_ready=u_ready)
    C = out.shape[-1]
    M = out.numel() // C
    cq = C // 4
    if C % 4 or cq > 256 or 256 % cq == 0:
        bn_train_stats(out.view(M, C), mean, rstd, running_mean, running_var, nbt, eps, momentum)
        return out
    # The statistics kernels lane a block as 256 / (C / 4) rows x C / 4 float4 columns and refuse a width whose quad count does not
    # divide 256 (e.g. 96 channels, which the Winograd path accepts).  No layer of the model has one; such an output is copied into
    # the next width the kernel takes, zero columns appended, and the statistics of the real columns are copied back.
    Cp = 4 << (cq - 1).bit_length()
    xp = torch.zeros(M, Cp, dtype=out.dtype, device=out.device)
    xp[:, :C].copy_(out.view(M, C))
    meanp, rstdp = (torch.empty(Cp, dtype=torch.float32, device=out.device) for _ in range(2))
    rmp, rvp = (torch.zeros(Cp, dtype=torch.float32, device=out.device) for _ in range(2))
    rmp[:C].copy_(running_mean)
    rvp[:C].copy_(running_var)
    bn_train_stats(xp, meanp, rstdp, rmp, rvp, nbt, eps, momentum)
    for dst, src in ((mean, meanp), (rstd, rstdp), (running_mean, rmp), (running_var, rvp)):
        dst.copy_(src[:C])
    return out


def conv2d_fwd(x, w, stride, pad, out=None, keep_v=None, keep_u=None, u_ready=False, x_bn=None, **epi):
    """y[B,OH,OW,Cout] = conv(x[B,H,W,Cin], w[Cout,KH,KW,Cin]).  x_bn: see conv2d_winograd (the caller checked winograd_f4_ok)."""
    g, oshape = conv_geom(x.shape, w.shape, stride, pad)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=x.device)
    if winograd_ok(x.shape, w.shape, stride, pad, epi):
        assert epi.get("ldr", oshape[3]) == oshape[3]
        return conv2d_winograd(x, w, out, res=epi.get("res"), keep_v=keep_v, keep_u=keep_u, u_ready=u_ready, x_bn=x_bn)
    assert x_bn is None
    B, OH, OW, Cout = oshape
    K = g[6] * g[7] * g[2]
    return gemm(x, w, out, B * OH * OW, Cout, K, 0, K, Cout, A_IM2COL, B_NK, conv=g, **epi)


_wflip = {}
FLIPPED_DGRAD = True  # A/B switch (tools/gemm_bench.py)


def _flip_scratch(n, device):
    """Per-(device, lane) buffer for the flipped filter of the running dgrad (grow-only; sized before graph capture)."""
    key = (str(device), _lane)
    buf = _wflip.get(key)
    if buf is None or buf.numel() < n:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("flipped-filter scratch must be sized before graph capture")
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(max(n, 512 * 9 * 512), dtype=torch.float32, device=device)
        _wflip[key] = buf
    return buf


def conv2d_dgrad(dy, w, x_shape, stride, pad, out=None, **epi):
    """dx[B,H,W,Cin] from dy[B,OH,OW,Cout]."""
    g, oshape = conv_geom(x_shape, w.shape, stride, pad)
    assert tuple(dy.shape) == oshape
    if out is None:
        out = torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    Co, KH, KW, Ci = w.shape
    if FLIPPED_DGRAD and stride == 1 and KH == KW and 2 * pad == KH - 1 and Co % 16 == 0 and Ci % 4 == 0:
        # stride 1, "same" padding: dx = conv(dy, flip(w)^T) - the forward implicit GEMM with k-contiguous weights
        # runs ~15 % faster than the gather form below; the 0.1-9 MB filter transpose costs 2-4 us
        wt = _flip_scratch(w.numel(), dy.device)[:w.numel()].view(Ci, KH, KW, Co)
        _call("mmfn_conv_weight_flip_f32", ptr(w), ptr(wt), Co, KH * KW, Ci, stream())
        return conv2d_fwd(dy, wt, 1, pad, out=out, **epi)
    B, H, W, Cin = x_shape
    K = g[6] * g[7] * g[5]
    return gemm(dy, w, out, B * H * W, Cin, K, 0, 0, Cin, A_DGRAD, B_DGRADW, conv=g, **epi)


WINOGRAD_WGRAD = True


def winograd_wgrad_ok(x_shape, w_shape, stride, pad):
    # also in bf16 mode (where the forward is a direct convolution): the weight gradient then runs in the Winograd domain in
    # fp32, transforming x itself
    return (WINOGRAD_WGRAD and WINOGRAD_F4 and winograd_ok(x_shape, w_shape, stride, pad, {}, for_wgrad=True)
            and x_shape[1] % 4 == 0 and x_shape[2] % 4 == 0)


def conv2d_wgrad_winograd(dy, x, out, v=None):
    """Weight gradient of a 3x3 stride-1 'same' convolution in the F(4x4,3x3) domain: 36 [Co x tiles] x [tiles x Ci] GEMMs.
    v: the transformed input kept by the forward (conv2d_fwd(keep_v=...)); recomputed from x when absent."""
    B, H, W, Ci = x.shape
    Co = dy.shape[3]
    T = B * (H // 4) * (W // 4)
    buf = _wino_scratch(36 * (Co * Ci + T * Ci + T * Co), x.device)
    dU = buf[:36 * Co * Ci]
    V = buf[36 * Co * Ci:36 * (Co * Ci + T * Ci)]
    dMt = buf[36 * (Co * Ci + T * Ci):36 * (Co * Ci + T * Ci + T * Co)]
    st = stream()
    with _whole_op("wgrad %dx%d c%d->%d k3 s1 (winograd F4)" % (H, W, Ci, Co), 2.0 * B * H * W * Co * 9 * Ci,
                   4.0 * (B * H * W * (Ci + Co) + 9 * Co * Ci), 2.0 * 36 * T * Co * Ci), precision("f32"):
        _wgrad_winograd_body(dy, x, out, v, B, H, W, Ci, Co, T, dU, V, dMt, st)   # never rounded in the Winograd domain
    return out


def _wgrad_winograd_body(dy, x, out, v, B, H, W, Ci, Co, T, dU, V, dMt, st, bn=None):
    """out None (conv2d_bwd_winograd with a frozen filter): only the transformed output gradient, which the data gradient shares."""
    want_dw = out is not None
    if want_dw and v is not None:
        V = v.view(-1)[:36 * T * Ci]
    elif want_dw:
        _call("mmfn_wino_input_f32", ptr(x), ptr(V), B, H, W, Ci, 4, st)
    if bn is not None:
        g, ymask, co, mean, rstd, weight, relu_bias, means, ge_out = bn
        _call("mmfn_wino_outgrad_bn_f32", ptr(g), ptr(ymask), ptr(co), ptr(mean), ptr(rstd), ptr(weight), ptr(relu_bias), ptr(means),
              ptr(ge_out), ptr(dMt), B, H, W, Co, st)
    else:
        _call("mmfn_wino_outgrad_f32", ptr(dy), ptr(dMt), B, H, W, Co, st)
    if not want_dw:
        return None
    # the split-K combine of this GEMM (K = tiles: thousands) runs inside the output transform, which sums the slices as it reads
    info = {} if (WGRAD_SLABS and Ci % 64 == 0) else None
    gemm(dMt, V, dU, Co, Ci, T, Co, Ci, Ci, A_COLMAJOR, B_KN, batch=36, strideA=T * Co, strideB=T * Ci, strideC=Co * Ci, slab_info=info)
    if info is not None and info["splits"] > 1:
        _call("mmfn_wino_wgrad_out_slabs_f32", ptr(info["slabs"]), info["splits"], ptr(out), Co, Ci, st)
    else:
        _call("mmfn_wino_wgrad_out_f32", ptr(dU), ptr(out), Co, Ci, st)
    return out


WGRAD_SLABS = True   # False: a split-K combine launch per Winograd weight gradient (the test of the slab path compares both)
WINOGRAD_ADJOINT_DGRAD = True


def winograd_adjoint_ok(x_shape, w_shape, stride, pad):
    """The adjoint data gradient covers whatever the F(4x4,3x3) weight gradient covers (image sides multiples of 4)."""
    return WINOGRAD_ADJOINT_DGRAD and winograd_wgrad_ok(x_shape, w_shape, stride, pad)


def conv2d_bwd_winograd(dy, x, u, dw_out, dx_out, v=None, res=None, bn=None):
    """Weight AND data gradient of a 3x3 stride-1 'same' convolution in the F(4x4,3x3) domain, sharing the transformed
    output gradient dM = A dy A^T:
        dw = G^T [ sum_tiles dM^T . V ] G          (V = B^T x B, kept by the forward or recomputed)
        dx = overlap-add( B (dM . U) B^T ) (+ res)  (U = G w G^T, kept by the forward: the ADJOINT of the forward pipeline,
                                                     no flipped filter, no second filter / input transform)
    bn = (g, ymask or None, conv_out, mean, rstd, weight, relu_bias or None, means, ge_out or None), all NHWC / [C]: dy is then the
    BatchNorm backward of g (reductions already done by bn_bwd_reduce) formed on the fly inside the transform; the `dy` argument
    only gives the shape.  relu_bias (with ymask None): the ReLU mask is recomputed from conv_out (bn_bwd).
    x: the convolution's input, or - with v given - anything carrying its .shape.  dw_out None: no weight gradient (a frozen filter)."""
    B, H, W, Ci = x.shape
    Co = dy.shape[3]
    T = B * (H // 4) * (W // 4)
    buf = _wino_scratch(36 * (Co * Ci + T * Ci + T * Co), x.device)
    dU = buf[:36 * Co * Ci]
    Vs = buf[36 * Co * Ci:36 * (Co * Ci + T * Ci)]
    dMt = buf[36 * (Co * Ci + T * Ci):36 * (Co * Ci + T * Ci + T * Co)]
    st = stream()
    conv_flops = 2.0 * B * H * W * Co * 9 * Ci
    conv_bytes = 4.0 * (B * H * W * (Ci + Co) + 9 * Co * Ci)
    with _whole_op("wgrad %dx%d c%d->%d k3 s1 (winograd F4)" % (H, W, Ci, Co), conv_flops, conv_bytes, 2.0 * 36 * T * Co * Ci):
        _wgrad_winograd_body(dy, x, dw_out, v, B, H, W, Ci, Co, T, dU, Vs, dMt, st, bn=bn)
    with _whole_op("dgrad %dx%d c%d->%d k3 s1 (winograd F4 adjoint)" % (H, W, Ci, Co), conv_flops, conv_bytes, 2.0 * 36 * T * Co * Ci):
        dV = Vs  # the scratch V region is free again: with a kept V it was never used, otherwise the wgrad GEMM is done with it
        gemm(dMt, u.view(-1)[:36 * Co * Ci], dV, T, Ci, Co, Co, Ci, Ci, A_ROWMAJOR, B_KN, batch=36, strideA=T * Co, strideB=Co * Ci,
             strideC=T * Ci)
        _call("mmfn_wino_input_adjoint_f32", ptr(dV), ptr(res), ptr(dx_out), B, H, W, Ci, st)
    return dw_out, dx_out


def conv2d_wgrad(dy, x, w_shape, stride, pad, out=None, v=None, **epi):
    """dw[Cout,KH,KW,Cin] = sum over pixels of dy (x) im2col(x)."""
    g, oshape = conv_geom(x.shape, w_shape, stride, pad)
    assert tuple(dy.shape) == oshape
    if out is None:
        out = torch.empty(w_shape, dtype=torch.float32, device=dy.device)
    if not epi and winograd_wgrad_ok(x.shape, w_shape, stride, pad):
        return conv2d_wgrad_winograd(dy, x, out, v=v)
    B, OH, OW, Cout = oshape
    N = g[6] * g[7] * g[2]
    return gemm(dy, x, out, Cout, N, B * OH * OW, Cout, 0, N, A_COLMAJOR, B_IM2COL, conv=g, **epi)


# ---------------------------------------------------------------- small helpers
def _call(name, *args):
    check(getattr(lib(), name)(*args), name)


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


_norm_ws = {}


def norm_workspace(device, nbytes=None):
    """Scratch for norm / colsum / token-bwd reductions (grow-only, fp64-aligned), per (device, lane)."""
    key = (str(device), _lane)
    need = max(nbytes or 0, lib().mmfn_norm_workspace_bytes(1024) + 8192)
    buf = _norm_ws.get(key)
    if buf is None or buf.numel() * 8 < need:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("norm workspace must be sized before graph capture")
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(need // 8 + 1, dtype=torch.float64, device=device)
        _norm_ws[key] = buf
    return buf


def fill(t, value):
    _call("mmfn_fill_f32", ptr(t), float(value), t.numel(), stream())
    return t


def axpby(y, x, a=1.0, b=1.0):
    _call("mmfn_axpby_f32", ptr(y), ptr(x), float(a), float(b), y.numel(), stream())
    return y


# ---------------------------------------------------------------- BatchNorm / LayerNorm
def bn_train_stats(x2d, mean, rstd, running_mean, running_var, nbt, eps=1e-5, momentum=0.1):
    M, C = x2d.shape
    _call("mmfn_bn_train_stats_bf16" if x2d.dtype == BF16 else "mmfn_bn_train_stats_f32", ptr(x2d), M, C, eps, momentum, ptr(mean),
          ptr(rstd), ptr(running_mean), ptr(running_var), ptr(nbt), ptr(norm_workspace(x2d.device)), stream())


def bn_finalize_stats(partials, nblk, M, C, mean, rstd, running_mean, running_var, nbt, eps=1e-5, momentum=0.1):
    """Second half of bn_train_stats for producers that emit the per-block (sum, sum of squares) rows themselves (the bf16
    convolution's epilogue, ops16.conv2d_fwd(stats=...)): partials [nblk, 2, C] fp64."""
    _call("mmfn_bn_finalize_stats_f32", ptr(partials), nblk, M, C, eps, momentum, ptr(mean), ptr(rstd), ptr(running_mean),
          ptr(running_var), ptr(nbt), stream())


def bn_fold(w, gamma, beta, running_mean, running_var, eps, w_out, b_out):
    """Eval-mode BatchNorm folded into the convolution before it: w_out = w * s per output channel, b_out = beta - mean * s."""
    Cout = w.shape[0]
    _call("mmfn_bn_fold_f32", ptr(w), Cout, w.numel() // Cout, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(eps),
          ptr(w_out), ptr(b_out), stream())


def bn_eval_prepare(running_mean, running_var, mean, rstd, eps=1e-5):
    _call("mmfn_bn_eval_prepare_f32", ptr(running_mean), ptr(running_var), eps, mean.numel(), ptr(mean), ptr(rstd), stream())


def bn_apply(x2d, y2d, mean, rstd, weight, bias, relu, res=None):
    M, C = x2d.shape
    if y2d.dtype == BF16:   # x: the convolution output, bf16 or (stems) fp32
        _call("mmfn_bn_apply_bf16", ptr(x2d), 0 if x2d.dtype == BF16 else 1, ptr(res), ptr(y2d), M, C, ptr(mean), ptr(rstd),
              ptr(weight), ptr(bias), 1 if relu else 0, stream())
        return y2d
    _call("mmfn_bn_apply_f32", ptr(x2d), ptr(res), ptr(y2d), M, C, ptr(mean), ptr(rstd), ptr(weight), ptr(bias),
          1 if relu else 0, stream())
    return y2d


def bn_bwd(g2d, y2d, x2d, mean, rstd, weight, dx, dweight, dbias, ge_out=None, relu_bias=None):
    """relu_bias (the BatchNorm's bias) with y2d None: the ReLU mask is recomputed from x2d - the forward applied this BatchNorm
    inside its consumer's Winograd input transform and never wrote y (conv2d_winograd(x_bn=...))."""
    M, C = x2d.shape
    if g2d.dtype != BF16 and (x2d.dtype == BF16 or (y2d is not None and y2d.dtype == BF16)):
        raise TypeError("bn_bwd: fp32 output gradient with bf16 activations (every activation-side tensor of the bf16 mode is bf16)")
    if g2d.dtype == BF16:   # x / dx: bf16, or both fp32 (stems)
        assert dx.dtype == x2d.dtype
        _call("mmfn_bn_bwd_bf16", ptr(g2d), ptr(y2d), ptr(x2d), 0 if x2d.dtype == BF16 else 1, M, C, ptr(mean), ptr(rstd), ptr(weight),
              ptr(dx), ptr(ge_out), ptr(dweight), ptr(dbias), ptr(norm_workspace(x2d.device)), stream())
        return dx
    _call("mmfn_bn_bwd_f32", ptr(g2d), ptr(y2d), ptr(x2d), M, C, ptr(mean), ptr(rstd), ptr(weight), ptr(relu_bias), ptr(dx),
          ptr(ge_out), ptr(dweight), ptr(dbias), ptr(norm_workspace(x2d.device)), stream())
    return dx


def bn_bwd_reduce(g2d, y2d, x2d, mean, rstd, dweight, dbias, means, relu_wb=None):
    """The reductions of bn_bwd only (dweight, dbias, means[2][C]); conv2d_bwd_winograd(bn=...) applies them inside its
    output-gradient transform.  relu_wb = (weight, bias) with y2d None: the recomputed ReLU mask (bn_bwd)."""
    M, C = x2d.shape
    rw, rb = relu_wb if relu_wb is not None else (None, None)
    _call("mmfn_bn_bwd_reduce_f32", ptr(g2d), ptr(y2d), ptr(x2d), M, C, ptr(mean), ptr(rstd), ptr(rw), ptr(rb), ptr(dweight),
          ptr(dbias), ptr(means), ptr(norm_workspace(x2d.device)), stream())
    return means


ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


def layernorm_fwd(x, w, b, y, mean, rstd, act=ACT_NONE, eps=1e-5):
    """y bf16 (the bf16 mode): x bf16, or fp32 - the transformers' residual stream, which stays fp32 in that mode."""
    M, C = x.shape
    if y.dtype == BF16:
        _call("mmfn_layernorm_fwd_bf16", ptr(x), 0 if x.dtype == BF16 else 1, ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), M, C, eps, act,
              stream())
        return y
    _call("mmfn_layernorm_fwd_f32", ptr(x), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), M, C, eps, act, stream())
    return y


def layernorm_bwd(g, x, w, b, mean, rstd, dx, dw, db, act=ACT_NONE, dres=None, dx_dropped=None, drop_p=0.0, rng_state=None,
                  rng_stream=0, dx_colsum=None):
    """dx_dropped: optional second output dx * dropout keep-scale (the mask of the residual branch that consumes dx).
    dx_colsum: optional [C] output, column sums of dx_dropped (of dx without a dropped copy): the next bias gradient."""
    M, C = x.shape
    if g.dtype == BF16:   # the two halves separately (same kernels as the fused entry)
        rows = layernorm_bwd_rows(M)
        part = norm_workspace(x.device).view(torch.float32)[:rows * 3 * C].view(rows, 3, C)
        layernorm_bwd_partial(g, x, w, b, mean, rstd, dx, part, act, dres=dres, dx_dropped=dx_dropped, drop_p=drop_p,
                              rng_state=rng_state, rng_stream=rng_stream, want_colsum=dx_colsum is not None)
        layernorm_bwd_finalize(part, rows, C, dw, db, dx_colsum)
        return dx
    _call("mmfn_layernorm_bwd_drop_f32", ptr(g), ptr(x), ptr(w), ptr(b), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dw),
          ptr(db), M, C, act, ptr(dx_dropped), float(drop_p), ptr(rng_state), rng_stream, ptr(dx_colsum),
          ptr(norm_workspace(x.device)), stream())
    return dx


def layernorm_bwd_rows(M):
    return lib().mmfn_layernorm_bwd_rows(M)


def layernorm_bwd_partial(g, x, w, b, mean, rstd, dx, partials, act=ACT_NONE, dres=None, dx_dropped=None, drop_p=0.0,
                          rng_state=None, rng_stream=0, want_colsum=False):
    """First half of layernorm_bwd: dx (and dx_dropped) now, the row reductions as partial rows in `partials`
    ([layernorm_bwd_rows(M), 3 or 2, C] floats) for layernorm_bwd_finalize - which may run later, on another stream."""
    M, C = x.shape
    if g.dtype == BF16:
        # bf16 mode: g and the dropped copy are GEMM operands (bf16); x / dres / dx are bf16 too, or - inside the fusion transformers -
        # the fp32 residual stream and its gradient
        f32_stream = x.dtype == torch.float32
        assert dx.dtype == x.dtype and (dres is None or dres.dtype == x.dtype) and (dx_dropped is None or dx_dropped.dtype == BF16)
        _call("mmfn_layernorm_bwd_partial_bf16", ptr(g), ptr(x), 1 if f32_stream else 0, ptr(w), ptr(b), ptr(mean), ptr(rstd), ptr(dres),
              ptr(dx), M, C, act, ptr(dx_dropped), float(drop_p), ptr(rng_state), rng_stream, 1 if want_colsum else 0, ptr(partials),
              stream())
        return dx
    _call("mmfn_layernorm_bwd_partial_f32", ptr(g), ptr(x), ptr(w), ptr(b), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), M, C, act,
          ptr(dx_dropped), float(drop_p), ptr(rng_state), rng_stream, 1 if want_colsum else 0, ptr(partials), stream())
    return dx


def layernorm_bwd_finalize(partials, rows, C, dw, db, dx_colsum=None):
    _call("mmfn_layernorm_bwd_finalize_f32", ptr(partials), rows, C, ptr(dw), ptr(db), ptr(dx_colsum), stream())


def layernorm_finalize_table(entries, device):
    """Device pointer table for layernorm_bwd_finalize_batched: entries = [(partials, dw, db, dx_colsum or None), ...]."""
    flat = []
    for part, dw, db, cs in entries:
        flat += [part.data_ptr(), dw.data_ptr(), db.data_ptr(), 0 if cs is None else cs.data_ptr()]
    return torch.tensor(flat, dtype=torch.int64).to(device)


def layernorm_bwd_finalize_batched(table, n, rows, C):
    _call("mmfn_layernorm_bwd_finalize_batched_f32", ptr(table), n, rows, C, stream())


def colsum(x2d, out, M=None, C=None, ld=None):
    M = x2d.shape[0] if M is None else M
    C = x2d.shape[1] if C is None else C
    ld = x2d.stride(0) if ld is None else ld
    need = lib().mmfn_colsum_workspace_bytes(M, C)
    _call("mmfn_colsum_bf16" if x2d.dtype == BF16 else "mmfn_colsum_f32", ptr(x2d), M, C, ld, ptr(out),
          ptr(norm_workspace(x2d.device, need)), stream())
    return out


def maxpool_fwd(x, y, idx):
    B, H, W, C = x.shape
    _call("mmfn_maxpool3x3s2_fwd_bf16" if x.dtype == BF16 else "mmfn_maxpool3x3s2_fwd_f32", ptr(x), ptr(y), ptr(idx), B, H, W, C, stream())
    return y


def maxpool_bwd(gy, idx, gx):
    B, H, W, C = gx.shape
    _call("mmfn_maxpool3x3s2_bwd_bf16" if gy.dtype == BF16 else "mmfn_maxpool3x3s2_bwd_f32", ptr(gy), ptr(idx), ptr(gx), B, H, W, C, stream())
    return gx


def stem_pool_ok(co_shape, dtype=torch.float32):
    """Do stem_bn_relu_maxpool / stem_bn_bwd_pooled take a stem whose convolution output is co_shape [B,H,W,C]?  (fp32, even
    extents; anything else keeps bn_apply + maxpool_fwd and maxpool_bwd + bn_bwd.)"""
    B, H, W, C = co_shape
    return dtype == torch.float32 and lib().mmfn_stem_pool_ok(B, H, W, C) == 1


def stem_bn_relu_maxpool(co, mean, rstd, weight, bias, pooled, idx):
    """pooled, idx = maxpool3x3s2(relu(bn(co))) in one pass; relu(bn(co)) is never written."""
    B, H, W, C = co.shape
    _call("mmfn_stem_bn_relu_maxpool_fwd_f32", ptr(co), ptr(mean), ptr(rstd), ptr(weight), ptr(bias), ptr(pooled), ptr(idx), B, H, W, C,
          stream())
    return pooled


def stem_bn_bwd_pooled(g, idx, co, mean, rstd, weight, bias, dco, dweight, dbias):
    """bn_bwd of the stem fed by the POOLED gradient g [B,H/2,W/2,C]: maxpool_bwd and the ReLU mask happen in the loaders."""
    B, H, W, C = co.shape
    _call("mmfn_stem_bn_bwd_pooled_f32", ptr(g), ptr(idx), ptr(co), B, H, W, C, ptr(mean), ptr(rstd), ptr(weight), ptr(bias), ptr(dco),
          ptr(dweight), ptr(dbias), ptr(norm_workspace(co.device)), stream())
    return dco


def _frames(frames, n):
    """Host int32[n] of frames per sample for each modality (None: one each - seq_len = n_views = 1)."""
    if frames is None:
        return None
    if len(frames) != n or min(frames) < 1:
        raise ValueError("frames must hold one positive count per modality, got %r for %d modalities" % (frames, n))
    return (ctypes.c_int32 * n)(*[int(f) for f in frames])


def tokens_fwd(feats, pos, vel_w, vel_b, velocity, tok, drop_p=0.0, rng_state=None, rng_stream=0, frames=None):
    """feats[m] is [B * frames[m], S, S, C]; tok is [B, sum(frames) * 64, C]."""
    B = tok.shape[0]
    _, S, _, C = feats[0].shape
    for m, f in enumerate(feats):
        if f.shape[0] != B * (1 if frames is None else frames[m]):
            raise ValueError("modality %d holds %d frames for %d samples, expected %d per sample" % (m, f.shape[0], B, 1 if frames is None else frames[m]))
    if tok.shape[1] != 64 * (len(feats) if frames is None else sum(frames)):
        raise ValueError("token buffer has %d tokens, the frames need %d" % (tok.shape[1], 64 * (len(feats) if frames is None else sum(frames))))
    arr = _ptr_array(feats)
    if feats[0].dtype == BF16:   # bf16 features; the token matrix bf16 or (the transformers' residual stream) fp32
        _call("mmfn_tokens_fwd_bf16", arr, len(feats), _frames(frames, len(feats)), B, S, C, ptr(pos), ptr(vel_w), ptr(vel_b), ptr(velocity),
              ptr(tok), 0 if tok.dtype == BF16 else 1, float(drop_p), ptr(rng_state), rng_stream, stream())
        return tok
    _call("mmfn_tokens_fwd_f32", arr, len(feats), _frames(frames, len(feats)), B, S, C, ptr(pos), ptr(vel_w),
          ptr(vel_b), ptr(velocity), ptr(tok), float(drop_p), ptr(rng_state), rng_stream, stream())
    return tok


def tokens_bwd(gtok, velocity, dpos, dvel_w, dvel_b, drop_p=0.0, rng_state=None, rng_stream=0):
    B, T, C = gtok.shape
    need = lib().mmfn_tokens_bwd_workspace_bytes(T, C)
    _call("mmfn_tokens_bwd_bf16" if gtok.dtype == BF16 else "mmfn_tokens_bwd_f32", ptr(gtok), B, T, C, ptr(velocity), ptr(dpos), ptr(dvel_w), ptr(dvel_b), float(drop_p),
          ptr(rng_state), rng_stream, ptr(norm_workspace(gtok.device, need)), stream())


def _groups_ok(n_img, n_tok, T, m, frames):
    if frames < 1 or n_img != n_tok * frames or (m + frames) * 64 > T:
        raise ValueError("%d frames / %d samples / %d tokens do not fit token groups [%d, %d)" % (n_img, n_tok, T, m, m + frames))


def upsample_add_fwd(feat, tok, out, m, frames=1):
    """m: the modality's first token group, frames: its frames per sample (feat holds samples * frames maps)."""
    B, S, _, C = feat.shape
    T = tok.shape[1]
    _groups_ok(B, tok.shape[0], T, m, frames)
    _call("mmfn_upsample_add_fwd_bf16" if feat.dtype == BF16 else "mmfn_upsample_add_fwd_f32", ptr(feat), ptr(tok), ptr(out), B, S, C, T, m, frames, stream())
    return out


def upsample_adj(G, gtok, m, frames=1):
    B, S, _, C = G.shape
    T = gtok.shape[1]
    _groups_ok(B, gtok.shape[0], T, m, frames)
    _call("mmfn_upsample_adj_bf16" if G.dtype == BF16 else "mmfn_upsample_adj_f32", ptr(G), ptr(gtok), B, S, C, T, m, frames, stream())


def pool_bcast_add(G, gtok, dF, m, frames=1):
    B, S, _, C = G.shape
    T = gtok.shape[1]
    _groups_ok(B, gtok.shape[0], T, m, frames)
    if G.dtype == BF16:   # the token gradient bf16 or (the transformers' fp32 residual stream) fp32
        _call("mmfn_pool_bcast_add_bf16", ptr(G), ptr(gtok), 0 if gtok.dtype == BF16 else 1, ptr(dF), B, S, C, T, m, frames, stream())
        return dF
    _call("mmfn_pool_bcast_add_f32", ptr(G), ptr(gtok), ptr(dF), B, S, C, T, m, frames, stream())
    return dF


def gap_sum_fwd(feats, out, frames=None):
    """out[B, C] = sum over modalities and over each sample's frames of the spatial mean."""
    _, H, W, C = feats[0].shape
    B = out.shape[0]
    _call("mmfn_gap_sum_fwd_bf16" if feats[0].dtype == BF16 else "mmfn_gap_sum_fwd_f32", _ptr_array(feats), len(feats), _frames(frames, len(feats)), B, H * W, C,
          ptr(out), stream())
    return out


def gap_sum_bwd(g, outs, frames=None):
    _, H, W, C = outs[0].shape
    B = g.shape[0]
    _call("mmfn_gap_sum_bwd_bf16" if outs[0].dtype == BF16 else "mmfn_gap_sum_bwd_f32", ptr(g), _ptr_array(outs), len(outs), _frames(frames, len(outs)), B, H * W, C,
          stream())


def transpose(inp, out, B, R, Cc):
    name = {(torch.float32, torch.float32): "mmfn_transpose_f32", (torch.float32, BF16): "mmfn_transpose_f32_to_bf16",
            (BF16, torch.float32): "mmfn_transpose_bf16_to_f32"}[(inp.dtype, out.dtype)]
    _call(name, ptr(inp), ptr(out), B, R, Cc, stream())
    return out


# ---------------------------------------------------------------- attention
def attention_fwd(q, k, v, ld, o, ldo, lse, B, T, NH, HS, scale, kv_len=None, drop_p=0.0, rng_state=None, rng_stream=0):
    _call("mmfn_attention_fwd_bf16" if q.dtype == BF16 else "mmfn_attention_fwd_f32", ptr(q), ptr(k), ptr(v), ld, ptr(o), ldo, ptr(lse), B, T, NH, HS, float(scale),
          ptr(kv_len), float(drop_p), ptr(rng_state), rng_stream, stream())
    return o


def attention_bwd(q, k, v, ld, o, dO, ldo, lse, delta, dq, dk, dv, ldg, B, T, NH, HS, scale, kv_len=None, drop_p=0.0,
                  rng_state=None, rng_stream=0):
    _call("mmfn_attention_bwd_bf16" if q.dtype == BF16 else "mmfn_attention_bwd_f32", ptr(q), ptr(k), ptr(v), ld, ptr(o), ptr(dO), ldo, ptr(lse), ptr(delta), ptr(dq),
          ptr(dk), ptr(dv), ldg, B, T, NH, HS, float(scale), ptr(kv_len), float(drop_p), ptr(rng_state), rng_stream, stream())


# ---------------------------------------------------------------- fused GPT block (narrow fusion transformers)
GPT_ROWS = 32   # token rows per workgroup of the row-block kernels = rows per LayerNorm partial row
# bf16 mode: the fields of mmfn_gpt_block_desc that are bf16 (GEMM operands in HBM and the weight shadows); everything else stays fp32
GPT_BF16_FIELDS = frozenset(("wqkv", "wproj", "w1", "w2", "a", "qkv", "o", "a2", "h", "gd", "gh", "gd2", "go", "dqkv", "gd_below"))


def gpt_block_supported(C, NH, T):
    return lib().mmfn_gpt_block_supported(C, NH, T) == 0


def gpt_block_rows_supported(C, T):
    return lib().mmfn_gpt_block_rows_supported(C, T) == 0


def gpt_block_desc(B, T, C, NH, eps=1e-5, attn_pdrop=0.0, resid_pdrop=0.0, rng_state=None, rng_stream=0, rng_stream_below=0,
                   below_colsum=False, **tensors):
    """mmfn_gpt_block_desc (include/mmfn_hip.h): tensors by field name (contiguous); missing fields stay NULL.  fp32 everywhere on the
    fp32 path; in the bf16 mode the GEMM operands (GPT_BF16_FIELDS, and the weight shadows) are bf16.  The returned structure
    keeps its tensors alive and remembers whether it describes the bf16 mode (`d.bf16`)."""
    d = GptBlockDesc()
    bf16 = False
    for name, t in tensors.items():
        if name not in GptBlockDesc._PTRS:
            raise KeyError(name)
        if t is not None:
            assert t.is_contiguous(), name
            if t.dtype == BF16:
                assert name in GPT_BF16_FIELDS, name
                bf16 = True
            else:
                assert t.dtype == torch.float32, name
        setattr(d, name, ptr(t))
    if bf16:   # a descriptor is all-fp32 or has every operand it names in bf16
        assert all(t is None or t.dtype == BF16 for n, t in tensors.items() if n in GPT_BF16_FIELDS), "mixed operand precisions"
    d.bf16 = bf16
    d.rng_state = ptr(rng_state)
    d.B, d.T, d.C, d.NH = B, T, C, NH
    d.attn_pdrop, d.resid_pdrop, d.eps = float(attn_pdrop), float(resid_pdrop), float(eps)
    d.rng_stream, d.rng_stream_below, d.below_colsum = rng_stream, rng_stream_below, 1 if below_colsum else 0
    d._keep = (tensors, rng_state)
    return d


def gpt_block_attn_fwd(d):
    """ln1 -> key / query / value -> attention of one transformer block, one launch (model_vec.py:96-105,126).  fp32 path only."""
    assert not d.bf16
    _call("mmfn_gpt_block_attn_fwd_f32", ctypes.addressof(d), stream())


def gpt_block_mlp_fwd(d):
    """proj (+ residual) -> ln2 -> mlp.0 -> ReLU -> mlp.2 (+ residual) of one transformer block, one launch (model_vec.py:107-108,126-131)."""
    _call("mmfn_gpt_block_mlp_fwd_bf16" if d.bf16 else "mmfn_gpt_block_mlp_fwd_f32", ctypes.addressof(d), stream())


def gpt_block_bwd_rows(upper, lower):
    """The row-local backward between two attention backward passes: upper block's qkv dgrad + ln1 backward, lower block's mlp /
    ln2 / proj dgrads.  Either may be None."""
    bf16 = (upper if upper is not None else lower).bf16
    assert upper is None or lower is None or upper.bf16 == lower.bf16
    _call("mmfn_gpt_block_bwd_rows_bf16" if bf16 else "mmfn_gpt_block_bwd_rows_f32", None if upper is None else ctypes.addressof(upper),
          None if lower is None else ctypes.addressof(lower), stream())


def lane0_attention_fwd(qkv, kv_len, B, L, heads, head_dim, scale, att0, prob):
    """VectorNet lane attention for query 0 only (the only row the encoder consumes): any number of lanes."""
    _call("mmfn_lane0_attention_fwd_f32", ptr(qkv), ptr(kv_len), B, L, heads, head_dim, float(scale), ptr(att0), ptr(prob), stream())
    return att0


def lane0_attention_bwd(qkv, prob, g_att0, kv_len, B, L, heads, head_dim, scale, dqkv):
    _call("mmfn_lane0_attention_bwd_f32", ptr(qkv), ptr(prob), ptr(g_att0), ptr(kv_len), B, L, heads, head_dim, float(scale),
          ptr(dqkv), stream())
    return dqkv


# ---------------------------------------------------------------- head / optimizer / ingest / vectornet
def gru_head_fwd(z0, target, w_ih, w_hh, b_ih, b_hh, w_out, b_out, gt, pred, hs, gates, xin, loss_terms, loss, steps):
    B = z0.shape[0]
    _call("mmfn_gru_head_fwd_f32", ptr(z0), ptr(target), ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(w_out), ptr(b_out),
          ptr(gt), ptr(pred), ptr(hs), ptr(gates), ptr(xin), ptr(loss_terms), ptr(loss), B, steps, stream())


def gru_head_bwd(pred, gt, dpred, gscale, w_ih, w_hh, w_out, hs, gates, xin, dz0, part, steps):
    B = dz0.shape[0]
    _call("mmfn_gru_head_bwd_f32", ptr(pred), ptr(gt), ptr(dpred), float(gscale), ptr(w_ih), ptr(w_hh), ptr(w_out), ptr(hs),
          ptr(gates), ptr(xin), ptr(dz0), ptr(part), B, steps, stream())


def gru_head_fwd_loss(z0, target, w_ih, w_hh, b_ih, b_hh, w_out, b_out, gt, pred, hs, gates, xin, loss_terms, loss, kind, loss_table,
                      sample_weight, l1_terms, steps):
    """gru_head_fwd with the objective as a parameter (losses.WaypointLoss): kind = MMFN_LOSS_*, loss_table = 16 device floats
    (beta / delta, horizon weights), sample_weight [B] or None, l1_terms [B] or None."""
    B = z0.shape[0]
    _call("mmfn_gru_head_fwd_loss_f32", ptr(z0), ptr(target), ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(w_out), ptr(b_out),
          ptr(gt), ptr(pred), ptr(hs), ptr(gates), ptr(xin), ptr(loss_terms), ptr(loss), int(kind), ptr(loss_table),
          ptr(sample_weight), ptr(l1_terms), B, steps, stream())


def gru_head_bwd_loss(pred, gt, gscale, w_ih, w_hh, w_out, hs, gates, xin, dz0, part, kind, loss_table, sample_weight, steps):
    B = dz0.shape[0]
    _call("mmfn_gru_head_bwd_loss_f32", ptr(pred), ptr(gt), float(gscale), ptr(w_ih), ptr(w_hh), ptr(w_out), ptr(hs), ptr(gates),
          ptr(xin), ptr(dz0), ptr(part), int(kind), ptr(loss_table), ptr(sample_weight), B, steps, stream())


def step_advance(step, ok=None):
    """step += 1; ok: the non-finite guard's device flag (int32), only when it is set."""
    if ok is not None:
        _call("mmfn_step_advance_if", ptr(step), ptr(ok), stream())
        return
    _call("mmfn_step_advance", ptr(step), stream())


def rng_advance(state):
    _call("mmfn_rng_advance", ptr(state), stream())


def adamw(p, g, m, v, step, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, grad_scale=1.0, n=None):
    n = p.numel() if n is None else n
    _call("mmfn_adamw_f32", ptr(p), ptr(g), ptr(m), ptr(v), n, lr, beta1, beta2, eps, weight_decay, ptr(step),
          float(grad_scale), stream())


AVG_EMA, AVG_SWA = 0, 1   # mirror include/mmfn_hip.h


def weight_average(avg, src, n_averaged, ema_weight, mode, ok=None):
    """avg = src (first update: *n_averaged == 0) or ATen's lerp(avg, src, w) over avg.numel() floats; w = *ema_weight (EMA) or
    1 / (*n_averaged + 1) (SWA), both read on the device.  Does not advance n_averaged.  ok: the non-finite guard's device flag."""
    if src.numel() < avg.numel():
        raise ValueError("source holds %d floats, the average %d" % (src.numel(), avg.numel()))
    if ok is not None:
        _call("mmfn_weight_average_if_f32", ptr(avg), ptr(src), avg.numel(), ptr(n_averaged), ptr(ema_weight), int(mode), ptr(ok),
              stream())
        return
    _call("mmfn_weight_average_f32", ptr(avg), ptr(src), avg.numel(), ptr(n_averaged), ptr(ema_weight), int(mode), stream())


ADAMW_COEF, ADAMW_AVG, ADAMW_GUARD, ADAMW_MASK = 1, 2, 4, 8   # mirror include/mmfn_hip.h
ADAMW_FROZEN = 255   # group_of byte of a float4 that belongs to a frozen parameter (ADAMW_MASK)


def adamw_max_blocks():
    """The grid cap of the grouped / rows AdamW launches: beyond 1024 * this many floats their grid-stride loops go round again."""
    return int(lib().mmfn_adamw_max_blocks())


ADAMW_MAX_ROWS = 254   # mirror include/mmfn_hip.h


def _check_vmax(vmax, p, n):
    if vmax.dtype != torch.float32 or vmax.device != p.device or vmax.numel() < n:
        raise ValueError("vmax (max_exp_avg_sq) is a float32 tensor on the parameters' device with one entry per parameter of the range")


def _check_momentum_buffer(buf, p, n):
    if buf is None or buf.dtype != torch.float32 or buf.device != p.device or buf.numel() < n:
        raise ValueError("buf (momentum_buffer) is a float32 tensor on the parameters' device with one entry per parameter of the range")


# What the four fronts of the step family (adamw_groups / adamw_rows / sgd_groups / sgd_rows) share; rule: "AdamW" or "SGD", the
# word their error messages name the launch by.
def _check_group_table(rule, group_of, n):
    if group_of is None or group_of.dtype != torch.uint8 or group_of.numel() * 4 < n:
        raise ValueError("the masked %s launch needs a uint8 group table with one byte per float4 of the range" % rule)


def _check_rows(rule, row_of, rows, class_steps, n_classes, n):
    if row_of is None or row_of.dtype != torch.uint8 or row_of.numel() * 4 < n:
        raise ValueError("the %s launch with step classes needs a uint8 row table with one byte per float4 of the range" % rule)
    if rows.device.type != "cpu" or rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 2 or not rows.is_contiguous():
        raise ValueError("rows is a contiguous CPU int32 tensor [n_rows, 2] of (group, class)")
    if not 1 <= rows.shape[0] <= ADAMW_MAX_ROWS:
        raise ValueError("%d (group, step class) rows: the %s launch holds at most %d" % (rows.shape[0], rule, ADAMW_MAX_ROWS))
    if class_steps.dtype != torch.int64 or class_steps.numel() < n_classes:
        raise ValueError("class_steps holds %d %s counters, the launch reads %d int64" % (class_steps.numel(), class_steps.dtype, n_classes))


def _avg_args(avg, n):
    """The average's four C arguments from the fronts' avg tuple (None: no average)."""
    a, n_averaged, ema_weight, mode = (None, None, None, 0) if avg is None else avg
    if a is not None and a.numel() < n:
        raise ValueError("average holds %d floats, the step covers %d" % (a.numel(), n))
    return ptr(a), ptr(n_averaged), ptr(ema_weight), int(mode)


def _step_variant(rule, coef, avg, ok, mask=False):
    if ok is not None and coef is None:
        raise ValueError("the guarded %s launch is the coefficient instance: pass coef" % rule)
    variant = sum(bit for bit, arg in ((ADAMW_COEF, coef), (ADAMW_AVG, avg), (ADAMW_GUARD, ok)) if arg is not None)
    return variant | ADAMW_MASK if mask else variant


def adamw_groups(p, g, m, v, step, hyper, n_groups, group_of=None, n=None, coef=None, avg=None, ok=None, mask=False, vmax=None):
    """AdamW with the hyper-parameter rows (and optional per-float4 group ids) in device memory.  coef: a device scalar that
    multiplies every group's grad_scale (the clip coefficient).  avg: (avg, n_averaged, ema_weight, mode), every new parameter is
    also folded into avg[0, n) as weight_average does.  ok (with coef): the non-finite guard's device flag (int32), the launch
    touches nothing when it is 0.  mask: float4s whose group_of byte is ADAMW_FROZEN keep p / m / v untouched (an average is still
    updated from p); group_of is then mandatory, also with one group.  vmax: the amsgrad launch (mmfn_adamw_groups_ams_f32) - the
    running maximum of v, read and written for the groups whose hyper row has a non-zero last float; None: the launch without."""
    n = p.numel() if n is None else n
    if mask:
        _check_group_table("AdamW", group_of, n)
    avg_args = _avg_args(avg, n)
    variant = _step_variant("AdamW", coef, avg, ok, mask)
    if vmax is not None:
        _check_vmax(vmax, p, n)
        _call("mmfn_adamw_groups_ams_f32", ptr(p), ptr(g), ptr(m), ptr(v), ptr(vmax), n, ptr(group_of), ptr(hyper), n_groups, ptr(step),
              variant, ptr(coef), *avg_args, ptr(ok), stream())
        return
    _call("mmfn_adamw_groups_f32", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(group_of), ptr(hyper), n_groups, ptr(step), variant,
          ptr(coef), *avg_args, ptr(ok), stream())


def adamw_rows(p, g, m, v, class_steps, n_classes, hyper, n_groups, row_of, rows, n=None, coef=None, avg=None, ok=None, vmax=None):
    """AdamW with per-tensor step counts: row_of (uint8, one byte per float4, ADAMW_FROZEN over frozen float4s) selects a row of
    `rows` (a CPU int32 tensor [n_rows, 2] of (hyper group, step class)); a row's bias corrections come from class_steps[class]
    (int64, device).  coef / avg / ok / vmax as in adamw_groups; frozen float4s as in its masked launch."""
    n = p.numel() if n is None else n
    _check_rows("AdamW", row_of, rows, class_steps, n_classes, n)
    avg_args = _avg_args(avg, n)
    variant = _step_variant("AdamW", coef, avg, ok)
    if vmax is not None:
        _check_vmax(vmax, p, n)
        _call("mmfn_adamw_rows_ams_f32", ptr(p), ptr(g), ptr(m), ptr(v), ptr(vmax), n, ptr(row_of), ptr(hyper), n_groups, rows.data_ptr(),
              rows.shape[0], ptr(class_steps), n_classes, variant, ptr(coef), *avg_args, ptr(ok), stream())
        return
    _call("mmfn_adamw_rows_f32", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(row_of), ptr(hyper), n_groups, rows.data_ptr(), rows.shape[0],
          ptr(class_steps), n_classes, variant, ptr(coef), *avg_args, ptr(ok), stream())


def sgd_groups(p, g, buf, step, hyper, n_groups, group_of=None, n=None, coef=None, avg=None, ok=None, mask=False):
    """torch.optim.SGD with the hyper-parameter rows (lr, momentum, dampening, nesterov, weight_decay, grad_scale) in device memory:
    mmfn_sgd_groups_f32.  buf: the momentum buffer; *step == 1 makes this the first step (buf = d).  group_of / coef / avg / ok /
    mask as in adamw_groups."""
    n = p.numel() if n is None else n
    _check_momentum_buffer(buf, p, n)
    if mask:
        _check_group_table("SGD", group_of, n)
    avg_args = _avg_args(avg, n)
    _call("mmfn_sgd_groups_f32", ptr(p), ptr(g), ptr(buf), n, ptr(group_of), ptr(hyper), n_groups, ptr(step),
          _step_variant("SGD", coef, avg, ok, mask), ptr(coef), *avg_args, ptr(ok), stream())


def sgd_rows(p, g, buf, class_steps, n_classes, hyper, n_groups, row_of, rows, n=None, coef=None, avg=None, ok=None):
    """torch.optim.SGD with per-tensor step counts (mmfn_sgd_rows_f32): a row's class counter at 1 makes this the first step of
    the row's tensors.  row_of / rows / class_steps as in adamw_rows; coef / avg / ok as in sgd_groups."""
    n = p.numel() if n is None else n
    _check_momentum_buffer(buf, p, n)
    _check_rows("SGD", row_of, rows, class_steps, n_classes, n)
    avg_args = _avg_args(avg, n)
    _call("mmfn_sgd_rows_f32", ptr(p), ptr(g), ptr(buf), n, ptr(row_of), ptr(hyper), n_groups, rows.data_ptr(), rows.shape[0],
          ptr(class_steps), n_classes, _step_variant("SGD", coef, avg, ok), ptr(coef), *avg_args, ptr(ok), stream())



def class_steps_advance(class_steps, active, n_classes, ok=None):
    """class_steps[c] += 1 for every class c < n_classes whose byte in `active` (uint8, device) is set; ok: the guard's flag."""
    if class_steps.dtype != torch.int64 or active.dtype != torch.uint8 or min(class_steps.numel(), active.numel()) < n_classes:
        raise ValueError("class_steps (int64) and active (uint8) hold one entry per class")
    _call("mmfn_class_steps_advance", ptr(class_steps), ptr(active), n_classes, ptr(ok), stream())


ACCUM_NONE, ACCUM_ADD, ACCUM_FOLD = 0, 1, 2   # mirror include/mmfn_hip.h


def grad_accum_blocks(n):
    """fp64 partial slots a grad_accum call over n floats writes (fixed per n)."""
    return int(lib().mmfn_grad_accum_blocks(int(n)))


def grad_accum(g, acc, mode, partials=None):
    """ADD: acc += g;  FOLD: g += acc, acc = 0;  NONE: read g.  `partials`: a float64 view of grad_accum_blocks(g.numel())
    slots that receives one sum of squares of g (as it leaves) per workgroup."""
    if partials is not None and partials.numel() < grad_accum_blocks(g.numel()):
        raise ValueError("partials view holds %d slots, the pass writes %d" % (partials.numel(), grad_accum_blocks(g.numel())))
    _call("mmfn_grad_accum_f32", ptr(g), ptr(acc), g.numel(), int(mode), ptr(partials), stream())


def grad_norm_finalize(partials, scale, max_norm, norm, coef=None, ok=None, skipped=None):
    """norm = scale * sqrt(sum(partials)), coef = min(1, max_norm / (norm + 1e-6)); scale / max_norm / norm / coef: one-element
    device float tensors (views).  ok (int32 [1]), skipped (int64 [1]): the finalize also decides the step, ok = isfinite(norm),
    skipped += 1 when not (coef required)."""
    if ok is not None:
        _call("mmfn_grad_norm_finalize_guard", ptr(partials), partials.numel(), ptr(scale), ptr(max_norm), ptr(norm), ptr(coef),
              ptr(ok), ptr(skipped), stream())
        return
    _call("mmfn_grad_norm_finalize", ptr(partials), partials.numel(), ptr(scale), ptr(max_norm), ptr(norm), ptr(coef), stream())


def copy_if(dst, src, flag, when):
    """dst = src (same dtype and size, contiguous) when (flag != 0) == bool(when); flag: a device int32."""
    if dst.dtype != src.dtype or dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()):
        raise ValueError("copy_if takes two contiguous tensors of one dtype and size")
    _call("mmfn_copy_if", ptr(dst), ptr(src), dst.numel() * dst.element_size(), ptr(flag), 1 if when else 0, stream())


def tensor_stats_table(ranges, device):
    """The device table of tensor_stats for [(offset, count), ...] (float offsets into a flat buffer, multiples of 4):
    {"table": int64 [n, 3] of (offset, count, first chunk), "n_chunks", "limit": the floats the buffer must hold}."""
    chunk = int(lib().mmfn_tensor_stats_chunk())
    rows, first, limit = [], 0, 0
    for off, n in ranges:
        if n < 1 or off % 4 or off < 0:
            raise ValueError("tensor_stats ranges are (offset %% 4 == 0, count >= 1), got (%d, %d)" % (off, n))
        rows.append((off, n, first))
        first += (n + chunk - 1) // chunk
        limit = max(limit, off + n)
    if not rows:
        raise ValueError("tensor_stats needs at least one range")
    return {"table": torch.tensor(rows, dtype=torch.int64).to(device), "n_chunks": first, "limit": limit}


def fill_ranges_table(ranges, device):
    """The device table of fill_ranges for [(offset, count), ...], offsets and counts multiples of 4 floats, no overlap:
    tensor_stats_table's format."""
    ranges = sorted(ranges)
    for (off, n), nxt in zip(ranges, ranges[1:] + [None]):
        if n % 4 or (nxt is not None and off + n > nxt[0]):
            raise ValueError("fill_ranges ranges are whole float4s that do not overlap, got (%d, %d)" % (off, n))
    return tensor_stats_table(ranges, device)


def fill_ranges(flat, tab, value=0.0):
    """flat[offset:offset + count] = value over every range of `tab` (fill_ranges_table) in one launch."""
    if flat.dtype != torch.float32 or flat.numel() < tab["limit"] or not flat.is_contiguous():
        raise ValueError("the table covers %d floats, the buffer holds %d %s" % (tab["limit"], flat.numel(), flat.dtype))
    _call("mmfn_fill_ranges_f32", ptr(flat), ptr(tab["table"]), tab["table"].shape[0], tab["n_chunks"], float(value), stream())


def nonfinite_slot(x, slot):
    """slot (a one-element float64 view) = NaN when any entry of the fp32 tensor x is not finite, else 0.0."""
    if x.dtype != torch.float32 or slot.dtype != torch.float64 or slot.numel() != 1 or not x.is_contiguous():
        raise ValueError("nonfinite_slot takes a contiguous fp32 tensor and one float64 slot")
    _call("mmfn_nonfinite_slot_f32", ptr(x), x.numel(), ptr(slot), stream())


def tensor_stats(flat, tab, scale=1.0):
    """Per-tensor (|scale| * L2 norm, |scale| * max |x| over the finite entries, count of non-finite entries) of the ranges of
    `tab` (tensor_stats_table) in the fp32 buffer `flat`: float64 [n, 3] on the device, deterministic, no host sync."""
    if flat.dtype != torch.float32 or flat.numel() < tab["limit"]:
        raise ValueError("the table covers %d floats, the buffer holds %d %s" % (tab["limit"], flat.numel(), flat.dtype))
    n = tab["table"].shape[0]
    out = torch.empty(n, 3, dtype=torch.float64, device=flat.device)
    workspace = torch.empty(3 * tab["n_chunks"], dtype=torch.float64, device=flat.device)
    _call("mmfn_tensor_stats_f32", ptr(flat), ptr(tab["table"]), n, tab["n_chunks"], float(scale), ptr(out), ptr(workspace), stream())
    return out


def ingest_rgb_u8(img_u8, out, crop=256):
    B, H, W, _ = img_u8.shape
    _call("mmfn_ingest_rgb_u8", ptr(img_u8), ptr(out), B, H, W, crop, stream())
    return out


def nchw_to_nhwc(inp, out, mean=None, inv_std=None):
    B, C = inp.shape[0], inp.shape[1]
    P = inp.numel() // (B * C)
    _call("mmfn_nchw_to_nhwc_f32", ptr(inp), ptr(out), B, C, P, ptr(mean), ptr(inv_std), stream())
    return out


def lidar_splat(pts, out, flip_y=False):
    B, N, S = pts.shape
    _call("mmfn_lidar_splat_f32", ptr(pts), B, N, S, ptr(out), 1 if flip_y else 0, stream())
    return out


def lane_to_vector(lane, vec):
    n = lane.shape[-2]
    R = lane.numel() // (n * 5)
    _call("mmfn_lane_to_vector_f32", ptr(lane), ptr(vec), R, n, stream())
    return vec


def gather_field(src, dst, row_elems=None, dst_stride=None, dst_offset=0, row_off=None, count_out=None, lmax=0, palette=None):
    """One mmfn_gather_field.  src: u8 / f32 [n, ...] (dense) or the samples' rows concatenated [rows, ...] (ragged, with `row_off`
    the int64 device prefix sum [n + 1], `lmax` destination rows per sample and `count_out` int32 [B]); dst: f32.  row_elems defaults
    to the elements of one src row; dst_stride to one sample's destination (row_elems, or lmax * row_elems); both in elements.
    A u8 src with `palette` (f32 [16] on the device) is a coded field: two 4-bit codes per byte, low nibble first, each replaced
    by its palette entry; row_elems then counts destination floats (default: twice the bytes of one src row)."""
    f = _lib.GatherField()
    coded = palette is not None and src is not None and src.dtype == torch.uint8
    if row_elems is None:
        row_elems = src[0].numel() if src.shape[0] else int(torch.Size(src.shape[1:]).numel())
        if coded:
            row_elems *= 2
    if dst_stride is None:
        dst_stride = row_elems * (lmax if row_off is not None else 1)
    f.src, f.dst, f.row_off, f.count_out = ptr(src), ptr(dst), ptr(row_off), ptr(count_out)
    f.row_elems, f.dst_stride, f.dst_offset, f.lmax = int(row_elems), int(dst_stride), int(dst_offset), int(lmax)
    if coded:
        f.src_type, f.palette = _lib.GATHER_PAL4, ptr(palette)
    else:
        f.src_type = _lib.GATHER_U8 if src is not None and src.dtype == torch.uint8 else _lib.GATHER_F32
    return f


def gather_batch(fields, index, n):
    """Every field of one batch from a device-resident store in ONE launch (csrc/resident.hip): `fields` = gather_field(...) records
    (at most 16), `index` = int64 device tensor [B] of sample rows, n = rows in the store.  Capturable: the kernel reads `index`."""
    if index.dtype != torch.int64 or not index.is_contiguous():
        raise ValueError("gather_batch: index must be a contiguous int64 tensor")
    table = _lib.GatherTable()
    for k, f in enumerate(fields[:_lib.GATHER_MAX_FIELDS]):
        table.f[k] = f
    table.n_fields = len(fields)
    _call("mmfn_gather_batch", ctypes.byref(table), ptr(index), index.numel(), int(n), stream())


def gather_camera_jitter(srcs, dst, gray_mean, state, index, n, brightness=0.0, contrast=0.0, saturation=0.0, erase_thresh=0,
                         erase_h=(1, 1), erase_w=(1, 1), sample_id=None):
    """The camera frames of one batch gathered AND colour-jittered in one launch (csrc/resident.hip, mmfn_gather_camera_jitter).
    srcs: 1..4 tensors [n, 3, H, W] (or [n, 3 * H * W] with dst giving H, W), all u8 or all f32 with values 0..255: frame s of every
    sample; dst: f32 [B * S, 3, H, W], frame s of batch sample b at entry b * S + s; gray_mean: f32 [n, S] device; state: uint64
    (or int64) [2] device = {seed, epoch}; index: int64 device [B]; sample_id: int64 device [n] or None (= the row).  Strengths in
    [0, 1]; erase_thresh = round(prob * 2^24); erase_h / erase_w = (min, max) of the erased rectangle's sides in pixels.
    Capturable: index, state and sample_id are read by the kernel."""
    if index.dtype != torch.int64 or not index.is_contiguous():
        raise ValueError("gather_camera_jitter: index must be a contiguous int64 tensor")
    if not 1 <= len(srcs) <= _lib.JITTER_MAX_FRAMES:
        raise ValueError("gather_camera_jitter: 1..%d frames per sample, got %d" % (_lib.JITTER_MAX_FRAMES, len(srcs)))
    if dst.dim() != 4 or dst.shape[1] != 3 or dst.dtype != torch.float32 or not dst.is_contiguous():
        raise ValueError("gather_camera_jitter: dst must be a contiguous f32 [B * S, 3, H, W] tensor")
    d = _lib.CameraJitterDesc()
    for s, t in enumerate(srcs):
        if t is not None and (t.dtype != srcs[0].dtype or not t.is_contiguous() or (t.shape[0] and t[0].numel() != dst[0].numel())):
            raise ValueError("gather_camera_jitter: every source is a contiguous [n, 3, H, W] tensor of one dtype")
        d.src[s] = ptr(t)
    d.dst, d.gray_mean, d.sample_id, d.state = ptr(dst), ptr(gray_mean), ptr(sample_id), ptr(state)
    d.n_frames, d.H, d.W = len(srcs), dst.shape[2], dst.shape[3]
    d.src_type = _lib.GATHER_U8 if srcs[0] is not None and srcs[0].dtype == torch.uint8 else _lib.GATHER_F32
    d.brightness, d.contrast, d.saturation, d.erase_thresh = float(brightness), float(contrast), float(saturation), int(erase_thresh)
    (d.erase_h_min, d.erase_h_max), (d.erase_w_min, d.erase_w_max) = (int(v) for v in erase_h), (int(v) for v in erase_w)
    _call("mmfn_gather_camera_jitter", ctypes.byref(d), ptr(index), index.numel(), int(n), stream())
    return dst


def gather_camera_degrade(srcs, dst, gray_mean, state, degrade_state, index, n, brightness=0.0, contrast=0.0, saturation=0.0,
                          erase_thresh=0, erase_h=(1, 1), erase_w=(1, 1), hue=0.0, blur_thresh=0, blur_sigma=(0.5, 2.0), blur_radius=0,
                          noise_thresh=0, noise_std=(0.0, 0.0), sample_id=None):
    """gather_camera_jitter with a hue shift, a Gaussian blur and sensor noise between the blends and the erased rectangle, in one
    launch (csrc/resident.hip, mmfn_gather_camera_degrade; formulas in include/mmfn_hip.h).  Arguments as there, plus
    degrade_state: int64 [2] device = {seed, epoch} of the new draws; hue in [0, 0.5]; blur_thresh / noise_thresh = round(prob *
    2^24); blur_sigma = (lo, hi) with 0 < lo <= hi <= 8/3; blur_radius = R in 0..8, below min(H, W); noise_std = (lo, hi) in the
    image's 0..255 units.  Capturable: index, both states and sample_id are read by the kernel."""
    if index.dtype != torch.int64 or not index.is_contiguous():
        raise ValueError("gather_camera_degrade: index must be a contiguous int64 tensor")
    if not 1 <= len(srcs) <= _lib.JITTER_MAX_FRAMES:
        raise ValueError("gather_camera_degrade: 1..%d frames per sample, got %d" % (_lib.JITTER_MAX_FRAMES, len(srcs)))
    if dst.dim() != 4 or dst.shape[1] != 3 or dst.dtype != torch.float32 or not dst.is_contiguous():
        raise ValueError("gather_camera_degrade: dst must be a contiguous f32 [B * S, 3, H, W] tensor")
    d = _lib.CameraDegradeDesc()
    for s, t in enumerate(srcs):
        if t is not None and (t.dtype != srcs[0].dtype or not t.is_contiguous() or (t.shape[0] and t[0].numel() != dst[0].numel())):
            raise ValueError("gather_camera_degrade: every source is a contiguous [n, 3, H, W] tensor of one dtype")
        d.src[s] = ptr(t)
    d.dst, d.gray_mean, d.sample_id, d.state, d.degrade_state = ptr(dst), ptr(gray_mean), ptr(sample_id), ptr(state), ptr(degrade_state)
    d.n_frames, d.H, d.W = len(srcs), dst.shape[2], dst.shape[3]
    d.src_type = _lib.GATHER_U8 if srcs[0] is not None and srcs[0].dtype == torch.uint8 else _lib.GATHER_F32
    d.brightness, d.contrast, d.saturation, d.erase_thresh = float(brightness), float(contrast), float(saturation), int(erase_thresh)
    (d.erase_h_min, d.erase_h_max), (d.erase_w_min, d.erase_w_max) = (int(v) for v in erase_h), (int(v) for v in erase_w)
    d.hue, d.blur_thresh, d.blur_radius, d.noise_thresh = float(hue), int(blur_thresh), int(blur_radius), int(noise_thresh)
    (d.blur_sigma_lo, d.blur_sigma_hi), (d.noise_std_lo, d.noise_std_hi) = (float(v) for v in blur_sigma), (float(v) for v in noise_std)
    _call("mmfn_gather_camera_degrade", ctypes.byref(d), ptr(index), index.numel(), int(n), stream())
    return dst


def gather_augment(index, n, sample_id=None, lidar=None, lanes=None, target=None, map_state=None):
    """The bird's-eye-view fields of one batch gathered AND augmented in one launch (csrc/resident.hip, mmfn_gather_augment); each
    of the three parts is a dict or None:
      lidar  = dict(srcs = 1..4 tensors [n, C * H * W] u8 / f32 or [n, C * H * W / 2] u8 codes, palettes = None or one f32 [16] per
               frame (coded), dst = f32 [B * S, C, H, W], state = int64 [2] {seed, epoch}, cell_thresh, erase_thresh, erase_h, erase_w)
      lanes  = dict(src = f32 [rows, nodes, 5], row_off = int64 [n + 1], dst = f32 [B, lmax, nodes, 5], count_out = int32 [B] or
               None, lane_thresh, shift, yaw_rad)
      target = dict(src = f32 [n, 2], dst = f32 [B, 2], shift)
    map_state: int64 [2] {seed, epoch} of lanes and target; index: int64 device [B]; sample_id: int64 device [n] or None (= the
    row).  Thresholds are round(prob * 2^24).  Capturable: index, sample_id, the states and row_off are read by the kernel."""
    if index.dtype != torch.int64 or not index.is_contiguous():
        raise ValueError("gather_augment: index must be a contiguous int64 tensor")
    d = _lib.GatherAugmentDesc()
    d.sample_id, d.map_state = ptr(sample_id), ptr(map_state)
    if lidar is not None:
        srcs, dst, pals = lidar["srcs"], lidar["dst"], lidar.get("palettes")
        if not 1 <= len(srcs) <= _lib.AUGMENT_MAX_FRAMES:
            raise ValueError("gather_augment: 1..%d LiDAR frames per sample, got %d" % (_lib.AUGMENT_MAX_FRAMES, len(srcs)))
        if dst.dim() != 4 or dst.dtype != torch.float32 or not dst.is_contiguous():
            raise ValueError("gather_augment: the LiDAR dst must be a contiguous f32 [B * S, C, H, W] tensor")
        coded = pals is not None
        if coded and (len(pals) != len(srcs) or any(t is not None and t.dtype != torch.uint8 for t in srcs)):
            raise ValueError("gather_augment: a coded LiDAR field is u8 codes with one palette per frame")
        row = dst[0].numel() if dst.shape[0] else int(torch.Size(dst.shape[1:]).numel())
        for s, t in enumerate(srcs):
            if t is not None and (t.dtype != srcs[0].dtype or t.dtype not in (torch.uint8, torch.float32) or not t.is_contiguous()
                                  or (t.shape[0] and t[0].numel() * (2 if coded else 1) != row)):
                raise ValueError("gather_augment: every LiDAR source is a contiguous [n, C * H * W] u8 / f32 tensor (or [n, C * H * W / 2] "
                                 "codes) of one dtype")
            d.lidar_src[s] = ptr(t)
            if coded:
                d.lidar_palette[s] = ptr(pals[s])
        d.parts |= _lib.AUGMENT_LIDAR
        d.lidar_dst, d.lidar_state = ptr(dst), ptr(lidar["state"])
        d.n_frames, d.C, d.H, d.W = len(srcs), dst.shape[1], dst.shape[2], dst.shape[3]
        d.src_type = _lib.GATHER_PAL4 if coded else (_lib.GATHER_U8 if srcs[0] is not None and srcs[0].dtype == torch.uint8 else _lib.GATHER_F32)
        d.cell_thresh, d.erase_thresh = int(lidar.get("cell_thresh", 0)), int(lidar.get("erase_thresh", 0))
        (d.erase_h_min, d.erase_h_max), (d.erase_w_min, d.erase_w_max) = ((int(v) for v in lidar.get(k, (1, 1))) for k in ("erase_h", "erase_w"))
    if lanes is not None:
        src, dst = lanes["src"], lanes["dst"]
        if dst.dim() != 4 or dst.shape[3] != 5 or dst.dtype != torch.float32 or not dst.is_contiguous():
            raise ValueError("gather_augment: the lane dst must be a contiguous f32 [B, lmax, nodes, 5] tensor")
        if src is not None and (src.dtype != torch.float32 or not src.is_contiguous() or (src.shape[0] and src[0].numel() != dst.shape[2] * 5)):
            raise ValueError("gather_augment: the lane source is a contiguous f32 [rows, nodes * 5] tensor")
        if dst.shape[1] > _lib.AUGMENT_MAX_LANES:
            raise ValueError("gather_augment: a lane-augmented launch takes at most %d lanes per sample, got lmax = %d" % (
                _lib.AUGMENT_MAX_LANES, dst.shape[1]))
        d.parts |= _lib.AUGMENT_LANES
        d.lane_src, d.lane_row_off, d.lane_dst, d.lane_count_out = ptr(src), ptr(lanes["row_off"]), ptr(dst), ptr(lanes.get("count_out"))
        d.lane_nodes, d.lmax, d.lane_thresh = dst.shape[2], dst.shape[1], int(lanes.get("lane_thresh", 0))
        d.shift, d.yaw_rad = float(lanes.get("shift", 0.0)), float(lanes.get("yaw_rad", 0.0))
    if target is not None:
        d.parts |= _lib.AUGMENT_TARGET
        d.target_src, d.target_dst, d.target_shift = ptr(target["src"]), ptr(target["dst"]), float(target.get("shift", 0.0))
    _call("mmfn_gather_augment", ctypes.byref(d), ptr(index), index.numel(), int(n), stream())


def gather_radar_speed(index, n, sample_id=None, radar=None, speed=None):
    """The radar returns and the speed of one batch gathered AND augmented in one launch (csrc/resident.hip,
    mmfn_gather_radar_speed; draws and formulas in include/mmfn_hip.h); each of the two parts is a dict or None:
      radar = dict(src = f32 [n, 81, 5] (or [n, 405]), dst = f32 [B, 81, 5], adj = f32 [B, 81, 81], state = int64 [2] {seed, epoch},
              point_thresh, depth_std, angle_std, velocity_std): rows dropped and closed up, columns 0..3 perturbed, and the
              adjacency adj[i][j] = dst[j][1] - dst[i][1] rebuilt from the rows written
      speed = dict(src = f32 [n], dst = f32 [B], state = int64 [2] {seed, epoch}, drop_thresh, std)
    index: int64 device [B]; sample_id: int64 device [n] or None (= the row).  Thresholds are round(prob * 2^24).  Capturable: index,
    sample_id and the states are read by the kernel."""
    if index.dtype != torch.int64 or not index.is_contiguous():
        raise ValueError("gather_radar_speed: index must be a contiguous int64 tensor")
    d = _lib.RadarSpeedDesc()
    d.sample_id = ptr(sample_id)
    B = index.numel()
    if radar is not None:
        src, dst, adj = radar["src"], radar["dst"], radar["adj"]
        R = _lib.RADAR_ROWS
        if tuple(dst.shape) != (B, R, 5) or dst.dtype != torch.float32 or not dst.is_contiguous():
            raise ValueError("gather_radar_speed: the radar dst must be a contiguous f32 [B, %d, 5] tensor" % R)
        if tuple(adj.shape) != (B, R, R) or adj.dtype != torch.float32 or not adj.is_contiguous():
            raise ValueError("gather_radar_speed: the adjacency dst must be a contiguous f32 [B, %d, %d] tensor" % (R, R))
        if src is not None and (src.dtype != torch.float32 or not src.is_contiguous() or src.shape[0] < n
                                or int(torch.Size(src.shape[1:]).numel()) != R * 5):
            raise ValueError("gather_radar_speed: the radar source is a contiguous f32 [n, %d, 5] tensor" % R)
        d.parts |= _lib.SIGNAL_RADAR
        d.radar_src, d.radar_dst, d.adj_dst, d.radar_state, d.rows = ptr(src), ptr(dst), ptr(adj), ptr(radar["state"]), R
        d.point_thresh = int(radar.get("point_thresh", 0))
        d.depth_std, d.angle_std, d.velocity_std = (float(radar.get(k, 0.0)) for k in ("depth_std", "angle_std", "velocity_std"))
    if speed is not None:
        src, dst = speed["src"], speed["dst"]
        if dst.numel() != B or dst.dtype != torch.float32 or not dst.is_contiguous():
            raise ValueError("gather_radar_speed: the speed dst must be a contiguous f32 [B] tensor")
        if src is not None and (src.dtype != torch.float32 or not src.is_contiguous() or src.numel() < n):
            raise ValueError("gather_radar_speed: the speed source is a contiguous f32 [n] tensor")
        d.parts |= _lib.SIGNAL_SPEED
        d.speed_src, d.speed_dst, d.speed_state = ptr(src), ptr(dst), ptr(speed["state"])
        d.speed_drop_thresh, d.speed_std = int(speed.get("drop_thresh", 0)), float(speed.get("std", 0.0))
    _call("mmfn_gather_radar_speed", ctypes.byref(d), ptr(index), B, int(n), stream())


def polyline_pool_fwd(y, out, arg, R, V, H, last):
    _call("mmfn_polyline_pool_fwd_f32", ptr(y), ptr(out), ptr(arg), R, V, H, 1 if last else 0, stream())
    return out


def polyline_pool_bwd(gout, arg, gy, R, V, H, last):
    _call("mmfn_polyline_pool_bwd_f32", ptr(gout), ptr(arg), ptr(gy), R, V, H, 1 if last else 0, stream())
    return gy


def dropout_apply(inp, out, p, rng_state, rng_stream):
    _call("mmfn_dropout_apply_f32", ptr(inp), ptr(out), inp.numel(), float(p), ptr(rng_state), rng_stream, stream())
    return out


def relu_mask(g, y, out=None):
    out = g if out is None else out
    _call("mmfn_relu_mask_f32", ptr(g), ptr(y), ptr(out), g.numel(), stream())
    return out


# ---------------------------------------------------------------- radar GAT pieces
def elu_fwd(x, y):
    _call("mmfn_elu_fwd_f32", ptr(x), ptr(y), x.numel(), stream())
    return y


def elu_bwd(g, y, dx):
    _call("mmfn_elu_bwd_f32", ptr(g), ptr(y), ptr(dx), g.numel(), stream())
    return dx


def gat_softmax_fwd(e_pre, adj, alpha, p, att, drop_p=0.0, rng_state=None, rng_stream=0):
    R, N = e_pre.shape
    _call("mmfn_gat_softmax_fwd_f32", ptr(e_pre), ptr(adj), float(alpha), ptr(p), ptr(att), R, N, float(drop_p), ptr(rng_state),
          rng_stream, stream())


def gat_softmax_bwd(g_att, p, e_pre, adj, alpha, g_epre, drop_p=0.0, rng_state=None, rng_stream=0):
    R, N = e_pre.shape
    _call("mmfn_gat_softmax_bwd_f32", ptr(g_att), ptr(p), ptr(e_pre), ptr(adj), float(alpha), ptr(g_epre), R, N, float(drop_p),
          ptr(rng_state), rng_stream, stream())


def log_softmax_fwd(x, y, R, C, swap):
    _call("mmfn_log_softmax_fwd_f32", ptr(x), ptr(y), R, C, 1 if swap else 0, stream())
    return y


def log_softmax_bwd(g, y, dx, R, C, swap):
    _call("mmfn_log_softmax_bwd_f32", ptr(g), ptr(y), ptr(dx), R, C, 1 if swap else 0, stream())
    return dx


# ---------------------------------------------------------------- bf16 weight shadows
def make_ln_fold_table(entries, device):
    """entries: [(W [N,K], gamma [K], beta [K], bias [N] or None, Wf [N,K], c1 [N], c2 [N])] -> (device table, n, total rows) for
    ln_fold_weights."""
    import struct
    blob, row0 = b"", 0
    for W, gamma, beta, bias, Wf, c1, c2 in entries:
        N, K = W.shape
        assert W.is_contiguous() and Wf.is_contiguous() and Wf.shape == W.shape and gamma.numel() == K and c1.numel() == N
        blob += struct.pack("<QQQQQQQiiq", W.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0 if bias is None else bias.data_ptr(),
                            Wf.data_ptr(), c1.data_ptr(), c2.data_ptr(), N, K, row0)
        row0 += N
    t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    return t, len(entries), row0


def ln_fold_weights(table, n, total_rows):
    """The folded operands of every (LayerNorm -> Linear) pair of the step in one launch (once per forward: weights change at the
    optimizer step)."""
    _call("mmfn_ln_fold_weights_f32", ptr(table), n, total_rows, stream())


def cast_to_bf16(src, dst):
    _call("mmfn_cast_f32_to_bf16", ptr(src), ptr(dst), src.numel(), stream())
    return dst


def cast_to_f32(src, dst):
    _call("mmfn_cast_bf16_to_f32", ptr(src), ptr(dst), src.numel(), stream())
    return dst


def make_shadow_table(entries, device):
    """entries: [(src fp32 storage tensor [R, T, C] or [R, C], dst bf16 flat tensor)] -> (device table, n, total tiles) for
    shadow_transpose (dst[c][t][r] = src[r][t][c])."""
    import struct
    blob, tile0 = b"", 0
    for src, dst in entries:
        if src.dim() == 2:
            R, T, C = src.shape[0], 1, src.shape[1]
        else:
            R, T, C = src.shape[0], src.numel() // (src.shape[0] * src.shape[-1]), src.shape[-1]
        tiles_c = (C + 31) // 32
        blob += struct.pack("<QQiiiiq", src.data_ptr(), dst.data_ptr(), R, T, C, tiles_c, tile0)
        tile0 += T * ((R + 31) // 32) * tiles_c
    t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    return t, len(entries), tile0


def shadow_transpose(table, n, total):
    _call("mmfn_shadow_transpose_bf16", ptr(table), n, total, stream())


# ---------------------------------------------------------------- 7x7 stems: explicit im2col + plain GEMM (engine.ConvBN.stem_conv)
def im2col_small(x, col, kh, kw, stride, pad):
    B, H, W, Cin = x.shape
    _call("mmfn_im2col_small", ptr(x), ptr(col), 1 if col.dtype == BF16 else 0, B, H, W, Cin, kh, kw, stride, pad, col.shape[1], stream())
    return col


def repitch_rows(src, dst, R, K, ps, pd):
    _call("mmfn_repitch_rows", ptr(src), ptr(dst), 1 if dst.dtype == BF16 else 0, R, K, ps, pd, stream())
    return dst
