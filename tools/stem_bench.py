"""Isolated timing of the stems' BatchNorm + ReLU + maxpool, forward and backward, as the two op sequences the engine can run:
  old  forward : mmfn_bn_apply_f32 (relu) -> mmfn_maxpool3x3s2_fwd_f32                      (y written and read back)
       backward: mmfn_maxpool3x3s2_bwd_f32 -> mmfn_bn_bwd_f32 with y as the ReLU mask         (gy written, gy + y + co read twice)
  new  forward : mmfn_stem_bn_relu_maxpool_fwd_f32                                           (co -> pooled, idx)
       backward: mmfn_stem_bn_bwd_pooled_f32                                                 (pooled gradient, idx, co -> dco)
on the stem output of the benched shapes (128 x 128 x 64 per frame; the camera and the LiDAR stem have the same output shape, so
one row covers both).  HIP events over back-to-back iterations after warm-up; bytes are counted from the shapes (every operand
once per launch that touches it), not measured.
  python tools/stem_bench.py [--batches 32,128] [--reps 20]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mmfn_amd import ops  # noqa: E402

DEV = "cuda:0"


def timeit(fn, reps=20, rounds=3):
    for _ in range(3):
        fn()
    best = None
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) / reps * 1e3
        best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    H = W = 128
    C = 64
    for B in [int(b) for b in a.batches.split(",")]:
        M = B * H * W
        g = torch.Generator(device=DEV).manual_seed(B)
        co = torch.randn(B, H, W, C, device=DEV, generator=g) * 2
        mean, rstd = torch.randn(C, device=DEV, generator=g) * 0.3, torch.rand(C, device=DEV, generator=g) + 0.5
        gamma, beta = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g) * 0.2
        y, gy, dco = torch.empty_like(co), torch.empty_like(co), torch.empty_like(co)
        pooled = torch.empty(B, H // 2, W // 2, C, device=DEV)
        idx = torch.empty(pooled.shape, dtype=torch.uint8, device=DEV)
        gp = torch.randn(pooled.shape, device=DEV, generator=g)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        big, small = 4.0 * M * C, 4.0 * (M // 4) * C      # a stem-resolution fp32 tensor, a pooled one
        sidx = 1.0 * (M // 4) * C

        def old_fwd():
            ops.bn_apply(co.view(M, C), y.view(M, C), mean, rstd, gamma, beta, True)
            ops.maxpool_fwd(y, pooled, idx)

        def new_fwd():
            ops.stem_bn_relu_maxpool(co, mean, rstd, gamma, beta, pooled, idx)

        def old_bwd():
            ops.maxpool_bwd(gp, idx, gy)
            ops.bn_bwd(gy.view(M, C), y.view(M, C), co.view(M, C), mean, rstd, gamma, dco.view(M, C), dg, db)

        def new_bwd():
            ops.stem_bn_bwd_pooled(gp, idx, co, mean, rstd, gamma, beta, dco, dg, db)

        rows = [("fwd old  bn_apply + maxpool_fwd", old_fwd, 3 * big + small + sidx),
                ("fwd new  stem_bn_relu_maxpool", new_fwd, big + small + sidx),
                ("bwd old  maxpool_bwd + bn_bwd", old_bwd, (small + sidx + big) + 3 * big + 4 * big),
                ("bwd new  stem_bn_bwd_pooled", new_bwd, 2 * (big + small + sidx) + big)]
        old_fwd()   # y and idx for the backward rows
        print("B = %d: stem output %d x %d x %d x %d fp32 = %.0f MB" % (B, B, H, W, C, big / 1e6))
        t = {}
        for name, fn, nbytes in rows:
            us = timeit(fn, a.reps)
            t[name[:7]] = us
            print("  %-34s %8.1f us  %7.0f MB  %5.2f TB/s" % (name, us, nbytes / 1e6, nbytes / us / 1e6))
        print("  forward x%.2f, backward x%.2f, together %.1f -> %.1f us per stem" % (
            t["fwd old"] / t["fwd new"], t["bwd old"] / t["bwd new"], t["fwd old"] + t["bwd old"], t["fwd new"] + t["bwd new"]))


if __name__ == "__main__":
    main()
