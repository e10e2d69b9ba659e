"""The bits of the optimizer-step launches, to compare two builds of libmmfn_hip.so (a refactor of mmfn_amd/csrc/optim.hip must
not change one of them).

    MMFN_HIP_LIB=/path/to/libmmfn_hip.so python tools/optim_bits.py dump OUT.pt      (GPU; one fresh process per library)
    python tools/optim_bits.py compare A.pt B.pt                                     (CPU; exit status 1 on any differing byte)

dump launches, through the six entry points (mmfn_adamw_groups_f32, mmfn_adamw_rows_f32, their _ams forms, mmfn_sgd_groups_f32,
mmfn_sgd_rows_f32), every valid variant (COEF / AVG / GUARD, and MASK for the groups forms) on fixed seeded inputs and records p,
the state streams and, where the variant has one, the average.  A (family, variant, case) cell:
  n           3076 (not a multiple of 1024, less than one grid trip) and 4194452 (past one grid trip); the tensors of the large
              size are recorded as SHA-256 digests of their bytes
  groups      AdamW: amsgrad set / clear / weight_decay 0.  SGD: momentum 0.9 nesterov / momentum 0.9 dampening 0.1 / momentum 0
  frozen      about a fifth of the float4s, wherever the variant can express it (MASK, rows)
  step        7; the SGD groups form also at 1 (its first step).  rows: two classes with counts 1 and 7
  average     EMA and SWA, n_averaged 0 and 5 (AVG variants)
  ok          1 and 0 (GUARD variants)
  coef        0.37 (COEF variants)
  stray byte  one group byte of 200 in the unmasked SGD groups form (it reads group 0)
"""
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

SIZES = (3076, 4194452)
FULL_BELOW = 1 << 16   # tensors of a larger n are recorded as digests
ADAMW_HYPER = [[1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5, 0.0, 1.0], [1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5, 0.0, 0.0],
               [2e-3, 0.8, 0.99, 1e-6, 0.0, 0.5, 0.0, 0.0]]
SGD_HYPER = [[1e-2, 0.9, 0.0, 1.0, 1e-2, 0.5, 0.0, 0.0], [1e-2, 0.9, 0.1, 0.0, 1e-2, 0.5, 0.0, 0.0], [1e-2, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0]]
ROWS = [[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1]]   # (group, class)


def inputs(n, dev):
    gen = torch.Generator().manual_seed(1234 + n)
    r = lambda scale: (torch.randn(n, generator=gen) * scale).to(dev)
    x = {"p": r(1.0), "g": r(0.01), "m": r(0.01), "v": r(0.01).square_(), "vmax": r(0.01).square_(), "avg": r(1.0)}
    n4 = n // 4
    group = torch.randint(0, 3, (n4,), generator=gen, dtype=torch.uint8)
    cls = torch.randint(0, 2, (n4,), generator=gen, dtype=torch.uint8)
    frozen = torch.rand(n4, generator=gen) < 0.2
    stray = group.clone()
    stray[5] = 200
    x["tables"] = {"plain": group.to(dev), "stray": stray.to(dev), "masked": group.masked_fill(frozen, 255).to(dev),
                   "rows": (group + 3 * cls).masked_fill(frozen, 255).to(dev)}
    return x


def digest(t, full):
    t = t.cpu()
    return t if full else hashlib.sha256(t.numpy().tobytes()).hexdigest()


def dump(out):
    from mmfn_amd import ops
    from mmfn_amd._lib import LIB_PATH
    dev = torch.device("cuda:0")
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    coef, class_steps = torch.tensor([0.37], device=dev), i64([1, 7])
    rows = torch.tensor(ROWS, dtype=torch.int32)
    ema_w = torch.tensor([1.0 - 0.999], dtype=torch.float64).to(torch.float32).to(dev)
    hyper = {"adamw": torch.zeros(16, 8, device=dev), "sgd": torch.zeros(16, 8, device=dev)}
    hyper["adamw"][:3] = torch.tensor(ADAMW_HYPER, device=dev)
    hyper["sgd"][:3] = torch.tensor(SGD_HYPER, device=dev)
    cells = {}
    for n in SIZES:
        x = inputs(n, dev)
        for family, with_coef, with_avg, guard in itertools.product(
                ("adamw_groups", "adamw_rows", "adamw_groups_ams", "adamw_rows_ams", "sgd_groups", "sgd_rows"), (0, 1), (0, 1), (0, 1)):
            if guard and not with_coef:
                continue   # not built
            sgd, by_rows, ams = family.startswith("sgd"), "rows" in family, family.endswith("ams")
            masks = (None,) if by_rows else (False, True)
            steps = (None,) if by_rows else ((1, 7) if sgd else (7,))
            avgs = tuple(itertools.product((ops.AVG_EMA, ops.AVG_SWA), (0, 5))) if with_avg else (None,)
            oks = (1, 0) if guard else (None,)
            for mask, step, av, ok in itertools.product(masks, steps, avgs, oks):
                t = {k: x[k].clone() for k in (("p", "m") if sgd else ("p", "m", "v", "vmax") if ams else ("p", "m", "v"))}
                kw = {"n": n, "coef": coef if with_coef else None, "ok": None if ok is None else torch.tensor([ok], dtype=torch.int32, device=dev)}
                if av is not None:
                    t["avg"] = x["avg"].clone()
                    kw["avg"] = (t["avg"], i64([av[1]]), ema_w, av[0])
                if ams:
                    kw["vmax"] = t["vmax"]
                state = (t["m"],) if sgd else (t["m"], t["v"])
                h = hyper["sgd" if sgd else "adamw"]
                if by_rows:
                    (ops.sgd_rows if sgd else ops.adamw_rows)(t["p"], x["g"], *state, class_steps, 2, h, 3, x["tables"]["rows"], rows, **kw)
                else:
                    table = x["tables"]["masked" if mask else "stray" if sgd else "plain"]
                    (ops.sgd_groups if sgd else ops.adamw_groups)(t["p"], x["g"], *state, i64([step]), h, 3, group_of=table, mask=mask, **kw)
                torch.cuda.synchronize()
                key = "%s/coef=%d,avg=%d,guard=%d,mask=%s/n=%d/step=%s,avg=%s,ok=%s" % (family, with_coef, with_avg, guard, mask, n, step, av, ok)
                cells[key] = {k: digest(v, n < FULL_BELOW) for k, v in t.items()}
    torch.save({"lib": LIB_PATH, "cells": cells}, out)
    print("optim_bits: %d cells from %s -> %s" % (len(cells), LIB_PATH, out), flush=True)


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return type(a) is type(b) and a == b
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def compare(path_a, path_b):
    a, b = (torch.load(p, map_location="cpu") for p in (path_a, path_b))
    ca, cb = a["cells"], b["cells"]
    bad = sorted(set(ca) ^ set(cb))
    tensors = 0
    for key in sorted(set(ca) & set(cb)):
        if set(ca[key]) != set(cb[key]):
            bad.append(key)
            continue
        for name in sorted(ca[key]):
            tensors += 1
            if not same(ca[key][name], cb[key][name]):
                bad.append("%s: %s" % (key, name))
    print("optim_bits: %s against %s: %d cells, %d tensors compared, %d differ" % (a["lib"], b["lib"], len(set(ca) & set(cb)), tensors, len(bad)))
    for line in bad:
        print("  differs: " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        raise SystemExit(__doc__)
