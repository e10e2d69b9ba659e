"""End-to-end rate of the real training loop (phase-1 frames -> loader -> pinned staging -> H2D -> fused step): pickled PRE_Data
frames through DataLoader workers with eager launches / static-input hipGraph replay, the packed store (data.pack_frames +
PackedLoader) with graph replay, and the same store resident in HBM (data.ResidentFrames + ResidentLoader: one gather launch per
batch).  Complements bench.py, whose inputs are resident in HBM.

  trainer_bench.py [--dtype f32|bf16] [--modes eager,graph,packed,resident]     one child process per listed mode, in order
  trainer_bench.py --modes packed,resident,packed,resident --dtype bf16        a repeated mode gives the run-to-run spread
  trainer_bench.py gather                                                      child: ResidentLoader alone, for a kernel trace
  trainer_bench.py resident --compact / gather --compact                       the store with 4-bit palette codes (compact=True)
  trainer_bench.py resident --store DIR / gather --store DIR                   keep the frames and their packed form in DIR (made
                                                                               on first use) instead of a temporary directory"""
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmfn_amd import data as D  # noqa: E402
from mmfn_amd.config import GlobalConfig  # noqa: E402
from mmfn_amd.model import MMFN  # noqa: E402
from mmfn_amd.optim import FusedAdamW  # noqa: E402
from mmfn_amd.trainer import Trainer  # noqa: E402


def write_frames(root, n, seed=0):
    rng = np.random.RandomState(seed)
    for i in range(n):
        radar = rng.randn(81, 5)
        s = {"fronts": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8))],
             "lidars": [(rng.randint(0, 6, (2, 256, 256)) / 5.0).astype(np.float32)],
             "vectormaps": [torch.from_numpy(rng.randn(int(rng.randint(49, 65)), 10, 5))],
             "radar": [radar], "maps": [torch.from_numpy(rng.randint(0, 256, (3, 256, 256)).astype(np.uint8))],
             "waypoints": [tuple(rng.randn(2)) for _ in range(5)], "target_point": tuple(rng.randn(2) * 10.0),
             "steer": 0.0, "throttle": 0.5, "brake": False, "command": 1, "velocity": float(rng.uniform(0, 8))}
        with open(os.path.join(root, "%d.pkl" % i), "wb") as fd:
            pickle.dump(s, fd)


def gather_bytes(res, inp, gt):
    """(bytes read, bytes written) by the gather launch that produced (inp, gt), from the shapes: every source row once at its
    stored width (the lane sets at their true sizes, plus index and prefix-table entries), every output element once."""
    B = gt.shape[0]
    read = 8 * B
    for nm in res.plan_["arrays"]:
        t = res.tensors[nm]
        if nm + ".row_off" in res.tensors:
            read += int(inp["lane_num"].sum().item()) * t.shape[1] * t.element_size() + 16 * B
        else:
            read += B * t.shape[1] * t.element_size()
    read += sum(B * res.tensors[k][0].numel() * 4 for k in ("target_point", "velocity", "waypoints"))
    written = sum(t.numel() * t.element_size() for t in inp.values()) + gt.numel() * 4
    return read, written


def packed_store(root, n, cfg):
    """The packed form of write_frames(root, n), made on first use."""
    out = os.path.join(root, "packed")
    if not os.path.exists(os.path.join(out, "schema.json")):
        write_frames(root, n)
        D.pack_frames(D.PRE_Data(root, cfg, "train"), out)
    return D.PackedFrames(out)


def run_gather(B=32, n=768, epochs=3, dtype="f32", compact=False, store=None):
    """ResidentLoader alone (no training step): what a kernel trace of the gather launch should be taken on.  The wall time per
    launch (host clock over whole epochs that end in a synchronise, after a warm epoch) holds the host's work per batch too; the
    kernel's own time is the trace's."""
    cfg = GlobalConfig(act_dtype=dtype)
    with tempfile.TemporaryDirectory() as tmp:
        if store:
            os.makedirs(store, exist_ok=True)
        packed = packed_store(store or tmp, n, cfg)
        res = D.ResidentFrames(packed, "cuda:0", cfg, "vec", compact=compact)
        loader = D.ResidentLoader(res, batch_size=B, lane_bucket=16)
        read = written = launches = 0
        for inp, gt in loader:      # warm epoch: the byte counts (which read lane_num back) stay outside the timed window
            r, w = gather_bytes(res, inp, gt)
            read, written, launches = read + r, written + w, launches + 1
        torch.cuda.synchronize()
        t0 = time.time()
        timed = 0
        for _ in range(epochs):
            for inp, gt in loader:
                timed += 1
        torch.cuda.synchronize()
        dt = time.time() - t0
        return {"compact": bool(compact), "gather_launches": launches + timed, "wall_us_per_launch": round(dt / timed * 1e6, 1),
                "bytes_read_per_launch": read // launches, "bytes_written_per_launch": written // launches,
                "resident_store_bytes": res.nbytes()}


def run(mode, B=32, n=768, epochs=2, dtype="f32", compact=False, store=None):
    cfg = GlobalConfig(act_dtype=dtype)
    with tempfile.TemporaryDirectory() as tmp:
        if mode == "resident" and store:
            os.makedirs(store, exist_ok=True)
            packed_store(store, n, cfg)
            tmp = store
        else:
            write_frames(tmp, n)
        store = D.PRE_Data(tmp, cfg, "train")
        torch.manual_seed(0)
        net = MMFN(cfg, "cuda:0")
        opt = FusedAdamW(net, lr=1e-4)
        tr = Trainer("cuda:0", None)
        if mode == "packed":   # the flat memory-mapped store (data.pack_frames, one-time conversion) + its threaded loader
            t_pack = time.time()
            packed = D.PackedFrames(D.pack_frames(store, os.path.join(tmp, "packed")))
            t_pack = time.time() - t_pack
            loader = D.PackedLoader(packed, batch_size=B)
        elif mode == "resident":   # the packed store uploaded once; a batch is one gather launch on the training stream
            packed = packed_store(tmp, n, cfg)
            t_up = time.time()
            resident = D.ResidentFrames(packed, "cuda:0", cfg, "vec", compact=compact)
            torch.cuda.synchronize()
            t_up = time.time() - t_up
            loader = D.ResidentLoader(resident, batch_size=B, lane_bucket=16)
        else:
            loader = torch.utils.data.DataLoader(store, batch_size=B, shuffle=False, num_workers=8, collate_fn=D.collate,
                                                 persistent_workers=True, prefetch_factor=4)
        graph = mode != "eager"
        tr.train(net, loader, cfg, opt, graph=graph)  # warm epoch (buffers, capture, worker start-up)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(epochs):
            tr.train(net, loader, cfg, opt, graph=graph)
        torch.cuda.synchronize()
        dt = time.time() - t0
        res = {"dtype": dtype, "samples_per_s": round(epochs * n / dt, 1), "ms_per_step": round(dt / (epochs * n / B) * 1e3, 2),
               "host_threads": torch.get_num_threads()}
        # what the input side alone sustains (loader + pinned staging + H2D, no training step)
        t1 = time.time()
        for _ in D.DevicePrefetcher(loader, "cuda:0", cfg):
            pass
        torch.cuda.synchronize()
        res["input_side_only_samples_per_s"] = round(n / (time.time() - t1), 1)
        if mode == "packed":
            res["pack_seconds_per_1000_frames"] = round(t_pack / n * 1000, 2)
        if mode == "resident":
            res["upload_seconds_per_1000_frames"] = round(t_up / n * 1000, 2)
            res["resident_store_bytes"] = resident.nbytes()
            res["compact"] = bool(compact)
        return res


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", choices=["eager", "graph", "packed", "resident", "gather"],
                    help="child: run this one mode in this process (loader workers and 20 GB of engine buffers do not pile up)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="f32 = the parity path, bf16 = the bf16 training mode")
    ap.add_argument("--modes", default="eager,graph,packed,resident", help="parent: the modes to run, in this order; repeats allowed")
    ap.add_argument("--compact", action="store_true", help="resident / gather: keep few-valued float fields (the LiDAR histogram) "
                    "as 4-bit palette codes (ResidentFrames(compact=True))")
    ap.add_argument("--store", default=None, help="resident / gather: directory that keeps the frames and their packed form between runs")
    args = ap.parse_args()
    if args.mode:
        print(json.dumps(run_gather(dtype=args.dtype, compact=args.compact, store=args.store) if args.mode == "gather"
                         else run(args.mode, dtype=args.dtype, compact=args.compact, store=args.store)))
        return
    import subprocess
    out = []
    for mode in args.modes.split(","):
        extra = ["--compact"] if args.compact and mode == "resident" else []
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, "--dtype", args.dtype] + extra, capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stderr)
            raise SystemExit("mode %s failed with exit status %d" % (mode, r.returncode))
        out.append({"mode": mode, **json.loads(r.stdout.strip().splitlines()[-1])})
    print(json.dumps({"workload": "Trainer.train, batch 32, 768 phase-1 frames/epoch, one MI355X, dtype %s; eager / graph: pickles through "
                                  "8 persistent DataLoader workers; packed: data.PackedLoader over the memory-mapped conversion of the "
                                  "same frames, graph replay; resident: data.ResidentLoader over the same store in HBM, graph replay"
                                  % args.dtype, "runs": out}))


if __name__ == "__main__":
    main()
