"""Data side of the training path: the PRE_Data sample store, batch collation and host->device staging.

Mirrors, for the formats either side of the hot path:
  FrameStore        <- PRE_Data                    (mmfn_utils/datasets/dataloader.py:349-385)
  collate           <- collate_single_cpu          (mmfn_utils/datasets/data_utils.py:9-67)
  stage_batch       <- the H2D block of Engine.train (run_steps/phase2_train_net.py:63-103)
  radar_to_size / radar_adjacency / ego_transform / local_waypoints / local_target_point
                    <- dataloader.py:336-346, 381-384, 311-334, 240-261
The sample dict, the collated dict and the tensors handed to MMFN.forward keep the reference's keys,
nesting, dtypes and shapes.  What differs is where bytes are widened: uint8 camera / raster-map frames
cross PCIe as uint8 (the reference widens them to fp32 on the host first, 4x the traffic) and the
float64 lane / radar / label tensors are narrowed to fp32 on the host before the copy.

Host-side only (numpy / torch CPU tensors + async copies): no kernels live here, and nothing here is
part of the CPU oracle - with one exception: ResidentFrames / ResidentLoader keep the packed store in HBM and
assemble every batch with one launch of the gather kernel (csrc/resident.hip, through ops.gather_batch), and with
ResidentLoader(augment=CameraJitter(...)) a second one that gathers and colour-jitters the camera frames.
"""
import os
import pickle

import numpy as np
import torch

RADAR_ROWS = 81


# ------------------------------------------------------------------------------------------ per-sample geometry
def radar_to_size(points, rows=RADAR_ROWS, cols=5):
    """Force a radar return list to exactly `rows` rows (dataloader.py:336-346): short lists are zero
    padded; long ones lose the surplus rows with the largest |depth / velocity| (time to collision),
    in the order a descending argsort names them."""
    pts = np.asarray(points)
    n = pts.shape[0]
    if n < rows:
        out = np.zeros((rows, cols))
        out[:n, :] = pts[:n, :]
        return out
    ttc = np.abs(pts[:, 0] / pts[:, 3])
    surplus = np.argsort(-ttc)[:n - rows]
    return np.delete(pts, surplus, 0)


def radar_adjacency(radar):
    """adj[i, j] = radar[j, 1] - radar[i, 1] (dataloader.py:381-384); only its sign is used downstream."""
    col = np.asarray(radar)[:, 1]
    return col[None, :] - col[:, None]


def ego_transform(xyz, r1, t1_x, t1_y, r2, t2_x, t2_y):
    """Move 2-D points from frame 1 (rotation r1, translation t1) into frame 2 (dataloader.py:311-334).
    The z column rides along unchanged."""
    xyz = np.asarray(xyz, dtype=np.float64)
    h = np.stack([xyz[:, 0], xyz[:, 1], np.ones(len(xyz))], 0)

    def frame(r, tx, ty):
        c, s = np.cos(r), np.sin(r)
        return np.array([[c, s, tx], [-s, c, ty], [0.0, 0.0, 1.0]])

    world = frame(r1, t1_x, t1_y) @ h
    local = np.linalg.inv(frame(r2, t2_x, t2_y)) @ world
    out = local.T.copy()
    out[:, 2] = xyz[:, 2]
    return out


def local_waypoints(xs, ys, thetas, ego_index):
    """Ego-frame positions of the recorded poses (dataloader.py:240-248): pose i's origin seen from the
    pose at `ego_index`, using 90deg - theta as the reference does."""
    ex, ey, et = xs[ego_index], ys[ego_index], thetas[ego_index]
    out = []
    for x, y, t in zip(xs, ys, thetas):
        p = ego_transform(np.zeros((1, 3)), np.pi / 2 - t, -x, -y, np.pi / 2 - et, -ex, -ey)
        out.append((float(p[0, 0]), float(p[0, 1])))
    return out


def local_target_point(x_command, y_command, ego_x, ego_y, ego_theta):
    """Route command point in the ego frame (dataloader.py:250-261): R(90deg + theta)^T (p - ego)."""
    a = np.pi / 2 + ego_theta
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return tuple(rot.T.dot(np.array([x_command - ego_x, y_command - ego_y])))


# ------------------------------------------------------------------------------------------ host cores
def usable_cores():
    """Cores this process may actually use: affinity mask capped by the cgroup CPU quota (a GPU box may report 256 logical
    CPUs and grant a 16-CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def limit_host_threads():
    """torch's intra-op pool defaults to one thread per LOGICAL cpu.  Under a smaller cgroup quota every tiny host-side tensor
    op of the loader / staging code (a float64 -> float32 cast of the lane tensor, a stack of labels) then pays an OpenMP barrier
    across threads that are mostly descheduled - milliseconds each, ~100 ms per step measured on a 256-cpu box with a 16-cpu
    quota (tools/trainer_bench.py: 214 samples/s instead of > 900).  Lowers the pool to the usable cores; never raises it."""
    n = usable_cores()
    if torch.get_num_threads() > n:
        torch.set_num_threads(n)
    return torch.get_num_threads()


# ------------------------------------------------------------------------------------------ sample store
class FrameStore(torch.utils.data.Dataset):
    """Reader of the phase-1 output: one pickle per frame (written by run_steps/phase1_preprocess_data.py:42-48)
    plus the `rg_vec_mmfn_diag_pl_<seq>_<pred>_<use>.npy` file-list cache, created on first use exactly as
    PRE_Data does (dataloader.py:356-371) so both implementations can share a directory."""

    def __init__(self, root, config, data_use="train"):
        self.seq_len, self.pred_len = config.seq_len, config.pred_len
        index = os.path.join(root, "rg_vec_mmfn_diag_pl_%d_%d_%s.npy" % (self.seq_len, self.pred_len, data_use))
        if not os.path.exists(index):
            files = [str(root) + "/" + f for f in os.listdir(root) if f.split(".")[-1] == "pkl"]
            np.save(index, files)
        self.files = np.load(index)

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        with open(self.files[i], "rb") as fd:
            sample = pickle.load(fd)
        sample["radar_adj"] = radar_adjacency(sample["radar"][0])
        return sample


PRE_Data = FrameStore  # reference name


# ------------------------------------------------------------------------------------------ packed frames (row f1 at full rate)
# FrameStore unpickles ~0.9 MB per sample on the host; at the step rate of one MI355X (1000 samples/s) that, plus the
# worker -> main-process hand-over of every batch, is the bottleneck of the training loop.  pack_frames
# converts a directory of phase-1 pickles ONCE into flat per-field arrays; PackedFrames memory-maps them and PackedLoader gathers
# a batch's rows straight into pinned staging tensors in a background thread: one memcpy per field, no pickling, no worker
# processes.  The batches are bit-identical to collate([FrameStore[i] for i in indices]) (tests/test_data_cpu.py).
PACK_FORMAT = "mmfn-packed-frames-1"


def _leaf_kind(v):
    if isinstance(v, (torch.Tensor, np.ndarray)):
        return "array"
    if isinstance(v, (float, np.floating)):
        return "float"
    if isinstance(v, (bool, np.bool_)):
        return "bool"
    if isinstance(v, (int, np.integer)):
        return "int"
    if isinstance(v, (str, bytes)):
        return "str"
    if isinstance(v, (tuple, list)):
        return "list"
    raise TypeError("pack_frames: unsupported field type %s" % type(v))


def pack_frames(store, out_dir):
    """FrameStore (or any dataset of phase-1 sample dicts) -> out_dir/{schema.json, <field>.bin ...}.  One streaming pass.
    Every field must have the same structure in all samples (what `collate` requires too); lane sets may be ragged."""
    import json
    os.makedirs(out_dir, exist_ok=True)
    files, scalars, schema = {}, {}, None

    def emit(name, arr):
        arr = np.ascontiguousarray(arr.numpy() if isinstance(arr, torch.Tensor) else np.asarray(arr))
        ent = files.get(name)
        if ent is None:
            ent = files[name] = {"fd": open(os.path.join(out_dir, name + ".bin"), "wb"), "dtype": arr.dtype.str, "shape": list(arr.shape)}
        if arr.dtype.str != ent["dtype"] or list(arr.shape) != ent["shape"]:
            raise ValueError("pack_frames: field %s changes dtype / shape between samples (%s %s vs %s %s)"
                             % (name, arr.dtype.str, list(arr.shape), ent["dtype"], ent["shape"]))
        ent["fd"].write(arr.tobytes())

    def walk(v, name):
        kind = _leaf_kind(v)
        if kind == "array":
            emit(name, v)
            return {"kind": "array", "name": name}
        if kind == "list":
            return {"kind": "list", "items": [walk(x, "%s.%d" % (name, j)) for j, x in enumerate(v)]}
        scalars.setdefault(name, []).append(v.decode() if isinstance(v, bytes) else (v.item() if isinstance(v, np.generic) else v))
        return {"kind": kind, "name": name}

    def lanes(v, name):   # per frame of the sequence: ragged [L, n, F] -> concatenated rows + a count
        items = []
        for j, x in enumerate(v):
            x = np.ascontiguousarray(x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x))
            nm = "%s.%d" % (name, j)
            ent = files.get(nm)
            if ent is None:
                ent = files[nm] = {"fd": open(os.path.join(out_dir, nm + ".bin"), "wb"), "dtype": x.dtype.str, "shape": list(x.shape[1:]), "ragged": True}
            if x.dtype.str != ent["dtype"] or list(x.shape[1:]) != ent["shape"]:
                raise ValueError("pack_frames: lane field %s changes dtype / row shape between samples" % nm)
            ent["fd"].write(x.tobytes())
            scalars.setdefault(nm + ".count", []).append(int(x.shape[0]))
            items.append({"kind": "lanes", "name": nm})
        return {"kind": "list", "items": items}

    n = len(store)
    for i in range(n):
        sample = store[i]
        node = {k: (lanes(v, k) if k == "vectormaps" else walk(v, k)) for k, v in sample.items()}
        if schema is None:
            schema = node
        elif node != schema:
            raise ValueError("pack_frames: sample %d has a different structure than sample 0" % i)
    for ent in files.values():
        ent.pop("fd").close()
    with open(os.path.join(out_dir, "schema.json"), "w") as f:
        json.dump({"format": PACK_FORMAT, "n": n, "fields": schema, "files": files, "scalars": scalars}, f)
    return out_dir


class PackedFrames(object):
    """Memory-mapped view of a pack_frames directory.  batch(indices) == collate([store[i] for i in indices]), bit for bit
    (values, dtypes, shapes, container types), with the tensors optionally in pinned memory."""

    def __init__(self, root):
        import json
        with open(os.path.join(root, "schema.json")) as f:
            meta = json.load(f)
        if meta.get("format") != PACK_FORMAT:
            raise ValueError("%s is not a %s directory" % (root, PACK_FORMAT))
        self.n, self.fields, self.scalars = meta["n"], meta["fields"], meta["scalars"]
        self.arrays, self.offsets = {}, {}
        for name, ent in meta["files"].items():
            dt, shape = np.dtype(ent["dtype"]), tuple(ent["shape"])
            path = os.path.join(root, name + ".bin")
            if ent.get("ragged"):
                counts = np.asarray(self.scalars[name + ".count"], dtype=np.int64)
                self.offsets[name] = np.concatenate([[0], np.cumsum(counts)])
                rows = int(self.offsets[name][-1])
            else:
                rows = self.n
            self.arrays[name] = np.memmap(path, dtype=dt, mode="r", shape=(rows,) + shape) if rows else np.zeros((0,) + shape, dt)

    def __len__(self):
        return self.n

    def _gather(self, node, idx, pin):
        kind = node["kind"]
        if kind == "list":
            return [self._gather(c, idx, pin) for c in node["items"]]
        name = node["name"]
        if kind == "array":
            src = self.arrays[name]
            out = torch.empty((len(idx),) + src.shape[1:], dtype=_TORCH_DTYPE[src.dtype.str], pin_memory=pin)
            np.take(src, idx, axis=0, out=out.numpy(), mode="clip")   # (indices are in range; "clip" writes into `out` directly)
            return out
        if kind == "lanes":   # as _pad_lanes: [padded [B, Lmax, ...], counts i64 [B], int Lmax]
            src, off = self.arrays[name], self.offsets[name]
            nums = torch.tensor([int(off[i + 1] - off[i]) for i in idx])
            lmax = int(nums.max().item())
            out = torch.zeros((len(idx), lmax) + src.shape[1:], dtype=_TORCH_DTYPE[src.dtype.str], pin_memory=pin)
            o = out.numpy()
            for b, i in enumerate(idx):
                o[b, :off[i + 1] - off[i]] = src[off[i]:off[i + 1]]
            return [out, nums, lmax]
        vals = self.scalars[name]
        if kind == "float":
            return torch.tensor([float(vals[i]) for i in idx], dtype=torch.float64)
        if kind in ("int", "bool"):
            return torch.tensor([vals[i] for i in idx])
        if kind == "str":
            return [vals[i] for i in idx]
        raise ValueError(kind)

    def batch(self, indices, pin=False):
        idx = np.asarray(list(indices), dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise IndexError("sample index out of range")
        return {k: self._gather(node, idx, pin) for k, node in self.fields.items()}

    def __getitem__(self, i):
        """One sample as a batch of one (debugging aid; training goes through PackedLoader)."""
        return self.batch([i])


_TORCH_DTYPE = {np.dtype(k).str: v for k, v in (("uint8", torch.uint8), ("int8", torch.int8), ("int16", torch.int16), ("int32", torch.int32),
                                                  ("int64", torch.int64), ("float16", torch.float16), ("float32", torch.float32),
                                                  ("float64", torch.float64), ("bool", torch.bool))}


def _epoch_order(n, shuffle, sampler, seed, epoch):
    """Sample order of one epoch, shared by PackedLoader and ResidentLoader: the sampler's, else a seeded permutation, else 0..n-1."""
    if sampler is not None:
        return [int(i) for i in sampler]
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        return torch.randperm(n, generator=g).tolist()
    return list(range(n))


def _chunks(order, batch_size, drop_last):
    chunks = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    if drop_last and chunks and len(chunks[-1]) < batch_size:
        chunks.pop()
    return chunks


def _num_batches(n, batch_size, drop_last):
    return n // batch_size if drop_last else (n + batch_size - 1) // batch_size


class PackedLoader(object):
    """Iterates collated batches of a PackedFrames store; a background thread assembles them `prefetch` batches ahead into
    pinned memory (the caching host allocator keeps a block until the asynchronous copy that reads it has completed).
    Same role as make_loader(FrameStore, ...) for Trainer.train / DevicePrefetcher; `sampler` takes a DistributedSampler."""

    def __init__(self, packed, batch_size, shuffle=False, sampler=None, seed=0, drop_last=False, prefetch=3, pin_memory=True):
        self.packed, self.batch_size, self.shuffle, self.sampler = packed, int(batch_size), shuffle, sampler
        self.seed, self.drop_last, self.prefetch = seed, drop_last, max(1, int(prefetch))
        self.pin = bool(pin_memory) and torch.cuda.is_available()
        self.epoch = 0

    def _order(self):
        return _epoch_order(len(self.packed), self.shuffle, self.sampler, self.seed, self.epoch)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.packed)
        return _num_batches(n, self.batch_size, self.drop_last)

    def __iter__(self):
        import queue
        import threading
        order = self._order()
        self.epoch += 1
        chunks = _chunks(order, self.batch_size, self.drop_last)
        q, stop = queue.Queue(maxsize=self.prefetch), threading.Event()

        def work():
            try:
                for c in chunks:
                    if stop.is_set():
                        return
                    q.put(self.packed.batch(c, pin=self.pin))
                q.put(None)
            except BaseException as exc:   # hand the failure to the consumer instead of dying silently
                q.put(exc)

        t = threading.Thread(target=work, name="mmfn-packed-loader", daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            stop.set()
            while t.is_alive():    # unblock a producer waiting on a full queue
                try:
                    q.get_nowait()
                except queue.Empty:
                    t.join(timeout=0.05)


# ------------------------------------------------------------------------------------------ device-resident frames
# PackedLoader still moves every batch host -> device (one np.take per field into pinned memory, a copy, a u8 -> f32 widening):
# ~0.7-0.9 MB of host memcpy per sample on one Python thread per rank.  A 0.73 MB sample times 100 000 frames is 73 GB, and one
# MI355X has 288 GB: ResidentFrames uploads the fields the engine reads ONCE, and ResidentLoader then assembles a batch with a single
# gather launch by index (csrc/resident.hip) on the consumer's stream - no host thread, no pinned staging, no PCIe per batch.
# Bit-identical to MMFN._pack(*stage_batch(PackedFrames.batch(idx))[0]) (tests/test_resident_gpu.py).
RESIDENT_RESERVE_BYTES = 24 << 30   # kept free of the store by default: the engine's ~20 GB of buffers at batch 32, graph pools, slack
_BOUNCE_BYTES = 32 << 20            # pinned upload buffer


# ---- 4-bit palette coding of few-valued float fields (ResidentFrames(compact=True)): exact, bit patterns compared as uint32
def _f32_bits(rows):
    """[n, row] uint32 view of a float array after the f64 -> f32 rounding of the upload, or None for another dtype."""
    a = np.asarray(rows)
    if a.dtype not in (np.float32, np.float64):
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(a.shape[0], -1).view(np.uint32)


def _more_patterns(bits, known):
    """Appends the f32 bit patterns of `bits` that `known` (a list) lacks; False as soon as a 17th appears."""
    x = bits.ravel()
    for v in known:
        x = x[x != v]
    while x.size:
        if len(known) == 16:
            return False
        known.append(x[0])
        x = x[x != x[0]]
    return True


def _palette(known):
    """f32 [16]: the patterns in ascending uint32 order, unused slots +0.0."""
    pal = np.zeros(16, dtype=np.uint32)
    pal[:len(known)] = np.sort(np.asarray(known, dtype=np.uint32))
    return pal.view(np.float32)


def _encode_bits(bits, palette, count, out=None):
    """uint32 [n, row] -> u8 [n, row / 2]: element 2j in the low nibble of byte j, element 2j + 1 in the high nibble."""
    codes = np.searchsorted(palette.view(np.uint32)[:count], bits).astype(np.uint8)
    return np.bitwise_or(codes[:, 0::2], codes[:, 1::2] << 4, out=out)


def palette_encode(rows):
    """(codes u8 [n, row / 2], palette f32 [16], count) of a float field [n, ...] with at most 16 distinct f32 bit patterns (+0.0
    and -0.0, and two NaN payloads, are different entries) and an even row length; None for any other field.  f64 is rounded to
    f32 first."""
    bits = _f32_bits(rows)
    known = []
    if bits is None or bits.shape[1] % 2 or not _more_patterns(bits, known):
        return None
    palette = _palette(known)
    return _encode_bits(bits, palette, len(known)), palette, len(known)


def palette_decode(codes, palette):
    """f32 [n, 2 * bytes per row]: the inverse of palette_encode, bit for bit."""
    codes = np.asarray(codes, dtype=np.uint8)
    pal = np.asarray(palette, dtype=np.float32).view(np.uint32)
    out = np.empty((codes.shape[0], 2 * codes.shape[1]), dtype=np.uint32)
    out[:, 0::2] = pal[codes & 15]
    out[:, 1::2] = pal[codes >> 4]
    return out.view(np.float32)


# ---- camera colour jitter and random erasing inside the gather (ResidentLoader(augment=CameraJitter(...)))
# Every epoch of a resident store replays the same bytes; a host pipeline would put a transform into its Dataset.  The camera
# field's gather has each pixel in a register on its way from u8 to f32, so the photometric augmentation happens there
# (csrc/resident.hip, mmfn_gather_camera_jitter; formulas in include/mmfn_hip.h): no extra pass over HBM.  It is label-consistent
# for this model - LiDAR histogram, lanes, target point and waypoints are untouched, no geometry to keep in sync.
# The bird's-eye-view inputs are augmented the same way (Augment(lidar=LidarDropout(...), map=MapNoise(...)); one more launch,
# mmfn_gather_augment): cells and one rectangle of the LiDAR histogram dropped, lanes dropped, the lane set moved rigidly and the
# target point shifted, as localisation noise moves them in closed loop.  The camera's sensor degradation - a hue shift, a
# Gaussian blur and additive Gaussian noise (Augment(degrade=CameraDegrade(...))) - sits between the jitter's blends and its
# rectangle in a launch that takes the jitter launch's place (mmfn_gather_camera_degrade): the blur is a neighbourhood operation,
# so that kernel blends on load into LDS tiles and filters there.  The radar returns of a 'rad' store and the speed input of every
# variant (Augment(radar=RadarNoise(...), speed=SpeedNoise(...))) go through a fourth, small launch (mmfn_gather_radar_speed):
# returns dropped and closed up, depth, angles and velocity perturbed, the speed perturbed or zeroed - and the 81 x 81 adjacency,
# a function of the radar rows, rebuilt from the rows that launch wrote, since the stored one no longer describes them.  The
# rebuilt adjacency is the f32 difference of f32 values, the stored one the f32 rounding of a float64 difference: the two can
# differ in the last bit, so an inactive radar part keeps the plain launch and the stored bits.  Not built: augmentation of
# PackedLoader / the pickle loaders, rotating or shifting the LiDAR image or the raster map (both need resampling and would disagree
# with the un-shifted camera), ghost radar returns, reordered radar rows, waypoint noise, per-pixel dropout, a random stage order.
RNG_STREAM_JITTER = 0x4A49      # csrc/common.h: MMFN_RNG_STREAM_JITTER
RNG_STREAM_DEGRADE = 0x4447     # MMFN_RNG_STREAM_DEGRADE: a sample's degradation draws (hue, blur or not, sigma, noise or not, std)
RNG_STREAM_PIXEL_NOISE = 0x504E  # MMFN_RNG_STREAM_PIXEL_NOISE: two draws per camera element
DEGRADE_MAX_RADIUS = 8          # include/mmfn_hip.h: MMFN_DEGRADE_MAX_RADIUS
RNG_STREAM_LIDAR = 0x4C44       # MMFN_RNG_STREAM_LIDAR: a sample's LiDAR draws (erase or not, the rectangle)
RNG_STREAM_LIDAR_CELL = 0x4C43  # MMFN_RNG_STREAM_LIDAR_CELL: one draw per LiDAR element
RNG_STREAM_MAP = 0x4D50         # MMFN_RNG_STREAM_MAP: a sample's map draws (shift, yaw, target shift)
RNG_STREAM_LANE = 0x4C4E        # MMFN_RNG_STREAM_LANE: one draw per lane
AUGMENT_MAX_LANES = 4096        # include/mmfn_hip.h: MMFN_AUGMENT_MAX_LANES
RNG_STREAM_RADAR = 0x5244       # MMFN_RNG_STREAM_RADAR: one draw per stored radar row (kept or not)
RNG_STREAM_RADAR_NOISE = 0x524E  # MMFN_RNG_STREAM_RADAR_NOISE: two draws per radar row and column
RNG_STREAM_SPEED = 0x5350       # MMFN_RNG_STREAM_SPEED: a sample's speed draws (dropped or not, the two of its normal draw)
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _prob(owner, nm, v, hi=1.0):
    """float(v) in [0, hi], ValueError otherwise (a NaN fails it too)."""
    if not 0.0 <= float(v) <= hi:
        raise ValueError("%s: %s must lie in [0, %g], got %r" % (owner, nm, hi, v))
    return float(v)


def _thresh(p):
    """A 24-bit draw below this happens with probability p."""
    return int(round(p * (1 << 24)))


class _Erasing(object):
    """The one-rectangle-per-sample settings CameraJitter and LidarDropout share: erase_prob, erase_scale = (lo, hi) fractions of
    the frame's sides."""

    def _set_erase(self, erase_prob, erase_scale):
        owner = type(self).__name__
        try:
            lo, hi = (float(v) for v in erase_scale)
        except (TypeError, ValueError):
            raise ValueError("%s: erase_scale is a (lo, hi) pair of fractions, got %r" % (owner, erase_scale))
        if not 0.0 < lo <= hi <= 1.0:
            raise ValueError("%s: erase_scale needs 0 < lo <= hi <= 1, got %r" % (owner, erase_scale))
        self.erase_prob, self.erase_scale = _prob(owner, "erase_prob", erase_prob), (lo, hi)

    @property
    def erase_thresh(self):
        """The sample is erased iff its 24-bit draw 3 is below this."""
        return _thresh(self.erase_prob)

    def erase_bounds(self, side):
        """(min, max) of the erased rectangle's extent along a side of `side` pixels."""
        lo, hi = (min(int(side), max(1, int(round(f * side)))) for f in self.erase_scale)
        return lo, max(lo, hi)


class CameraJitter(_Erasing):
    """Settings of the resident loader's camera augmentation.  brightness / contrast / saturation: strengths in [0, 1], the factor
    of a sample is 1 + strength * (2 u - 1) with u uniform in [0, 1) (torchvision's ColorJitter(strength) range), applied in the
    order contrast, brightness, saturation; erase_prob: probability that one rectangle per sample becomes the frame's gray mean,
    its sides uniform in erase_scale = (lo, hi) as fractions of the frame's sides; seed: with the loader's epoch counter and the
    global sample id it decides every draw.  All frames of a sample's sequence get the same draws."""

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, erase_prob=0.0, erase_scale=(0.1, 0.3), seed=0):
        self.brightness, self.contrast, self.saturation = (_prob("CameraJitter", nm, v) for nm, v in (
            ("brightness", brightness), ("contrast", contrast), ("saturation", saturation)))
        self._set_erase(erase_prob, erase_scale)
        self.seed = int(seed)

    @property
    def active(self):
        return bool(self.brightness or self.contrast or self.saturation or self.erase_thresh)


class LidarDropout(_Erasing):
    """Settings of the resident loader's LiDAR augmentation.  cell_prob: probability that an element of the [C, H, W] histogram
    becomes 0 (each channel of a cell on its own); erase_prob: probability that one rectangle per sample loses every channel, its
    sides as in CameraJitter.  Kept elements keep their bits: occupancy features are not rescaled.  All frames of a sample's
    sequence get the same draws, decided by (seed, loader epoch, global sample id)."""

    def __init__(self, cell_prob=0.0, erase_prob=0.0, erase_scale=(0.1, 0.3), seed=0):
        self.cell_prob = _prob("LidarDropout", "cell_prob", cell_prob)
        self._set_erase(erase_prob, erase_scale)
        self.seed = int(seed)

    @property
    def cell_thresh(self):
        """An element is dropped iff its 24-bit draw is below this."""
        return _thresh(self.cell_prob)

    @property
    def active(self):
        return bool(self.cell_thresh or self.erase_thresh)


class MapNoise(object):
    """Settings of the resident loader's localisation noise on the vector map and the target point.  shift (metres, [0, 64]) and
    yaw_deg ([0, 45]): the lane set of a sample is rotated by yaw_deg * w and moved by shift * (w, w') with each w uniform in
    [-1, 1); lane_drop: probability that a lane other than lane 0 (the query of the lane attention) is left out, the others
    closing up; target_shift (metres, [0, 64]): the target point moves by target_shift * (w, w').  seed as in CameraJitter."""

    def __init__(self, shift=0.0, yaw_deg=0.0, lane_drop=0.0, target_shift=0.0, seed=0):
        self.shift, self.yaw_deg = _prob("MapNoise", "shift", shift, 64.0), _prob("MapNoise", "yaw_deg", yaw_deg, 45.0)
        self.lane_drop, self.target_shift = _prob("MapNoise", "lane_drop", lane_drop), _prob("MapNoise", "target_shift", target_shift, 64.0)
        self.seed = int(seed)

    @property
    def lane_thresh(self):
        """Lane j >= 1 is dropped iff its 24-bit draw is below this."""
        return _thresh(self.lane_drop)

    @property
    def yaw_rad(self):
        """The largest rotation as the f32 the kernel multiplies: rounded once, here."""
        return np.float32(self.yaw_deg * np.pi / 180.0)

    @property
    def lanes_active(self):
        return bool(self.shift or self.yaw_deg or self.lane_thresh)

    @property
    def active(self):
        return bool(self.lanes_active or self.target_shift)


def _range(owner, nm, v, lo_open, top):
    """(lo, hi) as floats with 0 <(=) lo <= hi <= top, ValueError otherwise (a NaN fails it too)."""
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError("%s: %s is a (lo, hi) pair, got %r" % (owner, nm, v))
    if not (lo <= hi <= top and (lo > 0.0 if lo_open else lo >= 0.0)):
        raise ValueError("%s: %s needs 0 %s lo <= hi <= %g, got %r" % (owner, nm, "<" if lo_open else "<=", top, v))
    return lo, hi


class CameraDegrade(object):
    """Settings of the resident loader's camera sensor degradation, applied between CameraJitter's blends and its erased
    rectangle.  hue in [0, 0.5]: the sample's hue turns by hue * (2 u - 1) of a full circle (torchvision's ColorJitter(hue)
    range); blur_prob: probability that a sample is blurred with a Gaussian whose sigma is uniform in blur_sigma = (lo, hi),
    0 < lo <= hi <= 8/3 - the filter radius is fixed per object, radius = ceil(3 hi) <= 8, as torchvision's GaussianBlur fixes
    its kernel size and varies sigma; noise_prob: probability that a sample gets additive Gaussian noise whose standard deviation
    is uniform in noise_std = (lo, hi), 0 <= lo <= hi <= 64, in the image's 0..255 units.  seed as in CameraJitter: all frames of
    a sample share its draws, the noise itself differs from frame to frame."""

    def __init__(self, hue=0.0, blur_prob=0.0, blur_sigma=(0.5, 2.0), noise_prob=0.0, noise_std=(2.0, 12.0), seed=0):
        self.hue = _prob("CameraDegrade", "hue", hue, 0.5)
        self.blur_prob, self.noise_prob = _prob("CameraDegrade", "blur_prob", blur_prob), _prob("CameraDegrade", "noise_prob", noise_prob)
        self.blur_sigma = _range("CameraDegrade", "blur_sigma", blur_sigma, True, 8.0 / 3.0)
        self.noise_std = _range("CameraDegrade", "noise_std", noise_std, False, 64.0)
        self.seed = int(seed)

    @property
    def radius(self):
        """R: the filter takes the 2 R + 1 pixels around each one, whatever sigma a sample draws."""
        return min(DEGRADE_MAX_RADIUS, int(np.ceil(3.0 * self.blur_sigma[1] - 1e-9)))

    @property
    def blur_thresh(self):
        """The sample is blurred iff its 24-bit draw 1 is below this."""
        return _thresh(self.blur_prob)

    @property
    def noise_thresh(self):
        """The sample gets noise iff its 24-bit draw 3 is below this."""
        return _thresh(self.noise_prob)

    @property
    def active(self):
        return bool(self.hue or self.blur_thresh or self.noise_thresh)


class RadarNoise(object):
    """Settings of the resident loader's radar augmentation ('rad' stores).  A radar sample is 81 rows [depth, altitude, azimuth,
    velocity, front/rear flag], the returns a frame recorded and zero rows after them (radar_to_size).  point_drop: probability
    that a return is left out, the others closing up in stored order with zero rows after them - a frame that recorded fewer;
    depth_std (metres, [0, 4]), angle_std (radians, [0, 0.1], altitude and azimuth alike) and velocity_std (m/s, [0, 4]): standard
    deviations of Gaussian noise on columns 0..3 of a kept return, the depth clamped at 0 from below.  Zero rows are never drawn for
    and never move, the flag is never touched, and the adjacency of the batch is rebuilt from the rows written.  seed as in
    CameraJitter."""

    def __init__(self, point_drop=0.0, depth_std=0.0, angle_std=0.0, velocity_std=0.0, seed=0):
        self.point_drop = _prob("RadarNoise", "point_drop", point_drop)
        self.depth_std, self.angle_std = _prob("RadarNoise", "depth_std", depth_std, 4.0), _prob("RadarNoise", "angle_std", angle_std, 0.1)
        self.velocity_std = _prob("RadarNoise", "velocity_std", velocity_std, 4.0)
        self.seed = int(seed)

    @property
    def point_thresh(self):
        """A return is dropped iff its 24-bit draw is below this."""
        return _thresh(self.point_drop)

    @property
    def column_std(self):
        """The standard deviations of columns 0..3 as the f32 values the kernel multiplies."""
        return tuple(float(np.float32(v)) for v in (self.depth_std, self.angle_std, self.angle_std, self.velocity_std))

    @property
    def active(self):
        return bool(self.point_thresh or self.depth_std or self.angle_std or self.velocity_std)


class SpeedNoise(object):
    """Settings of the resident loader's noise on the speed input (every variant).  std (m/s, [0, 4]): standard deviation of
    Gaussian noise on `velocity`, the result kept from crossing zero (max(v + std z, min(v, 0))); drop_prob: probability that a
    sample's speed is 0.0 instead - the usual remedy against a policy that copies its own speed into its waypoints.  seed as in
    CameraJitter."""

    def __init__(self, std=0.0, drop_prob=0.0, seed=0):
        self.std, self.drop_prob = _prob("SpeedNoise", "std", std, 4.0), _prob("SpeedNoise", "drop_prob", drop_prob)
        self.seed = int(seed)

    @property
    def drop_thresh(self):
        """The speed is dropped iff the sample's 24-bit draw 0 is below this."""
        return _thresh(self.drop_prob)

    @property
    def active(self):
        return bool(self.std or self.drop_thresh)


class Augment(object):
    """What ResidentLoader(augment=...) takes when more than the camera's colours is augmented: camera = CameraJitter or None,
    lidar = LidarDropout or None, map = MapNoise or None, degrade = CameraDegrade or None, radar = RadarNoise or None, speed =
    SpeedNoise or None.  A part that is None, or whose strengths are all zero, leaves its fields in the launch they would be in
    without it."""

    def __init__(self, camera=None, lidar=None, map=None, degrade=None, radar=None, speed=None):
        for nm, v, cls in (("camera", camera, CameraJitter), ("lidar", lidar, LidarDropout), ("map", map, MapNoise),
                           ("degrade", degrade, CameraDegrade), ("radar", radar, RadarNoise), ("speed", speed, SpeedNoise)):
            if v is not None and not isinstance(v, cls):
                raise TypeError("Augment: %s takes a %s (or None), got %r" % (nm, cls.__name__, v))
        self.camera, self.lidar, self.map, self.degrade, self.radar, self.speed = camera, lidar, map, degrade, radar, speed


def _hash32(x):
    """mmfn_hash32 (lowbias32) of a uint64 array holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(_M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(_M32)
    return x ^ (x >> np.uint64(16))


def rng_u32(seed, step, stream, idx):
    """mmfn_rng_u32(mmfn_rng_key({seed, step}, stream), idx) of csrc/common.h for an array of non-negative indices, restated with
    explicit 32 / 64-bit wrap-around: uint64 array of 32-bit draws."""
    key = ((int(seed) & _M64) * 0xD1342543DE82EF95 + (int(step) & _M64) * 0xA24BAED4963EE407) & _M64
    key ^= ((int(stream) << 40) & _M64) ^ (int(stream) * 0x9E3779B1)
    one = lambda v: np.asarray([v], dtype=np.uint64)
    salt = _hash32(one(key & _M32) ^ _hash32(one(key >> 32)))       # mmfn_rng_salt
    idx = np.asarray(idx).astype(np.uint64)
    lo, hi = idx & np.uint64(_M32), idx >> np.uint64(32)
    return _hash32(((lo ^ salt) + ((hi * np.uint64(0x9E3779B1)) & np.uint64(_M32))) & np.uint64(_M32))


def _sample_draws(seed, epoch, stream, sample_ids):
    """int64 [len(sample_ids), 8]: k_j = mmfn_rng_u32(key of `stream`, id * 8 + j) >> 8."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    idx = ids[:, None].astype(np.uint64) * np.uint64(8) + np.arange(8, dtype=np.uint64)[None, :]
    return (rng_u32(seed, epoch, stream, idx) >> np.uint64(8)).astype(np.int64)


def jitter_draws(seed, epoch, sample_ids):
    """int64 [len(sample_ids), 8]: the eight 24-bit draws k_0..k_7 the jitter kernel makes for global sample ids in epoch `epoch`
    (k_j = mmfn_rng_u32(key, id * 8 + j) >> 8): brightness, contrast, saturation, erase or not, rectangle height, width, x, y."""
    return _sample_draws(seed, epoch, RNG_STREAM_JITTER, sample_ids)


def lidar_draws(seed, epoch, sample_ids):
    """int64 [len(sample_ids), 8]: a sample's LiDAR draws (stream RNG_STREAM_LIDAR): k_0..k_2 reserved, then erase or not,
    rectangle height, width, x, y - the layout of jitter_draws, so erase_rectangle reads both."""
    return _sample_draws(seed, epoch, RNG_STREAM_LIDAR, sample_ids)


def map_draws(seed, epoch, sample_ids):
    """int64 [len(sample_ids), 8]: a sample's map draws (stream RNG_STREAM_MAP): shift x, shift y, yaw, target shift x, target
    shift y; k_5..k_7 unused.  w_j = 2 * k_j * 2^-24 - 1."""
    return _sample_draws(seed, epoch, RNG_STREAM_MAP, sample_ids)


def erase_rectangle(draws, jitter, H, W):
    """(y0, x0, h, w) of the rectangle a sample with draws k_0..k_7 loses in an [H, W] frame, or None when it keeps every pixel."""
    k = [int(v) for v in draws]
    if not k[3] < jitter.erase_thresh:
        return None
    (h_min, h_max), (w_min, w_max) = jitter.erase_bounds(H), jitter.erase_bounds(W)
    h = h_min + ((k[4] * (h_max - h_min + 1)) >> 24)
    w = w_min + ((k[5] * (w_max - w_min + 1)) >> 24)
    return (k[7] * (H - h + 1)) >> 24, (k[6] * (W - w + 1)) >> 24, h, w


def camera_jitter_reference(frames, gray_mean, draws, jitter):
    """What mmfn_gather_camera_jitter computes, in float64: frames [N, 3, H, W] with values 0..255, gray_mean [N] (the mean of
    0.299 R + 0.587 G + 0.114 B over each stored frame), draws int [N, 8] (jitter_draws of each frame's sample) -> float64
    [N, 3, H, W].  Contrast, brightness, saturation (each a blend clamped to [0, 255]), then the erased rectangle = gray_mean."""
    x = np.array(frames, dtype=np.float64)
    m = np.asarray(gray_mean, dtype=np.float64).reshape(-1)
    k = np.asarray(draws, dtype=np.int64).reshape(-1, 8)
    return _camera_erase(_camera_blends(x, m, k, jitter), m, k, jitter)


def _camera_blends(x, m, k, jitter):
    """The jitter's three blends on float64 frames [N, 3, H, W] (gray means m [N], draws k [N, 8])."""
    factor = lambda strength, j: (1.0 + float(np.float32(strength)) * (2.0 * (k[:, j] / 16777216.0) - 1.0))[:, None, None, None]
    f_b, f_c, f_s = factor(jitter.brightness, 0), factor(jitter.contrast, 1), factor(jitter.saturation, 2)
    x = np.clip(f_c * x + (1.0 - f_c) * m[:, None, None, None], 0.0, 255.0)
    x = np.clip(f_b * x, 0.0, 255.0)
    gray = 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
    return np.clip(f_s * x + (1.0 - f_s) * gray, 0.0, 255.0)


def _camera_erase(x, m, k, jitter):
    """The jitter's rectangle, in place: every channel of the erased pixels becomes the frame's gray mean."""
    H, W = x.shape[2:]
    for i in range(x.shape[0]):
        rect = erase_rectangle(k[i], jitter, H, W)
        if rect is not None:
            y0, x0, h, w = rect
            x[i, :, y0:y0 + h, x0:x0 + w] = m[i]
    return x


def degrade_draws(seed, epoch, sample_ids):
    """int64 [len(sample_ids), 8]: a sample's degradation draws (stream RNG_STREAM_DEGRADE): hue, blur or not, sigma, noise or
    not, noise std; k_5..k_7 reserved."""
    return _sample_draws(seed, epoch, RNG_STREAM_DEGRADE, sample_ids)


def hue_shift_reference(x, shift):
    """Stage 2 of mmfn_gather_camera_degrade in float64: x [..., 3, H, W] (any scale: the formulas divide only by the pixel's own
    max and chroma), shift in turns, broadcast against x's leading axes + [1, 1].  torchvision's _rgb2hsv, h <- frac(h + shift),
    _hsv2rgb."""
    x = np.asarray(x, dtype=np.float64)
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    c = mx - mn
    gray = mx == mn
    s = c / np.where(gray, 1.0, mx)
    inv = 1.0 / np.where(gray, 1.0, c)
    rc, gc, bc = (mx - r) * inv, (mx - g) * inv, (mx - b) * inv
    h6 = np.where(mx == r, bc - gc, np.where(mx == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = h6 / 6.0 + shift
    h = h - np.floor(h)
    hs = h * 6.0
    fl = np.floor(hs)
    f = hs - fl
    sector = fl.astype(np.int64) % 6
    top = np.max(np.abs(x)) if x.size else 0.0
    clamp = lambda v: np.clip(v, 0.0, max(top, 0.0))
    p, q, t = clamp(mx * (1.0 - s)), clamp(mx * (1.0 - s * f)), clamp(mx * (1.0 - s * (1.0 - f)))
    out = np.empty_like(x)
    out[..., 0, :, :] = np.choose(sector, [mx, q, p, p, t, mx])
    out[..., 1, :, :] = np.choose(sector, [t, mx, mx, q, p, p])
    out[..., 2, :, :] = np.choose(sector, [p, p, t, mx, mx, q])
    return out


def gaussian_blur_reference(x, sigma, radius):
    """Stage 3 in float64: x [..., H, W] filtered along W, then along H, with the 2 radius + 1 taps exp(-d^2 / (2 sigma^2)) over
    their sum; outside the frame the pixel mirrored at the border without repeating it (numpy's and torch's "reflect")."""
    x = np.asarray(x, dtype=np.float64)
    R = int(radius)
    d = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-d * d / (2.0 * float(sigma) ** 2))
    w /= w.sum()
    lead = [(0, 0)] * (x.ndim - 2)
    H, W = x.shape[-2:]
    xp = np.pad(x, lead + [(0, 0), (R, R)], mode="reflect")
    x = sum(w[k] * xp[..., :, k:k + W] for k in range(2 * R + 1))
    xp = np.pad(x, lead + [(R, R), (0, 0)], mode="reflect")
    return sum(w[k] * xp[..., k:k + H, :] for k in range(2 * R + 1))


def pixel_noise_reference(seed, epoch, sample_id, n_frames, frame, shape):
    """The standard normal draws of stage 4 for frame `frame` of sample `sample_id`, float64 [3, H, W]: element e draws at
    2 q and 2 q + 1 of stream RNG_STREAM_PIXEL_NOISE, q = (id * n_frames + frame) * 3 H W + e in wrapping 64-bit arithmetic;
    sqrt(-2 ln u1) cos(2 pi u2) with u1 = (k + 1) 2^-24, u2 = k' 2^-24."""
    numel = int(np.prod(shape))
    base = (((int(sample_id) & _M64) * int(n_frames) + int(frame)) * numel) & _M64
    q = np.arange(numel, dtype=np.uint64) + np.asarray([base], dtype=np.uint64)          # (arrays wrap silently)
    two = np.uint64(2)
    k0 = (rng_u32(seed, epoch, RNG_STREAM_PIXEL_NOISE, q * two) >> np.uint64(8)).astype(np.float64)
    k1 = (rng_u32(seed, epoch, RNG_STREAM_PIXEL_NOISE, q * two + np.uint64(1)) >> np.uint64(8)).astype(np.float64)
    z = np.sqrt(-2.0 * np.log((k0 + 1.0) / 16777216.0)) * np.cos(2.0 * np.pi * (k1 / 16777216.0))
    return z.reshape(shape)


def camera_degrade_reference(frames, gray_mean, ids, epoch, jitter, degrade):
    """What mmfn_gather_camera_degrade computes, in float64: frames [N, 3, H, W] (one frame per sample) or [N, S, 3, H, W] with
    values 0..255, gray_mean [N] or [N, S] as in camera_jitter_reference, ids [N] the samples' global ids, jitter = CameraJitter
    or None, degrade = CameraDegrade or None -> float64 of frames' shape.  The jitter's blends, hue, blur, noise, the jitter's
    rectangle; a degrade that does nothing gives camera_jitter_reference's result."""
    jitter = jitter if jitter is not None else CameraJitter()
    degrade = degrade if degrade is not None else CameraDegrade()
    x = np.array(frames, dtype=np.float64)
    shape = x.shape
    S = 1 if x.ndim == 4 else shape[1]
    x = x.reshape((-1,) + shape[-3:])
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    m = np.asarray(gray_mean, dtype=np.float64).reshape(-1)
    k = np.repeat(jitter_draws(jitter.seed, epoch, ids), S, axis=0)
    q = np.repeat(degrade_draws(degrade.seed, epoch, ids), S, axis=0)
    u = q / 16777216.0
    f32 = lambda v: float(np.float32(v))
    x = _camera_blends(x, m, k, jitter)
    if degrade.hue != 0.0:
        x = np.clip(hue_shift_reference(x, (f32(degrade.hue) * (2.0 * u[:, 0] - 1.0))[:, None, None]), 0.0, 255.0)
    lo, hi = (f32(v) for v in degrade.blur_sigma)
    n_lo, n_hi = (f32(v) for v in degrade.noise_std)
    for f in range(x.shape[0]):
        if q[f, 1] < degrade.blur_thresh:
            x[f] = gaussian_blur_reference(x[f], lo + (hi - lo) * u[f, 2], degrade.radius)
        if q[f, 3] < degrade.noise_thresh:
            z = pixel_noise_reference(degrade.seed, epoch, ids[f // S], S, f % S, x[f].shape)
            x[f] = np.clip(x[f] + (n_lo + (n_hi - n_lo) * u[f, 4]) * z, 0.0, 255.0)
    return _camera_erase(x, m, k, jitter).reshape(shape)


def lidar_dropout_reference(frames, ids, aug, epoch):
    """What mmfn_gather_augment writes for LiDAR frames [N, C, H, W] (f32 bits kept) whose samples have the global ids `ids` [N]
    under aug = LidarDropout in epoch `epoch`: f32 [N, C, H, W], dropped elements and the erased rectangle +0.0."""
    x = np.array(frames, dtype=np.float32)
    N, C, H, W = x.shape
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    bits = x.view(np.uint32).reshape(N, -1)
    if aug.cell_thresh:
        idx = ids.astype(np.uint64)[:, None] * np.uint64(C * H * W) + np.arange(C * H * W, dtype=np.uint64)[None, :]   # wraps mod 2^64
        bits[(rng_u32(aug.seed, epoch, RNG_STREAM_LIDAR_CELL, idx) >> np.uint64(8)) < np.uint64(aug.cell_thresh)] = 0
    k = lidar_draws(aug.seed, epoch, ids)
    for i in range(N):
        rect = erase_rectangle(k[i], aug, H, W)
        if rect is not None:
            y0, x0, h, w = rect
            x[i, :, y0:y0 + h, x0:x0 + w] = 0.0
    return x


def lane_keep_mask(ids, counts, aug, epoch):
    """bool [N, max(counts)]: True where lane j < counts[b] of the sample with global id ids[b] stays under aug = MapNoise in
    epoch `epoch` (lane 0 always; lane j >= 1 iff its draw mmfn_rng_u32(key_LANE, id * 65536 + j) >> 8 is not below lane_thresh);
    False from counts[b] on."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    L = int(counts.max()) if counts.size else 0
    j = np.arange(L, dtype=np.uint64)[None, :]
    draw = rng_u32(aug.seed, epoch, RNG_STREAM_LANE, ids.astype(np.uint64)[:, None] * np.uint64(65536) + j) >> np.uint64(8)
    keep = (draw >= np.uint64(aug.lane_thresh)) | (j == 0)
    return keep & (np.arange(L)[None, :] < counts[:, None])


def map_noise_reference(lanes, counts, target_point, ids, aug, epoch):
    """What mmfn_gather_augment writes for the padded lane sets lanes [N, lmax, nodes, 5] with `counts` [N] stored lanes each (the
    plain loader's lane / lane_num) and target points [N, 2], under aug = MapNoise: (lanes float64 [N, lmax, nodes, 5], counts
    int64 [N], target points float64 [N, 2]).  The first min(count, lmax) lanes take part; kept lanes close up in stored order, the
    rows after them are +0.0, counts lose the dropped lanes.  Nodes that are not all zero turn by yaw_rad * w_2 and move by
    shift * (w_0, w_1), in float64; with shift = yaw_deg = 0 (target_shift = 0) values are copied, so their f32 bits survive."""
    src = np.asarray(lanes)
    N, lmax = src.shape[:2]
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    w = 2.0 * (map_draws(aug.seed, epoch, ids).astype(np.float64) / 16777216.0) - 1.0
    shift, yaw, tshift = float(np.float32(aug.shift)), float(aug.yaw_rad), float(np.float32(aug.target_shift))
    keep = lane_keep_mask(ids, np.minimum(counts, lmax), aug, epoch)
    out = np.zeros(src.shape, dtype=np.float64)
    out_counts = counts.copy()
    for b in range(N):
        rows = np.flatnonzero(keep[b])
        out_counts[b] -= min(int(counts[b]), lmax) - len(rows)
        x = src[b, rows].astype(np.float64)                               # [kept, nodes, 5]
        if shift or yaw:
            c, s_ = np.cos(yaw * w[b, 2]), np.sin(yaw * w[b, 2])
            real = (x != 0.0).any(axis=-1)                                # an all-zero node is padding
            xr = c * x[..., 0] - s_ * x[..., 1] + shift * w[b, 0]
            yr = s_ * x[..., 0] + c * x[..., 1] + shift * w[b, 1]
            x[..., 0], x[..., 1] = np.where(real, xr, x[..., 0]), np.where(real, yr, x[..., 1])
        out[b, :len(rows)] = x
    tp = np.array(target_point, dtype=np.float64).reshape(N, 2)
    if tshift:
        tp = tp + tshift * w[:, 3:5]
    return out, out_counts, tp


def _normal(k0, k1):
    """The camera's sensor noise draw out of two arrays of 24-bit draws, float64: sqrt(-2 ln u1) cos(2 pi u2), u1 = (k0 + 1) 2^-24,
    u2 = k1 2^-24."""
    k0, k1 = np.asarray(k0, dtype=np.float64), np.asarray(k1, dtype=np.float64)
    return np.sqrt(-2.0 * np.log((k0 + 1.0) / 16777216.0)) * np.cos(2.0 * np.pi * (k1 / 16777216.0))


def _radar_row_index(sample_ids):
    """uint64 [N, 81]: id * 128 + r for stored row r of each sample (wraps mod 2^64)."""
    ids = np.asarray(sample_ids, dtype=np.int64).reshape(-1)
    return ids.astype(np.uint64)[:, None] * np.uint64(128) + np.arange(RADAR_ROWS, dtype=np.uint64)[None, :]


def radar_draws(seed, epoch, sample_ids):
    """int64 [len(sample_ids), 81]: the 24-bit draw of every stored radar row (stream RNG_STREAM_RADAR):
    k_r = mmfn_rng_u32(key, id * 128 + r) >> 8; a row that is not padding is dropped iff k_r < point_thresh."""
    return (rng_u32(seed, epoch, RNG_STREAM_RADAR, _radar_row_index(sample_ids)) >> np.uint64(8)).astype(np.int64)


def radar_normals(seed, epoch, sample_ids):
    """float64 [len(sample_ids), 81, 4]: the standard normal draw of column c of stored row r (stream RNG_STREAM_RADAR_NOISE):
    draws 2 q and 2 q + 1 with q = (id * 128 + r) * 4 + c in wrapping 64-bit arithmetic - whatever happens to the other rows."""
    q = _radar_row_index(sample_ids)[:, :, None] * np.uint64(4) + np.arange(4, dtype=np.uint64)[None, None, :]
    two = np.uint64(2)
    draw = lambda idx: rng_u32(seed, epoch, RNG_STREAM_RADAR_NOISE, idx) >> np.uint64(8)
    return _normal(draw(q * two), draw(q * two + np.uint64(1)))


def speed_draws(seed, epoch, sample_ids):
    """int64 [len(sample_ids), 8]: a sample's speed draws (stream RNG_STREAM_SPEED): dropped or not, then the two draws of its
    normal; k_3..k_7 unused."""
    return _sample_draws(seed, epoch, RNG_STREAM_SPEED, sample_ids)


def radar_keep_mask(radar, ids, aug, epoch):
    """bool [N, 81]: True where stored row r of radar [N, 81, 5], the sample with global id ids[b], stays under aug = RadarNoise in
    epoch `epoch`: it is not padding (its five values are not all zero) and its draw is not below point_thresh."""
    real = (np.asarray(radar).reshape(-1, RADAR_ROWS, 5) != 0.0).any(axis=-1)
    return real & (radar_draws(aug.seed, epoch, ids) >= aug.point_thresh)


def radar_noise_reference(radar, ids, aug, epoch):
    """What mmfn_gather_radar_speed writes for the stored radar rows radar [N, 81, 5] (f32 values) of the samples with global ids
    `ids` [N] under aug = RadarNoise: (radar float64 [N, 81, 5], adjacency float64 [N, 81, 81]).  Kept rows close up in stored
    order, the rows after them are +0.0; columns 0..3 of a kept row get std_c * z in float64 (std = depth, angle, angle, velocity),
    the depth then clamped at 0 from below; a column whose std is 0 is copied, so its f32 bits survive, and so is the flag.
    adjacency[b, i, j] = out[b, j, 1] - out[b, i, 1] over all rows (radar_adjacency of the rows written)."""
    src = np.asarray(radar).reshape(-1, RADAR_ROWS, 5)
    keep = radar_keep_mask(src, ids, aug, epoch)
    x = src.astype(np.float64)
    z = radar_normals(aug.seed, epoch, ids)
    for c, std in enumerate(aug.column_std):
        if std:
            x[..., c] += std * z[..., c]
            if c == 0:
                x[..., 0] = np.maximum(x[..., 0], 0.0)
    out = np.zeros(x.shape, dtype=np.float64)
    for b in range(x.shape[0]):
        rows = np.flatnonzero(keep[b])
        out[b, :len(rows)] = x[b, rows]
    return out, out[:, None, :, 1] - out[:, :, None, 1]


def speed_noise_reference(velocity, ids, aug, epoch):
    """What mmfn_gather_radar_speed writes for the stored speeds velocity [N] (f32 values) under aug = SpeedNoise: float64 [N].
    +0.0 where the sample's draw 0 is below drop_thresh; otherwise max(v + std z, min(v, 0)) with z from draws 1 and 2, or the
    stored value itself with std = 0."""
    v = np.array(velocity, dtype=np.float64).reshape(-1)
    k = speed_draws(aug.seed, epoch, ids)
    std = float(np.float32(aug.std))
    out = np.maximum(v + std * _normal(k[:, 1], k[:, 2]), np.minimum(v, 0.0)) if std else v.copy()
    out[k[:, 0] < aug.drop_thresh] = 0.0
    return out


class ResidentFrames(object):
    """A PackedFrames store (or the static shard `indices` of it) in device memory, reduced to what the `variant`'s engine input
    reads: camera and LiDAR frames, target point, velocity, waypoints; lane sets (vec, rad) or raster maps (img); radar and
    radar_adj (rad).  u8 stays u8 and f32 stays f32; float64 arrays and the JSON scalars are rounded to f32 on the host, the same
    conversion stage_batch applies before its copy.  Resident row r holds sample indices[r].
    compact=True keeps every dense float field whose kept rows take at most 16 distinct f32 values (the LiDAR histogram: counts
    clipped at 5, over 5) as 4-bit codes plus a 16-entry palette, an eighth of its f32 bytes; the gather kernel decodes it, so the
    batches are the same bits.  A field that does not qualify stays f32."""

    def __init__(self, packed, device, config, variant, indices=None, max_bytes=None, compact=False):
        plan, palettes = self._plan(packed, config, variant, indices, compact)
        self.device = torch.device(device)
        if max_bytes is None:
            if self.device.type != "cuda":
                raise ValueError("ResidentFrames keeps the store in GPU memory (got device %s)" % self.device)
            max_bytes = torch.cuda.mem_get_info(self.device)[0] - RESIDENT_RESERVE_BYTES
        if plan["bytes"] > max_bytes:
            raise ValueError("ResidentFrames: the store needs %d bytes of device memory, %d are available (free memory less a "
                             "%d-byte reserve for the engine's buffers unless max_bytes says otherwise); shard it with `indices` "
                             "%sor stay with PackedLoader" % (plan["bytes"], max_bytes, RESIDENT_RESERVE_BYTES,
                                                               "" if compact else ", pass compact=True "))
        self.config, self.variant, self.plan_ = config, variant, plan
        self.seq_len, self.pred_len = config.seq_len, config.pred_len
        rows = plan["rows"]
        self.n = len(rows)
        self.indices = rows
        self._row_of = np.full(len(packed), -1, dtype=np.int64)
        self._row_of[rows] = np.arange(self.n, dtype=np.int64)     # (a repeated sample keeps its last row)
        self.shapes = {nm: tuple(packed.arrays[nm].shape[1:]) for nm in plan["arrays"]}
        self.tensors = {}
        bounce = torch.empty(_BOUNCE_BYTES, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        for nm in plan["arrays"]:
            src = packed.arrays[nm]
            if nm in packed.offsets:   # ragged: the kept samples' rows, concatenated in resident order
                off = packed.offsets[nm]
                counts = (off[1:] - off[:-1])[rows]
                self.lane_counts = counts.astype(np.int64)
                new_off = np.concatenate([[0], np.cumsum(self.lane_counts)]).astype(np.int64)
                take = np.concatenate([np.arange(off[i], off[i + 1]) for i in rows]) if self.n else np.zeros(0, np.int64)
                self.tensors[nm] = self._upload(src, take, bounce)
                self.tensors[nm + ".row_off"] = torch.from_numpy(new_off).to(self.device)
            else:
                self.tensors[nm] = self._upload(src, rows, bounce, palettes.get(nm))
                if nm in palettes:
                    self.tensors[nm + ".palette"] = torch.from_numpy(palettes[nm][0]).to(self.device)
        f32 = lambda t: t.to(torch.float32).to(self.device)
        for nm, t in self._labels(packed, config, rows).items():
            self.tensors[nm] = f32(t)
        del bounce

    # ---- what goes to the device, and how many bytes: no device needed
    @classmethod
    def plan(cls, packed, config, variant, indices=None, compact=False):
        """{"fields": {name: bytes}, "bytes": total, "arrays": [packed array names], "rows": int64 sample ids, "compact": [names of
        the fields kept as 4-bit codes]}: the kept fields and the exact device bytes of ResidentFrames(packed, ..., variant,
        indices, compact=compact), computed from the schema alone - and, with compact=True, from one pass on the host over the
        kept rows of every candidate field, which counts its distinct values."""
        return cls._plan(packed, config, variant, indices, compact)[0]

    @classmethod
    def _plan(cls, packed, config, variant, indices, compact):
        """(plan, {coded field: (palette f32 [16], count)})"""
        if variant not in ("vec", "img", "rad"):
            raise ValueError("variant must be 'vec', 'img' or 'rad', got %r" % (variant,))
        S = config.seq_len
        if variant != "img" and S > 1:
            raise NotImplementedError("seq_len > 1 runs on the image-map model only (variant 'img')")
        rows = np.arange(len(packed), dtype=np.int64) if indices is None else np.asarray(list(indices), dtype=np.int64)
        if rows.size and (rows.min() < 0 or rows.max() >= len(packed)):
            raise IndexError("sample index out of range")
        n = len(rows)

        def frames(key, count):
            items = packed.fields[key]["items"] if packed.fields[key]["kind"] == "list" else [packed.fields[key]]
            if len(items) < count:
                raise ValueError("the store holds %d %s frame(s) per sample, the model reads %d" % (len(items), key, count))
            return [it["name"] for it in items[:count]]

        arrays = frames("fronts", S) + frames("lidars", S)
        if variant == "img":
            arrays += frames("maps", S)
        else:
            arrays += frames("vectormaps", 1)      # the lane set of frame 0 is the one MMFN._pack reads
        if variant == "rad":
            arrays += frames("radar", 1) + frames("radar_adj", 1)
        fields, palettes = {}, {}
        for nm in arrays:
            src = packed.arrays[nm]
            if src.dtype not in (np.uint8, np.float32, np.float64):
                raise ValueError("ResidentFrames: field %s has dtype %s (u8, f32 and f64 are supported)" % (nm, src.dtype))
            esz = 1 if src.dtype == np.uint8 else 4
            row = int(np.prod(src.shape[1:], dtype=np.int64))
            if nm in packed.offsets:
                off = packed.offsets[nm]
                fields[nm] = int((off[1:] - off[:-1])[rows].sum()) * row * esz
                fields[nm + ".row_off"] = (n + 1) * 8
            else:
                pal = cls._scan(src, rows) if compact and esz == 4 and row % 2 == 0 else None
                if pal is not None:
                    palettes[nm] = pal
                    fields[nm] = n * (row // 2)
                    fields[nm + ".palette"] = 64
                else:
                    fields[nm] = n * row * esz
        fields["target_point"] = n * 2 * 4
        fields["velocity"] = n * 4
        n_wp = len(packed.fields["waypoints"]["items"]) - S
        fields["waypoints"] = n * n_wp * 2 * 4
        if len(arrays) + 3 > 16:
            raise ValueError("a batch of %d fields does not fit the 16 fields of one gather launch" % (len(arrays) + 3))
        return {"fields": fields, "bytes": int(sum(fields.values())), "arrays": arrays, "rows": rows,
                "compact": list(palettes)}, palettes

    @staticmethod
    def _scan(src, take):
        """Pass 1 of a coded upload: (palette, count) of src[take] ([n, ...] f32 / f64), None as soon as a 17th value appears."""
        row = int(np.prod(src.shape[1:], dtype=np.int64))
        flat = src.reshape(src.shape[0], row)
        step = max(1, _BOUNCE_BYTES // max(1, row * 4))
        known = []
        for r0 in range(0, len(take), step):
            if not _more_patterns(_f32_bits(flat[take[r0:r0 + step]]), known):
                return None
        return _palette(known), len(known)

    @staticmethod
    def _labels(packed, config, rows):
        """target_point [n, 2], velocity [n] and gt [n, pred_len, 2] with the expressions of stage_batch, before its f32 rounding."""
        data = {k: packed._gather(packed.fields[k], rows, False) for k in ("target_point", "velocity", "waypoints")}
        S, wps = config.seq_len, data["waypoints"]
        return {"target_point": torch.stack(list(data["target_point"]), dim=1), "velocity": data["velocity"],
                "waypoints": torch.stack([torch.stack(list(wps[i]), dim=1) for i in range(S, len(wps))], dim=1)}

    def _upload(self, src, take, bounce, palette=None):
        """src[take] -> device tensor [len(take), row] (u8 as u8, f32 / f64 as f32), through the pinned bounce buffer.  With
        `palette` = (f32 [16], count) the chunks are encoded into the buffer and the tensor is u8 [len(take), row / 2]: pass 2 of
        a coded upload, the device never holds the f32 form."""
        dt = torch.uint8 if src.dtype == np.uint8 or palette is not None else torch.float32
        esz = 1 if dt == torch.uint8 else 4
        n_src = int(np.prod(src.shape[1:], dtype=np.int64))
        row = n_src // 2 if palette is not None else n_src
        out = torch.empty((max(1, len(take)), row), dtype=dt, device=self.device)[:len(take)]   # (never a NULL base)
        step = max(1, bounce.numel() // max(1, n_src * 4 if palette is not None else row * esz))   # (coded: its f32 form is the chunk)
        if row * esz > bounce.numel():
            raise ValueError("one row of %d bytes does not fit the %d-byte upload buffer" % (row * esz, bounce.numel()))
        flat = src.reshape(src.shape[0], n_src)
        for r0 in range(0, len(take), step):
            r1 = min(len(take), r0 + step)
            stage = bounce[:(r1 - r0) * row * esz].view(dt).view(r1 - r0, row)
            if palette is not None:
                _encode_bits(_f32_bits(flat[take[r0:r1]]), palette[0], palette[1], out=stage.numpy())
            elif src.dtype == np.float64:
                stage.numpy()[...] = flat[take[r0:r1]]          # float64 -> float32, round to nearest as torch's .to()
            else:
                np.take(flat, take[r0:r1], axis=0, out=stage.numpy(), mode="clip")
            out[r0:r1].copy_(stage)                            # synchronous: the buffer is free again when it returns
        return out

    def __len__(self):
        return self.n

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.tensors.values())

    def rows_of(self, sample_ids):
        """Resident rows of global sample ids; IndexError for one that is not resident."""
        ids = np.asarray(list(sample_ids), dtype=np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= len(self._row_of)):
            raise IndexError("sample index out of range")
        rows = self._row_of[ids]
        if ids.size and rows.min() < 0:
            raise IndexError("sample %d is not resident on this rank" % int(ids[int(np.argmin(rows))]))
        return rows

    def camera_frames(self):
        """The resident camera tensors, frame by frame ([n, 3 * H * W] u8 / f32 each), after checking that the jitter kernel can
        take them: ValueError for a camera field that is not [3, H, W] u8 / f32."""
        names = self.plan_["arrays"][:self.seq_len]
        for nm in names:
            shape, t = self.shapes[nm], self.tensors[nm]
            if len(shape) != 3 or shape[0] != 3 or shape != self.shapes[names[0]] or t.dtype not in (torch.uint8, torch.float32) \
                    or t.dtype != self.tensors[names[0]].dtype or nm + ".palette" in self.tensors:
                raise ValueError("camera jitter needs [3, H, W] u8 or f32 camera frames; field %s is %s %s%s" % (
                    nm, str(t.dtype).replace("torch.", ""), list(shape), " kept as 4-bit codes" if nm + ".palette" in self.tensors else ""))
        return [self.tensors[nm] for nm in names]

    def lidar_frames(self):
        """(the resident LiDAR tensors frame by frame, their palettes or None): [n, C * H * W] u8 / f32 each, or [n, C * H * W / 2]
        codes with one f32 [16] palette per frame, after checking that the augmenting gather can take them: ValueError for a
        LiDAR field that is not [C, H, W], or whose frames differ in shape, dtype or form."""
        S = self.seq_len
        names = self.plan_["arrays"][S:2 * S]
        coded = [nm + ".palette" in self.tensors for nm in names]
        for nm in names:
            shape, t = self.shapes[nm], self.tensors[nm]
            if len(shape) != 3 or shape != self.shapes[names[0]] or t.dtype not in (torch.uint8, torch.float32) \
                    or t.dtype != self.tensors[names[0]].dtype or any(c != coded[0] for c in coded):
                raise ValueError("LiDAR dropout needs [C, H, W] u8, f32 or 4-bit coded LiDAR frames, all of one form; field %s is %s %s%s" % (
                    nm, str(t.dtype).replace("torch.", ""), list(shape), " kept as 4-bit codes" if nm + ".palette" in self.tensors else ""))
        return [self.tensors[nm] for nm in names], ([self.tensors[nm + ".palette"] for nm in names] if coded[0] else None)

    def lane_field(self):
        """(the resident lane rows f32 [rows, nodes * 5], their prefix table) after checking that the augmenting gather can take
        them: ValueError for a store without a lane field (variant 'img') or one that is not f32 [nodes, 5]."""
        if self.variant == "img":
            raise ValueError("MapNoise: shift, yaw_deg and lane_drop act on the lane set, which an 'img' store does not hold "
                             "(target_shift works on every variant)")
        nm = self.plan_["arrays"][2 * self.seq_len]
        shape, t = self.shapes[nm], self.tensors[nm]
        if len(shape) != 2 or shape[1] != 5 or t.dtype != torch.float32:
            raise ValueError("map noise needs f32 lanes of [nodes, 5]; field %s is %s %s" % (nm, str(t.dtype).replace("torch.", ""), list(shape)))
        return t, self.tensors[nm + ".row_off"]

    def radar_field(self):
        """The resident radar rows f32 [n, 405] after checking that the radar launch can take them: ValueError for a store without
        a radar field (variants 'vec' and 'img') or one that is not f32 [81, 5] with an [81, 81] adjacency."""
        if self.variant != "rad":
            raise ValueError("RadarNoise acts on the radar returns, which a %r store does not hold (SpeedNoise works on every "
                             "variant)" % (self.variant,))
        nm, adj = self.plan_["arrays"][2 * self.seq_len + 1:2 * self.seq_len + 3]
        shape, t = self.shapes[nm], self.tensors[nm]
        if shape != (RADAR_ROWS, 5) or self.shapes[adj] != (RADAR_ROWS, RADAR_ROWS) or t.dtype != torch.float32 or nm + ".palette" in self.tensors:
            raise ValueError("radar noise needs f32 radar rows of [%d, 5] with a [%d, %d] adjacency; field %s is %s %s, %s is %s" % (
                RADAR_ROWS, RADAR_ROWS, RADAR_ROWS, nm, str(t.dtype).replace("torch.", ""), list(shape), adj, list(self.shapes[adj])))
        return t

    def gather(self, index, rows, lane_bucket=None, jitter=None, augment=None):
        """(engine input dict, gt) of the batch whose resident rows are `rows` (host) = `index` (int64 device tensor, the same
        values): fresh tensors from the caching allocator and one gather launch on the current stream.  `jitter` = (CameraJitter,
        gray_mean f32 [n, S], state uint64 [2], sample_id int64 [n]), the last three on the device (ResidentLoader keeps them): the
        camera field then goes through the jitter launch, every other field through the gather launch as before.
        `augment` = {"sample_id": int64 [n], "camera": (CameraJitter, gray_mean, state), "lidar": (LidarDropout, state), "map":
        (MapNoise, state)}, each part optional: the LiDAR frames, the lane set and the target point a part touches leave the gather
        launch for one mmfn_gather_augment launch - at most three launches per batch.  ValueError for a lane-augmented batch of
        more than 4096 lanes per sample.  "degrade": (CameraDegrade, gray_mean, state) sends the camera field through
        mmfn_gather_camera_degrade instead of the jitter launch, with the "camera" part's blends and rectangle if there is one:
        still at most three launches.  "radar": (RadarNoise, state) takes radar and radar_adj, "speed": (SpeedNoise, state) takes
        velocity out of the gather launch and into one mmfn_gather_radar_speed launch, the fourth."""
        from . import ops
        B, S, dev, T = len(rows), self.seq_len, self.device, self.tensors
        arrays = self.plan_["arrays"]
        fields = []
        augment = augment or {}
        if jitter is None and "camera" in augment:
            jitter = tuple(augment["camera"]) + (augment["sample_id"],)
        degrade = augment.get("degrade")
        if degrade is not None and jitter is None:      # no blends, no rectangle: the launch still wants a state to read
            jitter = (CameraJitter(), degrade[1], degrade[2], augment["sample_id"])
        lidar, noise = augment.get("lidar"), augment.get("map")
        move_lanes = noise is not None and noise[0].lanes_active
        move_target = noise is not None and noise[0].target_shift != 0.0
        radar, speed = augment.get("radar"), augment.get("speed")

        def frames(names, plain=True):   # frame s of sample b -> batch entry b * S + s, as MMFN._pack interleaves them
            shape = self.shapes[names[0]]
            out = torch.empty((B * S,) + shape, dtype=torch.float32, device=dev)
            if not plain:
                return out
            row = out[0].numel() if B else 0
            for s, nm in enumerate(names):
                fields.append(ops.gather_field(T[nm], out, row_elems=row, dst_stride=S * row, dst_offset=s * row,
                                               palette=T.get(nm + ".palette")))
            return out

        def dense(nm, shape, plain=True):
            out = torch.empty((B,) + shape, dtype=torch.float32, device=dev)
            if plain:
                fields.append(ops.gather_field(T[nm], out, row_elems=out[0].numel() if B else 0, palette=T.get(nm + ".palette")))
            return out

        inp = {"image": frames(arrays[:S], plain=jitter is None), "lidar": frames(arrays[S:2 * S], plain=lidar is None),
               "target_point": dense("target_point", (2,), plain=not move_target), "velocity": dense("velocity", (), plain=speed is None)}
        if self.variant == "img":
            inp["map"] = frames(arrays[2 * S:3 * S])
        else:
            nm = arrays[2 * S]
            lmax = int(self.lane_counts[rows].max()) if B else 0
            if lane_bucket and lane_bucket > 1 and lmax % lane_bucket:
                lmax += lane_bucket - lmax % lane_bucket       # what trainer._bucket_lanes would append, as zeros of the same launch
            if move_lanes and lmax > AUGMENT_MAX_LANES:
                raise ValueError("a lane-augmented batch takes at most %d lanes per sample, this one has %d" % (AUGMENT_MAX_LANES, lmax))
            inp["lane"] = torch.empty((B, lmax) + self.shapes[nm], dtype=torch.float32, device=dev)
            inp["lane_num"] = torch.empty(B, dtype=torch.int32, device=dev)
            if not move_lanes:
                fields.append(ops.gather_field(T[nm], inp["lane"], row_elems=T[nm].shape[1], row_off=T[nm + ".row_off"],
                                               count_out=inp["lane_num"], lmax=lmax))
        if self.variant == "rad":
            inp["radar"] = dense(arrays[2 * S + 1], (RADAR_ROWS, 5), plain=radar is None)
            inp["radar_adj"] = dense(arrays[2 * S + 2], (RADAR_ROWS, RADAR_ROWS), plain=radar is None)
        gt = dense("waypoints", tuple(T["waypoints"].shape[1:]))
        if B:
            ops.gather_batch(fields, index, self.n)
            if jitter is not None:
                aug, gray_mean, state, sample_id = jitter
                H, W = self.shapes[arrays[0]][1:]
                blends = dict(brightness=aug.brightness, contrast=aug.contrast, saturation=aug.saturation, erase_thresh=aug.erase_thresh,
                              erase_h=aug.erase_bounds(H), erase_w=aug.erase_bounds(W), sample_id=sample_id)
                if degrade is not None:
                    deg = degrade[0]
                    ops.gather_camera_degrade(self.camera_frames(), inp["image"], gray_mean, state, degrade[2], index, self.n,
                                              hue=deg.hue, blur_thresh=deg.blur_thresh, blur_sigma=deg.blur_sigma, blur_radius=deg.radius,
                                              noise_thresh=deg.noise_thresh, noise_std=deg.noise_std, **blends)
                else:
                    ops.gather_camera_jitter(self.camera_frames(), inp["image"], gray_mean, state, index, self.n, **blends)
            if lidar is not None or move_lanes or move_target:
                parts = {}
                if lidar is not None:
                    aug, state = lidar
                    srcs, palettes = self.lidar_frames()
                    H, W = self.shapes[arrays[S]][1:]
                    parts["lidar"] = dict(srcs=srcs, palettes=palettes, dst=inp["lidar"], state=state, cell_thresh=aug.cell_thresh,
                                          erase_thresh=aug.erase_thresh, erase_h=aug.erase_bounds(H), erase_w=aug.erase_bounds(W))
                if move_lanes:
                    src, row_off = self.lane_field()
                    parts["lanes"] = dict(src=src, row_off=row_off, dst=inp["lane"], count_out=inp["lane_num"],
                                          lane_thresh=noise[0].lane_thresh, shift=noise[0].shift, yaw_rad=noise[0].yaw_rad)
                if move_target:
                    parts["target"] = dict(src=T["target_point"], dst=inp["target_point"], shift=noise[0].target_shift)
                ops.gather_augment(index, self.n, sample_id=augment["sample_id"], map_state=noise[1] if noise is not None else None, **parts)
            if radar is not None or speed is not None:
                parts = {}
                if radar is not None:
                    aug, state = radar
                    depth_std, angle_std, _, velocity_std = aug.column_std
                    parts["radar"] = dict(src=self.radar_field(), dst=inp["radar"], adj=inp["radar_adj"], state=state,
                                          point_thresh=aug.point_thresh, depth_std=depth_std, angle_std=angle_std, velocity_std=velocity_std)
                if speed is not None:
                    aug, state = speed
                    parts["speed"] = dict(src=T["velocity"], dst=inp["velocity"], state=state, drop_thresh=aug.drop_thresh, std=aug.std)
                ops.gather_radar_speed(index, self.n, sample_id=augment["sample_id"], **parts)
        return inp, gt


def _as_i64(v):
    """The int64 with the bits of v mod 2^64 (the kernel reads the state as uint64)."""
    v = int(v) & _M64
    return v - (1 << 64) if v >> 63 else v


class ResidentLoader(object):
    """PackedLoader's twin over a ResidentFrames store: same arguments, same epoch order for the same seed, but it yields finished
    (engine input dict, gt) pairs - one gather launch per batch on the current stream, no thread, no pinned memory, no copy stream
    (DevicePrefetcher passes `device_resident` loaders through).  The epoch's index vector is uploaded once; the lane padding of a
    batch comes from the host's copy of the lane counts, so nothing is read back.  `lane_bucket` = k pads the lane sets to a
    multiple of k lanes right away (Trainer's own padding then finds nothing to do).  Sampler indices are global sample ids and
    are mapped to resident rows (IndexError for one that is not resident); without a sampler the order runs over the resident rows,
    so a sharded store shuffles inside its shard.
    `augment` = CameraJitter(...) jitters the camera frames inside their gather (a second launch per batch, for that field alone):
    the draws depend on (augment.seed, this loader's epoch counter, global sample id) only, so a shard draws what the full store
    would.  The loader then holds the frames' gray means (f32 [n, S], computed once here), the {seed, epoch} state the kernel reads
    and the sample ids, all on the device and none of them in the store.  `augment` = Augment(camera=, lidar=, map=) adds LiDAR
    dropout, lane dropout and map noise (LidarDropout, MapNoise): the fields they touch go through a third launch, each part with
    a state of its own; a part that is None or whose strengths are all zero stays in the plain launch, and Augment(camera=j) is
    augment=j.  Augment(degrade=CameraDegrade(...)) adds a hue shift, a Gaussian blur and sensor noise to the camera frames: the
    camera launch is then mmfn_gather_camera_degrade, with the camera part's blends and rectangle if there is one, and the loader
    holds a degrade state (and the gray means and sample ids, with or without a CameraJitter).  Augment(radar=RadarNoise(...),
    speed=SpeedNoise(...)) drops and perturbs the radar returns of a 'rad' store (ValueError on another variant) and rebuilds their
    adjacency, and perturbs or zeroes the speed input of any variant: radar, radar_adj and velocity then go through a fourth, small
    launch (mmfn_gather_radar_speed), each part with a state of its own (radar_state, speed_state).  None (the default) is the plain path, bit for bit; build validation loaders without it.  PackedLoader and the
    pickle loaders are not augmented."""
    device_resident = True

    def __init__(self, resident, batch_size, shuffle=False, sampler=None, seed=0, drop_last=False, lane_bucket=None, augment=None):
        self.resident, self.batch_size, self.shuffle, self.sampler = resident, int(batch_size), shuffle, sampler
        self.seed, self.drop_last, self.lane_bucket = seed, drop_last, lane_bucket
        self.epoch = 0
        self.augment = augment
        if augment is None:
            return
        if not isinstance(augment, (CameraJitter, Augment)):
            raise TypeError("augment takes a CameraJitter or an Augment (or None), got %r" % (augment,))
        # what the augmenting launches read besides the store lives HERE: the store, its plan and its byte count stay as they are
        state = lambda: torch.zeros(2, dtype=torch.int64, device=resident.device)      # {seed, epoch}, the kernel's uint64[2]
        parts = Augment(camera=augment) if isinstance(augment, CameraJitter) else augment
        if isinstance(augment, CameraJitter) or (parts.camera is not None and parts.camera.active):
            self.gray_mean = self._gray_mean(resident)
            self.jitter_state = state()
        if parts.lidar is not None and parts.lidar.active:
            resident.lidar_frames()
            self.lidar_state = state()
        if parts.map is not None and parts.map.active:
            if parts.map.lanes_active:
                resident.lane_field()
            self.map_state = state()
        if parts.degrade is not None and parts.degrade.active:
            if not hasattr(self, "gray_mean"):
                self.gray_mean = self._gray_mean(resident)
            H, W = resident.shapes[resident.plan_["arrays"][0]][1:]
            if parts.degrade.blur_thresh and min(H, W) <= parts.degrade.radius:
                raise ValueError("CameraDegrade: a blur of radius %d needs camera frames larger than that, these are %d x %d" % (
                    parts.degrade.radius, H, W))
            self.degrade_state = state()
        if parts.radar is not None and parts.radar.active:
            resident.radar_field()
            self.radar_state = state()
        if parts.speed is not None and parts.speed.active:
            self.speed_state = state()
        if any(hasattr(self, nm) for nm in ("jitter_state", "lidar_state", "map_state", "degrade_state", "radar_state", "speed_state")):
            self.sample_id = torch.from_numpy(np.ascontiguousarray(resident.indices, dtype=np.int64)).to(resident.device)

    @staticmethod
    def _gray_mean(resident, chunk=32):
        """f32 [n, S] on the device: the mean of 0.299 R + 0.587 G + 0.114 B over every stored camera frame - the mean the contrast
        blend (the first stage) calls for.  Once per loader, a chunk of frames at a time, accumulated in fp64."""
        cams = resident.camera_frames()
        out = torch.empty(max(1, resident.n), len(cams), dtype=torch.float32, device=resident.device)[:resident.n]   # (never a NULL base)
        weights = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64, device=resident.device)
        for s, t in enumerate(cams):
            for r0 in range(0, resident.n, chunk):
                x = t[r0:r0 + chunk].view(-1, 3, t.shape[1] // 3).to(torch.float64)
                out[r0:r0 + chunk, s] = (x.mean(dim=2) * weights).sum(dim=1).to(torch.float32)
        return out

    def _order(self):
        return _epoch_order(len(self.resident), self.shuffle, self.sampler, self.seed, self.epoch)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.resident)
        return _num_batches(n, self.batch_size, self.drop_last)

    def _states(self):
        """Writes {seed, epoch} of every augmenting part and returns gather()'s keywords: the epoch counter that seeds the shuffle
        also keys the draws."""
        if self.augment is None:
            return {}
        put = lambda t, seed: t.copy_(torch.tensor([_as_i64(seed), _as_i64(self.epoch)], dtype=torch.int64))
        if isinstance(self.augment, CameraJitter):
            put(self.jitter_state, self.augment.seed)
            return {"jitter": (self.augment, self.gray_mean, self.jitter_state, self.sample_id)}
        parts = {}
        if hasattr(self, "jitter_state"):
            parts["camera"] = (self.augment.camera, self.gray_mean, put(self.jitter_state, self.augment.camera.seed))
        if hasattr(self, "lidar_state"):
            parts["lidar"] = (self.augment.lidar, put(self.lidar_state, self.augment.lidar.seed))
        if hasattr(self, "map_state"):
            parts["map"] = (self.augment.map, put(self.map_state, self.augment.map.seed))
        if hasattr(self, "degrade_state"):
            parts["degrade"] = (self.augment.degrade, self.gray_mean, put(self.degrade_state, self.augment.degrade.seed))
        if hasattr(self, "radar_state"):
            parts["radar"] = (self.augment.radar, put(self.radar_state, self.augment.radar.seed))
        if hasattr(self, "speed_state"):
            parts["speed"] = (self.augment.speed, put(self.speed_state, self.augment.speed.seed))
        if not parts:
            return {}
        parts["sample_id"] = self.sample_id
        return {"augment": parts}

    def __iter__(self):
        order = self._order()
        extra = self._states()
        self.epoch += 1
        res = self.resident
        rows = res.rows_of(order) if self.sampler is not None else np.asarray(order, dtype=np.int64)
        index = torch.from_numpy(rows).to(res.device)          # the whole epoch's indices: one upload
        pos = 0
        for chunk in _chunks(order, self.batch_size, self.drop_last):
            b = len(chunk)
            yield res.gather(index[pos:pos + b], rows[pos:pos + b], self.lane_bucket, **extra)
            pos += b


# ------------------------------------------------------------------------------------------ collation
def _stack(items):
    first = items[0]
    if isinstance(first, torch.Tensor):
        return torch.stack(list(items), 0)
    if isinstance(first, np.ndarray):
        return torch.stack([torch.as_tensor(x) for x in items], 0)
    if isinstance(first, (float, np.floating)):
        return torch.tensor([float(x) for x in items], dtype=torch.float64)
    if isinstance(first, (bool, int, np.integer)):
        return torch.tensor(list(items))
    if isinstance(first, (str, bytes)):
        return list(items)
    if isinstance(first, (tuple, list)):
        width = len(first)
        if any(len(x) != width for x in items):
            raise RuntimeError("each element in list of batch should be of equal size")
        return [_stack([x[j] for x in items]) for j in range(width)]
    raise TypeError("collate: unsupported field type %s" % type(first))


def _pad_lanes(lanes):
    """Ragged per-sample lane sets [L_b, 10, 5] -> [padded [B, Lmax, 10, 5], lane_nums i64[B], int Lmax]
    (data_utils.py:19-25)."""
    lanes = [torch.as_tensor(x) for x in lanes]
    nums = torch.tensor([x.shape[0] for x in lanes])
    lmax = int(nums.max().item())
    out = lanes[0].new_zeros((len(lanes), lmax) + tuple(lanes[0].shape[1:]))
    for b, x in enumerate(lanes):
        out[b, :x.shape[0]] = x
    return [out, nums, lmax]


def collate(samples):
    """List of FrameStore samples -> the batch dict Engine.train consumes."""
    out = {}
    for key in samples[0]:
        column = [s[key] for s in samples]
        if key == "vectormaps":
            seq = len(column[0])
            out[key] = [_pad_lanes([c[i] for c in column]) for i in range(seq)]
        else:
            out[key] = _stack(column)
    return out


collate_single_cpu = collate  # reference name


# ------------------------------------------------------------------------------------------ host -> device
def stage_batch(data, device, config, non_blocking=True):
    """Collated batch -> (MMFN.forward argument tuple, gt_waypoints [B, pred_len, 2]) on `device`
    (phase2_train_net.py:63-103).  uint8 frames are copied as uint8 and widened on the device."""
    dev = torch.device(device)

    def f32(t, narrow_first=True):
        t = torch.as_tensor(t)
        if t.dtype == torch.uint8:  # 1 byte/pixel over PCIe, widened by the GPU
            return t.to(dev, non_blocking=non_blocking).to(torch.float32)
        if narrow_first and t.dtype != torch.float32:
            t = t.to(torch.float32)
        return t.to(dev, non_blocking=non_blocking)

    n = config.seq_len
    fronts = [f32(data["fronts"][i]) for i in range(n)]
    lidars = [f32(data["lidars"][i]) for i in range(n)]
    maps = [f32(data["maps"][i]) for i in range(n)]
    lanes = [f32(data["vectormaps"][i][0]) for i in range(n)]
    lane_nums = [f32(data["vectormaps"][i][1]) for i in range(n)]
    vectormaps = [lanes, lane_nums, data["vectormaps"][0][2]]
    radar = [f32(data["radar"][i]) for i in range(n)]
    radar_adj = [f32(data["radar_adj"]) for _ in range(n)]
    velocity = f32(data["velocity"])
    target_point = f32(torch.stack(list(data["target_point"]), dim=1))
    wps = data["waypoints"]
    gt = torch.stack([torch.stack(list(wps[i]), dim=1) for i in range(n, len(wps))], dim=1)
    return (fronts, lidars, maps, vectormaps, radar, radar_adj, target_point, velocity), f32(gt)


class DevicePrefetcher(object):
    """Iterates a loader of collated batches one batch ahead: the next batch's host->device copies run on a
    dedicated copy stream while the current step computes (the reference copies synchronously inside the
    step, phase2_train_net.py:78-91)."""

    def __init__(self, loader, device, config, variant="vec"):
        limit_host_threads()
        self.loader, self.device, self.config, self.variant = loader, torch.device(device), config, variant
        # a loader that declares `device_resident` (ResidentLoader) yields finished (engine input, gt) pairs on the consumer's
        # stream: nothing to stage, so no copy stream either
        self.resident = bool(getattr(loader, "device_resident", False))
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" and not self.resident else None

    def __len__(self):
        return len(self.loader)

    def _do_stage(self, data, non_blocking):
        if "rgb_u8" in data:  # RawFrameStore / collate_raw batches
            return stage_raw_batch(data, self.device, self.config, self.variant, non_blocking=non_blocking)
        return stage_batch(data, self.device, self.config, non_blocking=non_blocking)

    def _stage(self, data):
        if self.stream is None:
            return self._do_stage(data, False), None
        with torch.cuda.stream(self.stream):
            staged = self._do_stage(_pin(data), True)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        return staged, ready

    def __iter__(self):
        if self.resident:
            for item in self.loader:
                yield item
            return
        nxt = None
        for data in self.loader:
            cur, nxt = nxt, self._stage(data)
            if cur is not None:
                yield self._hand_over(cur)
        if nxt is not None:
            yield self._hand_over(nxt)

    def _hand_over(self, item):
        staged, ready = item
        if ready is not None:
            torch.cuda.current_stream(self.device).wait_event(ready)
            for t in _tensors(staged):
                t.record_stream(torch.cuda.current_stream(self.device))
        return staged


def _pin(obj):
    if isinstance(obj, torch.Tensor):
        return obj if obj.is_pinned() else obj.pin_memory()
    if isinstance(obj, dict):
        return {k: _pin(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_pin(v) for v in obj)
    return obj


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            for t in _tensors(v):
                yield t
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            for t in _tensors(v):
                yield t


def make_loader(store, batch_size, shuffle=False, sampler=None, num_workers=8, pin_memory=False):
    """DataLoader with this module's collate (phase2_train_net.py:268-274); raw-route stores get collate_raw."""
    fn = collate_raw if isinstance(store, RawFrameStore) else collate
    return torch.utils.data.DataLoader(store, batch_size=batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                                       num_workers=num_workers, pin_memory=pin_memory, collate_fn=fn)


def shard_sampler(store, rank, world, shuffle=True, seed=0):
    """Per-rank sample shard, as DistributedSampler does for the reference (phase2_train_net.py:265-266)."""
    return torch.utils.data.distributed.DistributedSampler(store, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)


# ------------------------------------------------------------------------------------------ raw recorded routes (row f2)
class RawFrameStore(torch.utils.data.Dataset):
    """Reader of the recorded CARLA routes themselves (`CARLA_Data`, dataloader.py:11-268): <root>/<route>/{rgb_front,
    maps,lidar,radar,vectormap,measurements}/NNNN.{png,npy,json}.  Frame indexing follows the reference exactly
    (first frame of a route skipped, the last pred_len + 1 frames have no future waypoints, dataloader.py:72-75).

    Unlike the reference, a sample carries the RAW sensor frames - the uint8 camera image as recorded and the XYZI
    point list - because crop / normalise / y-flip / histogram run on the GPU inside the network's ingest kernels
    (csrc/ingest.hip); the host only decodes files and does the O(10) pose arithmetic.

    seq_len > 1: a sample carries seq_len camera / map / lane / radar frames, and seq_len LiDAR sweeps, each moved into the ego
    frame of the LAST one (y flip + `ego_transform` = the reference's transform_2d_points, dataloader.py:225-231, 311-334) on the
    host in float64 - `lidar_pts` is then a list and `lidar_in_ego_frame` tells the device side not to flip again.  The reference
    itself runs that block once, after its frame loop, and so returns only the last sweep's histogram (its seq_len > 1 samples
    do not fit its own model); `lidar_reference_frame` = seq_len - 1 names that one."""

    def __init__(self, roots, config):
        self.seq_len, self.pred_len = config.seq_len, config.pred_len
        self.frames = []
        for sub_root in ([roots] if isinstance(roots, str) else list(roots)):
            for route in sorted(os.listdir(sub_root)):
                route_dir = os.path.join(sub_root, route)
                if os.path.isfile(route_dir):
                    continue
                n = (len(os.listdir(os.path.join(route_dir, "rgb_front"))) - self.pred_len - 2) // self.seq_len
                for seq in range(n):
                    ids = ["%04d" % (seq * self.seq_len + 1 + i) for i in range(self.seq_len + self.pred_len)]
                    meas = [_read_json(os.path.join(route_dir, "measurements", k + ".json")) for k in ids]
                    cur = meas[self.seq_len - 1]
                    thetas = [m["theta"] for m in meas]
                    # (the reference zeroes a NaN heading only for the future frames at scan time and for the current
                    # ones at load time, dataloader.py:133-137,224-226: same effect)
                    thetas = [0.0 if np.isnan(t) else t for t in thetas]
                    now = ids[:self.seq_len]
                    self.frames.append({
                        "rgb": [os.path.join(route_dir, "rgb_front", k + ".png") for k in now],
                        "map": [os.path.join(route_dir, "maps", k + ".png") for k in now],
                        "lidar": [os.path.join(route_dir, "lidar", k + ".npy") for k in now],
                        "radar": [os.path.join(route_dir, "radar", k + ".npy") for k in now],
                        "vectormap": [os.path.join(route_dir, "vectormap", k + ".npy") for k in now],
                        "x": [m["x"] for m in meas], "y": [m["y"] for m in meas], "theta": thetas,
                        "x_command": cur["x_command"], "y_command": cur["y_command"], "steer": cur["steer"],
                        "throttle": cur["throttle"], "brake": cur["brake"], "command": cur["command"], "velocity": cur["speed"],
                    })

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        from PIL import Image
        f = self.frames[i]
        S = self.seq_len
        ego = S - 1
        lanes = []
        for t in range(S):
            vm, j = f["vectormap"][t], i
            while not os.path.exists(vm):  # frames recorded without a lane file borrow a neighbour's (dataloader.py:199-207)
                j = j - 1 if j - 1 >= 0 else j + 1
                vm = self.frames[j]["vectormap"][t]
            lanes.append(torch.from_numpy(np.load(vm)))
        rgbs = [torch.from_numpy(np.array(Image.open(p).convert("RGB"), dtype=np.uint8)) for p in f["rgb"]]
        sample = {
            "vectormaps": lanes,
            "radar": [radar_to_size(np.load(p)) for p in f["radar"]],
            "waypoints": local_waypoints(f["x"], f["y"], f["theta"], ego),
            "target_point": local_target_point(f["x_command"], f["y_command"], f["x"][ego], f["y"][ego], f["theta"][ego]),
            "steer": f["steer"], "throttle": f["throttle"], "brake": f["brake"], "command": f["command"], "velocity": f["velocity"],
        }
        if S == 1:
            sample["rgb_u8"] = rgbs[0]
            sample["lidar_pts"] = torch.from_numpy(np.load(f["lidar"][0]).astype(np.float32)[:, :4])
        else:
            sample["rgb_u8"] = torch.stack(rgbs, 0)
            sweeps = []
            for t in range(S):
                raw = np.load(f["lidar"][t])
                xyz = raw[..., :3].astype(np.float64)
                xyz[:, 1] *= -1                                              # dataloader.py:227
                xyz = ego_transform(xyz, np.pi / 2 - f["theta"][t], -f["x"][t], -f["y"][t],
                                    np.pi / 2 - f["theta"][ego], -f["x"][ego], -f["y"][ego])
                pts = np.zeros((len(xyz), 4), np.float64)
                pts[:, :3] = xyz
                if raw.shape[1] > 3:
                    pts[:, 3] = raw[:, 3]
                sweeps.append(pts)
            sample["lidar_pts"] = sweeps          # float64 [N_t, 4] each, already in the ego frame
            sample["lidar_in_ego_frame"] = True
            sample["lidar_reference_frame"] = ego
        if all(os.path.exists(p) for p in f["map"]):
            sample["maps"] = [torch.from_numpy(np.ascontiguousarray(np.transpose(np.asarray(Image.open(p)), (2, 0, 1)))) for p in f["map"]]
        sample["radar_adj"] = radar_adjacency(sample["radar"][0])
        return sample


def _read_json(path):
    import json
    with open(path) as f:
        return json.load(f)


FAR_POINT = 1.0e6  # padding x coordinate: outside every histogram bin (np.histogramdd ignores it the same way)


def collate_raw(samples):
    """RawFrameStore samples -> batch with `rgb_u8` [B,H,W,3] u8 and `lidar_pts` [B,Nmax,4] padded with far points;
    everything else as `collate`."""
    skip = ("rgb_u8", "lidar_pts", "lidar_in_ego_frame", "lidar_reference_frame")
    rest = [{k: v for k, v in s.items() if k not in skip} for s in samples]
    out = collate(rest)
    out["rgb_u8"] = torch.stack([s["rgb_u8"] for s in samples], 0)          # [B, H, W, 3] or, seq_len > 1, [B, S, H, W, 3]
    several = isinstance(samples[0]["lidar_pts"], (list, tuple))
    sweeps = [s["lidar_pts"] if several else [s["lidar_pts"]] for s in samples]
    S = len(sweeps[0])
    nmax = max(int(p.shape[0]) for sw in sweeps for p in sw)
    nmax = (nmax + 1023) // 1024 * 1024  # few distinct shapes -> few buffer sets / graph captures downstream
    pts = torch.zeros(len(samples), S, nmax, 4, dtype=torch.float32)
    pts[:, :, :, 0] = FAR_POINT
    for b, sw in enumerate(sweeps):
        for t, p in enumerate(sw):
            p = torch.as_tensor(np.asarray(p)).to(torch.float32)
            pts[b, t, :p.shape[0], :p.shape[1]] = p
    out["lidar_pts"] = pts if several else pts[:, 0]                      # [B, S, N, 4] (ego frame already) / [B, N, 4] (raw)
    out["lidar_in_ego_frame"] = bool(samples[0].get("lidar_in_ego_frame", False))
    return out


def stage_raw_batch(data, device, config, variant="vec", non_blocking=True):
    """collate_raw batch -> (Engine input dict, gt_waypoints) on `device`: the frames stay uint8 / XYZI; the y flip of
    dataloader.py:233 is requested from the splat kernel."""
    dev = torch.device(device)
    to = lambda t, dt=None: torch.as_tensor(t).to(dt or torch.as_tensor(t).dtype).to(dev, non_blocking=non_blocking)
    if variant != "img" and config.seq_len > 1:
        # with several frames per sample the ego frame is the LAST one (waypoints, target point, sweeps moved into it); lanes and
        # radar below are frame 0's.  The vector-map / radar models cannot run seq_len > 1 anyway (Engine.__init__, as the
        # reference: model_vec.py:226) - refuse here too instead of pairing frame-0 lanes with last-frame labels
        raise NotImplementedError("raw batches with seq_len > 1 exist for the image-map model only (variant 'img')")
    lane, lane_num, _ = data["vectormaps"][0]
    rgb, pts = to(data["rgb_u8"]), to(data["lidar_pts"])
    if rgb.dim() == 5:   # seq_len > 1: a sample's frames become consecutive batch entries (model_vec.py:506-508)
        rgb, pts = rgb.flatten(0, 1), pts.flatten(0, 1)
    inp = {
        "rgb_u8": rgb, "lidar_pts": pts, "lidar_flip_y": not data.get("lidar_in_ego_frame", False),
        "target_point": to(torch.stack(list(data["target_point"]), dim=1), torch.float32),
        "velocity": to(data["velocity"], torch.float32),
    }
    if variant == "img":
        maps = [to(m).to(torch.float32) for m in data["maps"][:config.seq_len]]
        inp["map"] = maps[0] if len(maps) == 1 else torch.stack(maps, dim=1).flatten(0, 1)
    else:
        inp["lane"] = to(lane, torch.float32)
        inp["lane_num"] = to(lane_num, torch.int32)
    if variant == "rad":
        inp["radar"] = to(data["radar"][0], torch.float32)
        inp["radar_adj"] = to(data["radar_adj"], torch.float32)
    wps = data["waypoints"]
    n = config.seq_len
    gt = torch.stack([torch.stack(list(wps[i]), dim=1) for i in range(n, len(wps))], dim=1)
    return inp, to(gt, torch.float32)


def preprocess_routes(store, out_dir, device, batch_size=16):
    """Phase 1 on the GPU (run_steps/phase1_preprocess_data.py:42-48): RawFrameStore -> one PRE_Data pickle per frame, with
    the camera crop and the LiDAR histogram produced by the ingest kernels.  Returns the number of files written."""
    from . import ops
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device(device)
    n = 0
    for start in range(0, len(store), batch_size):
        samples = [store[i] for i in range(start, min(len(store), start + batch_size))]
        batch = collate_raw(samples)
        pts = batch["lidar_pts"].to(dev)
        S = 1
        if pts.dim() == 4:   # seq_len > 1: [B, S, N, 4], already in the ego frame (no y flip on the device)
            S = pts.shape[1]
            pts = pts.flatten(0, 1)
        bev = ops.lidar_splat(pts, torch.empty(len(samples) * S, 256, 256, 2, device=dev), flip_y=not batch["lidar_in_ego_frame"])
        bev = bev.permute(0, 3, 1, 2).cpu().numpy().reshape(len(samples), S, 2, 256, 256)
        for k, s in enumerate(samples):
            frames = s["rgb_u8"].numpy()
            frames = frames[None] if frames.ndim == 3 else frames
            H, W = frames.shape[1:3]
            rec = {key: s[key] for key in ("vectormaps", "radar", "waypoints", "target_point", "steer", "throttle", "brake", "command",
                                           "velocity") if key in s}
            rec["fronts"] = [torch.from_numpy(np.ascontiguousarray(np.transpose(fr[H // 2 - 128:H // 2 + 128, W // 2 - 128:W // 2 + 128], (2, 0, 1))))
                             for fr in frames]
            rec["lidars"] = [np.ascontiguousarray(bev[k, t]) for t in range(S)]
            rec["maps"] = s.get("maps", [torch.zeros(3, 256, 256, dtype=torch.uint8) for _ in range(S)])
            with open(os.path.join(out_dir, "%d.pkl" % (start + k)), "wb") as fd:
                pickle.dump(rec, fd)
            n += 1
    return n
