"""Epoch loop, validation and checkpoint / resume around the HIP training step.

Restates the reference's `Engine` (run_steps/phase2_train_net.py:44-220) and the resume block of its
`main` (:288-302).  Same attributes (`cur_epoch, cur_iter, bestval, bestval_epoch, train_loss, val_loss`),
same files in the log directory:
    recent.log        JSON {epoch, iter, bestval, bestval_epoch, train_loss, val_loss}        (:193-204)
    best_model.pth    model.state_dict() when the validation loss improved                    (:207-211)
    best_optim.pth    optimizer.state_dict() (torch.optim.AdamW layout)                       (:209)
    model.pth, recent_optim.pth   always                                                      (:215-216)
(a run with a weight average, averaging.AveragedMMFN, also writes averaged_model.pth and best_averaged_model.pth)
so a run can be resumed by either implementation.  Differences, all on the host side:
  * the step is the fused one (forward + L1 + backward + bucketed all-reduce + AdamW on device buffers);
    `fused=False` runs the reference's literal sequence through autograd instead;
  * the loss is accumulated on the device and read back once per `log_every` steps, not every step
    (:109 forces a host sync per step; anomaly mode :107 is not reproduced);
  * checkpoints always carry un-prefixed keys (the reference mixes `module.`-prefixed and plain keys
    under DDP, :208 vs :216).
"""
import json
import os

import torch

from . import data as D
from . import ops
from .parallel import StaticBatchStep, StaticEvalStep


def _evict_lru(cache):
    """Drop the least recently used entry of a capture cache (dict in LRU order) and free it - hipGraph exec, its private
    pool, the static input copies - HERE: nothing may still be replaying it, so wait for the device first.  The entry is popped
    inside this function and never handed in as an argument: a caller's argument slot would keep the capture alive until this
    call returned, i.e. past gc.collect() / drain_graveyard().  The "seen" / "eager" placeholders hold nothing."""
    state = cache.pop(next(iter(cache)))
    if isinstance(state, str) or state is None:
        return
    import gc
    from . import graphs
    torch.cuda.synchronize()
    del state                  # the last reference: Graph.__del__ parks the capture in the graveyard now
    gc.collect()
    graphs.drain_graveyard()   # the capture's hipGraphExecs are destroyed here, with the device idle


class Trainer(object):
    def __init__(self, device, log_dir, cur_epoch=0, cur_iter=0):
        self.cur_epoch = cur_epoch
        self.cur_iter = cur_iter
        self.bestval_epoch = cur_epoch
        self.train_loss = []
        self.val_loss = []
        self.bestval = 1e10
        self.device = device
        self.logdir = log_dir
        self.max_captured_shapes = 12  # ragged batches (lane buckets, LiDAR sizes) multiply the shapes: bound the captures
        # weight average (averaging.AveragedMMFN): its validation losses and best value; recent.log carries them only for runs
        # that have an average
        self.val_loss_average = []
        self.bestval_average = 1e10
        # optimizer steps the non-finite guard skipped (train(skip_nonfinite=True)); None = the option was never on, and recent.log
        # then has no such key
        self.skipped_steps = None

    # ------------------------------------------------------------------ one epoch of training
    def train(self, model, dataloader_train, config, optimizer, dp=None, fused=True, log_every=50, on_log=None, graph=True,
              lane_bucket=16, accum_steps=1, clip_grad_norm=None, average=None, skip_nonfinite=False, loss=None, sample_weight=None):
        """One epoch.  graph=True (fused path): the second batch of a given shape captures the step into hipGraphs over
        static input buffers and every later batch of that shape only copies its inputs and replays (the first one runs
        eagerly and sizes the buffers); lane sets are zero-padded to a multiple of `lane_bucket` lanes so that ragged
        batches fall into few shapes (padded lanes are masked by lane_num: outputs are unchanged, parameter gradients to
        the last ulp of their row sums).

        accum_steps = k: gradient accumulation, one optimizer step per k consecutive batches on the mean of their
        gradients (each batch's own mean L1 loss, BatchNorm statistics per batch); the epoch's last, partial group of r < k
        batches is stepped at the end of the epoch with 1 / r, so no gradient crosses an epoch (or checkpoint) boundary.
        cur_iter keeps counting batches.  Under data parallelism every rank must pass the same accum_steps (a
        DistributedSampler gives every rank the same number of batches), and the gradient all-reduce runs once per group.
        clip_grad_norm = max_norm: torch.nn.utils.clip_grad_norm_ over all trained parameters before each optimizer step
        (inf: only measure); on_log then also gets "grad_norm", the last optimizer step's global norm.  Each variant of the
        step (micro-step, group-closing step) is a captured shape of its own, bounded by max_captured_shapes.

        average (averaging.AveragedMMFN): updated after every optimizer step of the epoch - attached to the engine for the
        epoch, inside the fused step's AdamW launch (eager and replayed, captured as shapes of their own; micro-steps do not
        update it); fused=False: its update_parameters() after each optimizer.step().

        skip_nonfinite: the engine's non-finite guard (Engine.set_nonfinite_guard) is armed for the epoch: an optimizer step
        whose gradient norm is not finite is skipped on the device - weights, moments, BatchNorm statistics and the average stay
        as they were, the whole accumulation group is dropped.  on_log and recent.log gain "skipped_steps" (the run's count), the
        epoch's train_loss is the mean over the batches with a finite loss, and a log window (log_every batches, or the rest of
        the epoch) in which EVERY optimizer step was skipped raises RuntimeError naming tensors with non-finite gradients.

        loss (losses.WaypointLoss): the objective of the epoch's training steps - set on the engine for the epoch (Engine.set_loss)
        and the previous one restored afterwards; None leaves the engine's loss as it is.  fused=False calls loss.reference in the
        place of the L1 loss.  sample_weight: a callable (inp, gt) -> [B] float32 device tensor, evaluated per batch outside any
        capture; its result travels as inp["sample_weight"] (weights from gt's lateral extent, from inp["velocity"], ...).
        train_loss and on_log's "loss" are the objective; when it is not the plain mean L1, on_log also gets "l1", the window's mean
        of the batches' unweighted L1 (summed on the device, read with the loss).  validate() stays mean L1."""
        if skip_nonfinite and not fused:
            raise NotImplementedError("skip_nonfinite is an option of the fused step (fused=True)")
        if (average is None and not skip_nonfinite and loss is None) or not fused:
            return self._train(model, dataloader_train, config, optimizer, dp, fused, log_every, on_log, graph, lane_bucket,
                               accum_steps, clip_grad_norm, average, False, loss, sample_weight)
        eng = model._engine_for()
        if average is not None:
            eng.attach_average(average)
        previous = eng.loss
        try:
            if loss is not None:
                eng.set_loss(loss)
            if skip_nonfinite:
                eng.set_nonfinite_guard(True)
            return self._train(model, dataloader_train, config, optimizer, dp, fused, log_every, on_log, graph, lane_bucket,
                               accum_steps, clip_grad_norm, average, skip_nonfinite, loss, sample_weight)
        finally:
            if skip_nonfinite:
                eng.set_nonfinite_guard(False)
            if loss is not None:
                eng._install_loss(previous)
            if average is not None:
                eng.detach_average()

    def _train(self, model, dataloader_train, config, optimizer, dp, fused, log_every, on_log, graph, lane_bucket, accum_steps,
               clip_grad_norm, average, guard=False, loss_fn=None, sample_weight=None):
        """Trainer.train's epoch loop (an attached average, the armed guard and the engine's loss are the caller's)."""
        accum_steps = int(accum_steps)
        if accum_steps < 1:
            raise ValueError("accum_steps must be >= 1, got %d" % accum_steps)
        accumulating = accum_steps > 1 or clip_grad_norm is not None or guard
        if accumulating and not fused:
            raise NotImplementedError("accum_steps / clip_grad_norm are options of the fused step (fused=True)")
        model.train()
        eng = model._engine_for()
        if accumulating and eng.accum_pending:
            raise RuntimeError("%d micro-step(s) are pending from outside this epoch" % eng.accum_pending)
        in_group = 0
        if not hasattr(self, "_static_steps"):
            self._static_steps = {}      # input-shape signature -> "seen" | "eager" | StaticBatchStep, in LRU order
        total = torch.zeros(1, dtype=torch.float32, device=model._layout.device)
        window = torch.zeros_like(total)
        num_batches = 0
        if loss_fn is None:
            loss_fn = eng.loss   # (a loss set on the engine outside this epoch: the autograd path follows it too)
        # the objective is not the plain mean L1: the batches' unweighted L1 is summed beside it for on_log's "l1"
        weighted = sample_weight is not None or not (loss_fn is None or loss_fn.is_plain())
        l1_window = torch.zeros_like(total) if weighted else None
        if guard:
            # losses are summed over the batches where they are finite, counted on the device: [epoch, window]
            finite = torch.zeros(2, dtype=torch.float32, device=model._layout.device)
            if self.skipped_steps is None:
                self.skipped_steps = 0
            skipped_base = self.skipped_steps - int(eng.skipped_steps.item())   # the run's count = base + the engine's
            window_steps, window_skipped0 = 0, self.skipped_steps
        batches = D.DevicePrefetcher(dataloader_train, self.device, config, variant=model.variant)
        # (accumulating: one batch of look-ahead tells the epoch's last batch, which closes the partial group)
        for (args, gt), last in (_with_last(batches) if accumulating else ((b, False) for b in batches)):
            if fused:
                inp = args if isinstance(args, dict) else model._pack(*args)  # raw-frame batches are engine inputs already
                # per-group (lr, beta1, beta2, eps, weight_decay): read every step, so an LR scheduler just works - they go
                # to the device table the AdamW kernel reads, captured graphs stay valid
                adam = dict(groups=_hyper_rows(optimizer))
                lr = optimizer.param_groups[0]["lr"]
                inp = _bucket_lanes(inp, lane_bucket)  # in both modes, so that eager and replayed steps are bit-identical
                if sample_weight is not None:   # evaluated here, outside the capture; an input of the step like any other
                    inp = dict(inp)
                    inp["sample_weight"] = sample_weight(inp, gt).to(torch.float32).contiguous()
                in_group += 1
                final = in_group == accum_steps or last   # (not accumulating: every batch is a group of its own, the plain step)
                loss = self._step_call(eng, dp, inp, gt, lr, adam, final, accum_steps > 1, clip_grad_norm, graph, average)
                if final:
                    in_group = 0
                    if guard:
                        window_steps += 1
                l1 = eng.sample_l1(gt.shape[0]) if weighted else None
                if l1 is not None:
                    l1 = l1.mean().view(1)
            else:
                if dp is not None or isinstance(args, dict):
                    raise NotImplementedError("the autograd path takes reference-format batches on one GPU; use fused=True")
                for p in model.parameters():
                    p.grad = None
                pred = model(*args)
                if weighted:
                    from .losses import PLAIN
                    sw = None if sample_weight is None else sample_weight(model._pack(*args), gt)
                    loss = (loss_fn or PLAIN).reference(pred, gt, sw)
                    l1 = torch.nn.functional.l1_loss(pred.detach(), gt).view(1)
                else:
                    loss = torch.nn.functional.l1_loss(pred, gt, reduction="none").mean()
                loss.backward()
                optimizer.step()
                if average is not None:
                    average.update_parameters(model)
                loss = loss.detach().view(1)
            if guard:
                good = torch.isfinite(loss)
                loss = torch.where(good, loss, torch.zeros_like(loss))
                finite += good.to(finite.dtype)
                if weighted and l1 is not None:
                    l1 = torch.where(good, l1, torch.zeros_like(l1))
            total += loss
            window += loss
            if weighted and l1 is not None:
                l1_window += l1
            self.cur_iter += 1
            num_batches += 1
            if guard and num_batches % log_every == 0:
                # one read per window: the skip count, and with it the check that the window made progress
                self.skipped_steps = skipped_base + int(eng.skipped_steps.item())
                self._check_progress(eng, window_steps, self.skipped_steps - window_skipped0)
                window_steps, window_skipped0 = 0, self.skipped_steps
            if on_log is not None and num_batches % log_every == 0:
                # (the objective and, beside it, the unweighted L1: one read of both)
                sums = (torch.cat((window, l1_window)) if weighted else window).tolist()
                if guard:   # (the window's mean over its finite losses)
                    count = max(float(finite[1].item()), 1.0)
                    rec = {"loss": sums[0] / count, "iter": self.cur_iter, "skipped_steps": self.skipped_steps}
                    finite[1] = 0
                else:
                    count = log_every
                    rec = {"loss": sums[0] / count, "iter": self.cur_iter}
                if weighted:
                    rec["l1"] = sums[1] / count
                    l1_window.zero_()
                if clip_grad_norm is not None:   # (None until the first optimizer step of the run)
                    rec["grad_norm"] = None if eng.last_grad_norm is None else float(eng.last_grad_norm.item())
                on_log(rec)
                window.zero_()
        if guard:
            self.skipped_steps = skipped_base + int(eng.skipped_steps.item())
            self._check_progress(eng, window_steps, self.skipped_steps - window_skipped0)
            self.train_loss.append(float(total.item()) / max(float(finite[0].item()), 1.0))
        else:
            self.train_loss.append(float(total.item()) / max(num_batches, 1))
        self.cur_epoch += 1
        return self.train_loss[-1]

    @staticmethod
    def _check_progress(eng, steps, skipped):
        """skip_nonfinite: a window whose optimizer steps were ALL skipped is a run that has stopped training - say which tensors'
        gradients are not finite (Engine.tensor_stats, the last step's gradient) instead of spinning."""
        if steps == 0 or skipped < steps:
            return
        names, table = eng.tensor_stats("grads")
        bad = [n for n, c in zip(names, table[:, 2].tolist()) if c > 0]
        raise RuntimeError("all %d optimizer step(s) since the last check were skipped: the gradient is not finite in %d of %d tensors "
                           "(%s%s)" % (steps, len(bad), len(names), ", ".join(bad[:5]), ", ..." if len(bad) > 5 else ""))

    def _step_call(self, eng, dp, inp, gt, lr, adam, final, fold, clip, graph, average=None):
        """One batch: a micro-step of an accumulation group, or (final) the optimizer step - the one that closes the group, or
        with fold=False and clip=None the plain step.  graph=True: per (shape, variant, fold, clipped) the first call runs eagerly
        (it sizes the engine's buffers), the second captures (parallel.StaticBatchStep), later ones replay."""
        def run():   # the eager step
            return eng.train_step(inp, gt, lr=lr, dp=dp, clip_grad_norm=clip, **adam) if final else eng.accumulate_step(inp, gt)

        if not graph or any(eng.opt_amsgrad):   # (amsgrad steps are not captured: parallel.GraphedStep)
            return run()
        variant = "final" if final else "micro"
        with eng.mask_held() as mask:   # one read of the flags for the signature and the step
            sig = (StaticBatchStep.signature(inp, gt), variant, fold, clip is not None)
            if average is not None and final:   # a capture with the average in its AdamW launch is a shape of its own
                sig = sig + ("average",)
            if eng.opt_kind != "adamw" and final:   # (the optimizer launch of another update rule: Engine.set_optimizer)
                sig = sig + (("optimizer", eng.opt_kind),)
            if eng.nonfinite_guard and final:   # (the guarded launches are a capture of their own; micro-steps have none)
                sig = sig + ("guard",)
            if eng.loss_key() is not None:   # (the head launches of another objective: Engine.set_loss; every variant holds them)
                sig = sig + (("loss", eng.loss_key()),)
            if eng.frozen:   # (frozen parameters: the pruned backward and the masked AdamW are captures of their own, per set of flags)
                sig = sig + (mask,)
            if eng.classes.epoch and final:   # (per-tensor step counts: the AdamW launch follows the step classes of the moment)
                sig = sig + (("step classes", eng.classes.epoch),)
            state = self._static_steps.pop(sig, None)
            if state == "seen":
                try:
                    state = StaticBatchStep(eng, None if variant == "micro" else dp, inp, gt, lr, variant=variant, clip_grad_norm=clip,
                                            fold=fold, **adam)
                except RuntimeError as exc:   # a failed capture must not take the run down: this shape stays eager
                    import warnings
                    warnings.warn("hipGraph capture of the %s step failed (%s); continuing with eager launches" % (
                        variant if fold or clip is not None or eng.nonfinite_guard else "training", exc))
                    torch.cuda.synchronize()
                    state = "eager"
            if state is None or state == "eager":   # (None: the first batch of this shape allocates the engine's buffers for it)
                loss = run()
                state = state or "seen"
            else:
                state.seg.clip = clip   # max_norm lives in the hyper table: a new value is no new capture
                loss = state(inp, gt, lr=lr, **adam)
            self._static_steps[sig] = state   # re-inserted last: the dict is the LRU order
            while len(self._static_steps) > self.max_captured_shapes:
                _evict_lru(self._static_steps)
        return loss

    # ------------------------------------------------------------------ validation (no grad, eval-mode BN, no dropout)
    def validate(self, model, dataloader_val, config, graph=True, lane_bucket=16):
        """Mean L1 loss over the validation set in eval mode (phase2_train_net.py:124-177).  graph=True: as in train(), the
        second batch of a shape captures the forward into a hipGraph over static inputs (parallel.StaticEvalStep) and later
        batches of that shape replay it; lane sets are padded to a multiple of `lane_bucket` (padded lanes are masked by
        lane_num: the loss is unchanged)."""
        loss = self._mean_loss(model, dataloader_val, config, graph, lane_bucket, "_static_evals")
        if loss is not None:
            self.val_loss.append(loss)
        return loss

    def validate_average(self, average, dataloader_val, config, graph=True, lane_bucket=16):
        """validate() of a weight average's module (averaging.AveragedMMFN) into val_loss_average; val_loss, bestval and the
        best_* files stay the live model's."""
        loss = self._mean_loss(average.module, dataloader_val, config, graph, lane_bucket, "_static_evals_average")
        if loss is not None:
            self.val_loss_average.append(loss)
        return loss

    def _mean_loss(self, model, dataloader_val, config, graph, lane_bucket, cache):
        """Mean eval-mode L1 loss over the loader (None without batches); `cache`: the attribute holding this model's captures."""
        model.eval()
        eng = model._engine_for()
        if not hasattr(self, cache):
            setattr(self, cache, {})     # input-shape signature -> "seen" | "eager" | StaticEvalStep, in LRU order
        static_evals = getattr(self, cache)
        total = torch.zeros(1, dtype=torch.float32, device=model._layout.device)
        num_batches = 0
        with torch.no_grad():
            for args, gt in D.DevicePrefetcher(dataloader_val, self.device, config, variant=model.variant):
                inp = args if isinstance(args, dict) else model._pack(*args)
                if graph:
                    inp = _bucket_lanes(inp, lane_bucket)
                    sig = StaticBatchStep.signature(inp, gt)
                    state = static_evals.pop(sig, None)
                    if state is None:
                        state = "seen"
                        _, loss = eng.forward(inp, False, gt)
                    else:
                        if state == "seen":
                            try:
                                state = StaticEvalStep(eng, inp, gt)
                            except RuntimeError as exc:
                                import warnings
                                warnings.warn("hipGraph capture of the validation step failed (%s); continuing with eager launches" % exc)
                                torch.cuda.synchronize()
                                state = "eager"
                        loss = eng.forward(inp, False, gt)[1] if state == "eager" else state(inp, gt)
                    static_evals[sig] = state
                    while len(static_evals) > self.max_captured_shapes:
                        _evict_lru(static_evals)
                else:
                    _, loss = eng.forward(inp, False, gt)
                total += loss
                num_batches += 1
        if num_batches:
            return float(total.item()) / num_batches
        return None

    # ------------------------------------------------------------------ checkpoints
    def _log_table(self):
        return {"epoch": self.cur_epoch, "iter": self.cur_iter, "bestval": self.bestval, "bestval_epoch": self.bestval_epoch,
                "train_loss": self.train_loss, "val_loss": self.val_loss}

    def save(self, model, optimizer, logdir=None, average=None):
        """average (averaging.AveragedMMFN): also averaged_model.pth (a plain state_dict of the reference's layout, every save),
        best_averaged_model.pth (when the average's own validation loss improved) and, in recent.log, "average" (mode, decay,
        use_buffers, n_averaged), "val_loss_average" and "bestval_average"."""
        logdir = logdir or self.logdir
        os.makedirs(logdir, exist_ok=True)
        best = bool(self.val_loss) and self.val_loss[-1] <= self.bestval
        if best:
            self.bestval = self.val_loss[-1]
            self.bestval_epoch = self.cur_epoch
        if average is not None:
            best_avg = bool(self.val_loss_average) and self.val_loss_average[-1] <= self.bestval_average
            if best_avg:
                self.bestval_average = self.val_loss_average[-1]
            avg_weights = _plain_state_dict(average.module)
            if best_avg:
                _atomic_save(avg_weights, os.path.join(logdir, "best_averaged_model.pth"))
            _atomic_save(avg_weights, os.path.join(logdir, "averaged_model.pth"))
        weights = _plain_state_dict(model)
        opt_state = optimizer.state_dict()
        # every file goes to a temporary name first and is renamed into place, so no file is ever torn; recent.log is written
        # LAST and records size + a content hash of the files it belongs to: a crash between the renames can leave model.pth one save
        # newer than recent_optim.pth, and resume() then SAYS so (the files stay plain state_dicts the reference can load, so
        # the pairing cannot be stored inside them)
        if best:
            _atomic_save(weights, os.path.join(logdir, "best_model.pth"))
            _atomic_save(opt_state, os.path.join(logdir, "best_optim.pth"))
        _atomic_save(weights, os.path.join(logdir, "model.pth"))
        _atomic_save(opt_state, os.path.join(logdir, "recent_optim.pth"))
        tmp = os.path.join(logdir, "recent.log.tmp")
        table = self._log_table()
        files = ("model.pth", "recent_optim.pth", "best_model.pth", "best_optim.pth")
        if average is not None:
            files += ("averaged_model.pth", "best_averaged_model.pth")
            table["average"] = {"mode": average.mode, "decay": average.decay, "use_buffers": average.use_buffers,
                                "n_averaged": int(average.n_averaged.item())}
            table["val_loss_average"], table["bestval_average"] = self.val_loss_average, self.bestval_average
        if self.skipped_steps is not None:
            table["skipped_steps"] = self.skipped_steps
        table["files"] = {n: _stamp(os.path.join(logdir, n)) for n in files if os.path.isfile(os.path.join(logdir, n))}
        with open(tmp, "w") as f:
            f.write(json.dumps(table))
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, os.path.join(logdir, "recent.log"))
        return best

    def resume(self, model, optimizer, logdir=None, which="best", average=None):
        """Pick a run up from its log directory (phase2_train_net.py:288-302 loads the `best_*` pair).  average
        (averaging.AveragedMMFN): restored from averaged_model.pth and the counter in recent.log - the average of the last save
        whichever pair the model comes from (best_averaged_model.pth is chosen by another loss and is for deployment)."""
        logdir = logdir or self.logdir
        path = os.path.join(logdir, "recent.log")
        if not os.path.isfile(path):
            return False
        with open(path) as f:
            table = json.load(f)
        self.cur_epoch = table["epoch"]
        self.cur_iter = table.get("iter", self.cur_iter)
        self.bestval = table["bestval"]
        self.bestval_epoch = table.get("bestval_epoch", self.cur_epoch)
        self.train_loss = table["train_loss"]
        self.val_loss = table["val_loss"]
        if "skipped_steps" in table:
            self.skipped_steps = table["skipped_steps"]
        names = ("best_model.pth", "best_optim.pth") if which == "best" else ("model.pth", "recent_optim.pth")
        if not all(os.path.isfile(os.path.join(logdir, n)) for n in names):
            # no validation set / no improvement yet: save() never wrote the best_* pair - continue from the recent one
            names = ("model.pth", "recent_optim.pth")
        stale = [n for n in names if n in table.get("files", {}) and not _same_save(table["files"][n], _stamp(os.path.join(logdir, n)))]
        if stale:
            import warnings
            warnings.warn("checkpoint file(s) %s differ in size or content from what recent.log recorded (a save interrupted between "
                          "its renames, or files replaced afterwards): model, optimizer state and counters may come from different "
                          "saves" % ", ".join(stale))
        weights = torch.load(os.path.join(logdir, names[0]), map_location="cpu")
        model.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in weights.items()})
        optimizer.load_state_dict(torch.load(os.path.join(logdir, names[1]), map_location="cpu"))
        if average is not None and "average" in table and os.path.isfile(os.path.join(logdir, "averaged_model.pth")):
            meta = table["average"]
            average.load_state_dict({"module": torch.load(os.path.join(logdir, "averaged_model.pth"), map_location="cpu"),
                                     "n_averaged": meta["n_averaged"], "mode": meta["mode"], "decay": meta["decay"],
                                     "use_buffers": meta["use_buffers"]})
            self.val_loss_average = list(table.get("val_loss_average", []))
            self.bestval_average = table.get("bestval_average", 1e10)
        return True


def _with_last(it):
    """(item, is_last) pairs: one item of look-ahead (the prefetcher has it in flight already)."""
    it = iter(it)
    try:
        prev = next(it)
    except StopIteration:
        return
    for item in it:
        yield prev, False
        prev = item
    yield prev, True


def _bucket_lanes(inp, bucket):
    lane = inp.get("lane")
    if lane is None or bucket <= 1 or lane.shape[1] % bucket == 0:
        return inp
    pad = bucket - lane.shape[1] % bucket
    out = dict(inp)
    out["lane"] = torch.nn.functional.pad(lane, (0, 0, 0, 0, 0, pad))
    return out


def _stamp(path):
    """[size, sha256 of the first and last MiB]: identifies a save by CONTENT, so copying or restoring a log directory without
    its mtimes (cp, rsync without -t, an object-store download) does not look like an interrupted save."""
    import hashlib
    size = os.stat(path).st_size
    h = hashlib.sha256()
    with open(path, "rb") as f:
        h.update(f.read(1 << 20))
        if size > (2 << 20):
            f.seek(size - (1 << 20))
            h.update(f.read(1 << 20))
    return [size, h.hexdigest()]


def _same_save(logged, now):
    """A recent.log written before the stamps became content hashes holds [size, mtime_ns]: compare the size only for those
    (an int second element), so healthy older log directories resume without a spurious "files from different saves" warning."""
    if len(logged) == 2 and isinstance(logged[1], int):
        return logged[0] == now[0]
    return list(logged) == list(now)


def _atomic_save(obj, path):
    tmp = path + ".tmp"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def _hyper_rows(optimizer):
    if hasattr(optimizer, "hyper_rows"):
        return optimizer.hyper_rows()
    return [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in optimizer.param_groups]


_SGD_KEYS = ("lr", "momentum", "dampening", "weight_decay", "nesterov")   # a torch.optim.SGD / FusedSGD group's hyper-parameters


def sync_resume_state(trainer, optimizer, dist, src=0):
    """After rank `src` resumed from disk: every rank takes its epoch / iteration counters, loss history and the
    optimizer hyper-parameters (lr, betas, eps, weight decay and the amsgrad flag per group; an SGD optimizer's lr, momentum,
    dampening, weight decay and nesterov instead).  Without this the ranks would iterate different
    epoch ranges (and deadlock in the gradient all-reduce when rank 0 leaves the loop first), seed their samplers
    differently and step with different learning rates.  Weights / moments / step counter travel separately
    (DataParallel.broadcast_parameters)."""
    payload = [None]
    sgd = bool(optimizer.param_groups) and "momentum" in optimizer.param_groups[0]   # (chosen by what the groups hold)
    if dist.get_rank() == src:
        if sgd:
            groups = [{k: g[k] for k in _SGD_KEYS} for g in optimizer.param_groups]
        else:
            groups = [dict({k: g[k] for k in ("lr", "betas", "eps", "weight_decay")}, amsgrad=bool(g.get("amsgrad", False)))
                      for g in optimizer.param_groups]
        payload[0] = {"table": trainer._log_table(), "groups": groups}
    dist.broadcast_object_list(payload, src=src)
    st = payload[0]
    t = st["table"]
    trainer.cur_epoch, trainer.cur_iter = t["epoch"], t["iter"]
    trainer.bestval, trainer.bestval_epoch = t["bestval"], t["bestval_epoch"]
    trainer.train_loss, trainer.val_loss = list(t["train_loss"]), list(t["val_loss"])
    if len(st["groups"]) != len(optimizer.param_groups):
        raise ValueError("rank %d has %d optimizer groups, rank %d has %d" % (dist.get_rank(), len(optimizer.param_groups), src, len(st["groups"])))
    if any(("momentum" in new) != sgd for new in st["groups"]):
        raise ValueError("rank %d holds %s groups, rank %d sent the other optimizer's" % (dist.get_rank(), "SGD" if sgd else "AdamW", src))
    for g, new in zip(optimizer.param_groups, st["groups"]):
        if sgd:   # (lr, momentum, dampening, weight_decay, nesterov)
            g.update({k: new[k] for k in _SGD_KEYS})
            continue
        g["lr"], g["betas"], g["eps"], g["weight_decay"] = new["lr"], tuple(new["betas"]), new["eps"], new["weight_decay"]
        g["amsgrad"] = new["amsgrad"]
    if hasattr(optimizer, "sync_amsgrad"):   # (FusedAdamW: the flags reach the engine, which allocates max_exp_avg_sq if need be)
        optimizer.sync_amsgrad()


def _plain_state_dict(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def fit(model, optimizer, train_loader, val_loader, config, logdir, epochs, val_every=1, save_every=1, dp=None, rank=0,
        on_log=None, dist=None, accum_steps=1, clip_grad_norm=None, average=None, average_every="step", average_start_epoch=0,
        skip_nonfinite=False, unfreeze_at=None, loss=None, sample_weight=None):
    """The epoch loop of phase2_train_net.py:307-322: train every epoch; rank 0 validates every `val_every`
    epochs and saves every `save_every`.  Data parallel: pass `dp` (a parallel.DataParallel), or just the initialised
    torch.distributed module as `dist` - the transport is then chosen by parallel.connect: the C-ABI RCCL communicator when it
    passes its self-test on every rank (the whole step, gradient all-reduces included, replays as ONE hipGraph per batch shape),
    else torch.distributed (four graphs per step, buckets in between); a capture that fails continues eagerly.
    accum_steps / clip_grad_norm: gradient accumulation and global-norm clipping (Trainer.train; the same accum_steps on
    every rank).
    average (averaging.AveragedMMFN): average_every="step" updates it in every optimizer step (inside the AdamW launch) from epoch
    average_start_epoch on; "epoch" calls its update_parameters() at the end of each such epoch (the SWA schedule).  Rank 0 also
    validates average.module into trainer.val_loss_average and saves averaged_model.pth / best_averaged_model.pth; every rank
    keeps its own copy, in lock step because the parameters are (DataParallel.broadcast_average after a resume).
    skip_nonfinite: Trainer.train's option, every epoch (a skipped step is skipped on every rank: the norm is taken after the
    gradient reduction).
    unfreeze_at = {epoch: [name prefixes]}: gradual unfreezing.  The caller freezes what starts frozen (model.freeze(...)); at the
    start of that epoch every rank calls model.unfreeze(*prefixes) (a prefix that matches nothing raises, here, before the first
    step), and a resumed run applies the entries of the epochs up to the one it resumes into before its first step.  The tensors
    unfrozen late start their AdamW bias correction at step 1, as torch.optim.AdamW's per-parameter counts do (Engine.tensor_steps),
    and the optimizer checkpoint carries those counts.
    loss / sample_weight: Trainer.train's options, every epoch (the objective of the training steps; validation stays mean L1)."""
    if average_every not in ("step", "epoch"):
        raise ValueError("average_every must be 'step' or 'epoch', got %r" % (average_every,))
    if dp is None and dist is not None and dist.get_world_size() > 1:
        from .parallel import connect
        dp, _ = connect(model, dist)
        rank = dist.get_rank()
    schedule = {}
    have = [n for n, _ in model.named_parameters()]
    for at, prefixes in (unfreeze_at or {}).items():
        prefixes = [prefixes] if isinstance(prefixes, str) else list(prefixes)
        for pre in prefixes:
            if not any(n.startswith(pre) for n in have):
                raise ValueError("unfreeze_at[%r]: no parameter name starts with %r" % (at, pre))
        schedule[int(at)] = prefixes
    trainer = Trainer(model._layout.device, logdir)
    if rank == 0:
        trainer.resume(model, optimizer, average=average)
    if dp is not None:
        dp.broadcast_parameters()                       # weights, BN buffers, Adam moments, step counter, RNG
        sync_resume_state(trainer, optimizer, dp.dist)  # epoch / iteration counters, loss history, lr & co
        if average is not None:
            dp.broadcast_average(average)
    for at in sorted(schedule):   # a resumed run: what the epochs before this one unfroze (after sync_resume_state: on every rank)
        if at < trainer.cur_epoch:
            model.unfreeze(*schedule[at])
    for epoch in range(trainer.cur_epoch, epochs):
        if epoch in schedule:
            model.unfreeze(*schedule[epoch])
        sampler = getattr(train_loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        averaging = average is not None and epoch >= average_start_epoch
        trainer.train(model, train_loader, config, optimizer, dp=dp, on_log=on_log if rank == 0 else None, accum_steps=accum_steps,
                      clip_grad_norm=clip_grad_norm, average=average if averaging and average_every == "step" else None,
                      skip_nonfinite=skip_nonfinite, loss=loss, sample_weight=sample_weight)
        if averaging and average_every == "epoch":
            average.update_parameters(model)
        if epoch % val_every == 0 and rank == 0 and val_loader is not None:
            trainer.validate(model, val_loader, config)
            if average is not None:
                trainer.validate_average(average, val_loader, config)
            if epoch % save_every == 0:
                trainer.save(model, optimizer, average=average)
    return trainer
