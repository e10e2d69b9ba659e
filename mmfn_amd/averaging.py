"""Weight averages of an MMFN: an exponential moving average (EMA) or stochastic weight averaging (SWA), with the semantics of
torch.optim.swa_utils.AveragedModel (EMA = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay)), SWA = AveragedModel(m)).

AveragedModel deep-copies the module and lerps its standalone parameter tensors; an MMFN's HIP forward reads the flat buffer
(FlatLayout.params) instead, which such a copy leaves frozen.  AveragedMMFN keeps the average IN an MMFN of the same class,
variant and config, so `.module` is validated, checkpointed and deployed like the live model.  Updates:
  * update_parameters(model): torch's API, one launch over the flat buffer (mmfn_weight_average_f32) + the BatchNorm buffers;
  * Engine.attach_average(avg): every optimizer step of the fused path folds the new weights into the average inside the
    AdamW launch (mmfn_adamw_groups_f32 with MMFN_ADAMW_AVG), eager or graph-replayed.
The weight is formed as torch forms it (EMA: fp32(1 - decay) from a Python float; SWA: 1 / (n_averaged + 1) in fp32 on the
device), the first update copies, and both n_averaged and the EMA weight live in device memory (a captured step stays valid).
Frozen parameters (requires_grad = False) are averaged like the others, as AveragedModel does: the masked AdamW launch skips
their step and their moments but still loads them and updates the average (MMFN_ADAMW_MASK with MMFN_ADAMW_AVG).
"""
import copy

import torch

from . import ops

MODES = {"ema": ops.AVG_EMA, "swa": ops.AVG_SWA}


class AveragedMMFN(object):
    """mode "ema" (decay) or "swa" (equal average).  use_buffers=False (torch's default): every update copies the live model's
    BatchNorm running statistics and counters; True: the fp32 running statistics are averaged with the same weight and the int64
    counters copied (torch would lerp-truncate the counters)."""

    def __init__(self, model, mode="ema", decay=0.999, use_buffers=False):
        if mode not in MODES:
            raise ValueError("mode must be 'ema' or 'swa', got %r" % (mode,))
        L = model._layout
        if L.device is None or L.device.type != "cuda":
            raise ops._lib.MMFNLibraryError("AveragedMMFN needs an MMFN on a GPU device (got %s)" % L.device)
        self.mode, self.use_buffers = mode, bool(use_buffers)
        self.module = type(model)(copy.deepcopy(model.config), L.device, variant=model.variant)
        self.module.train(model.training)
        A = self.module._layout
        if A.total != L.total or A.tail != L.tail or A.offsets != L.offsets:
            raise ValueError("the averaged copy's flat layout differs from the model's")
        if A.buffers_flat.numel() % 4:
            raise ValueError("the BatchNorm buffer holds %d floats, the averaging kernel takes multiples of 4" % A.buffers_flat.numel())
        A.params.copy_(L.params)        # (the first update copies again; until then the average is the model at construction)
        A.buffers_flat.copy_(L.buffers_flat)
        A.counters_flat.copy_(L.counters_flat)
        dev = L.device
        self.n_averaged = torch.zeros((), dtype=torch.int64, device=dev)   # as AveragedModel's buffer
        self.ema_weight = torch.zeros(1, dtype=torch.float32, device=dev)  # fp32(1 - decay), read by the EMA kernels
        self.set_decay(decay)
        self.module.weights_changed()

    @property
    def mode_code(self):
        return MODES[self.mode]

    def set_decay(self, decay):
        """The EMA decay.  The kernels read the weight from device memory: a captured step picks the new value up on its next
        replay.  w = 1 - decay is formed in double on the host and rounded to fp32, as torch's _foreach_lerp_ receives it."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_decay() inside a hipGraph capture; call it before or between replays")
        self.decay = float(decay)
        self.ema_weight.fill_(1.0 - self.decay)

    def check_model(self, model):
        L, A = model._layout, self.module._layout
        if L.offsets is not A.offsets and (L.total != A.total or L.offsets != A.offsets):
            raise ValueError("model and average have different flat layouts (another variant or config?)")

    def update_buffers(self, model, ok=None):
        """BatchNorm running statistics: averaged (use_buffers) or copied; the int64 counters copied.  ok: the non-finite guard's
        device flag (Engine.final_adam): nothing changes when it is 0."""
        L, A = model._layout, self.module._layout
        if self.use_buffers:
            ops.weight_average(A.buffers_flat, L.buffers_flat, self.n_averaged, self.ema_weight, self.mode_code, ok=ok)
        elif ok is None:
            A.buffers_flat.copy_(L.buffers_flat)
        else:
            ops.copy_if(A.buffers_flat, L.buffers_flat, ok, when=True)
        if ok is None:
            A.counters_flat.copy_(L.counters_flat)
        else:
            ops.copy_if(A.counters_flat, L.counters_flat, ok, when=True)

    def update_parameters(self, model):
        """AveragedModel.update_parameters: average every parameter of `model` into the copy (the never-trained tail included:
        a lerp of an unchanged value returns the value), then the buffers, then n_averaged += 1.  One launch over the flat
        buffer, one over the BatchNorm statistics, no host sync."""
        self.check_model(model)
        L, A = model._layout, self.module._layout
        ops.weight_average(A.params, L.params, self.n_averaged, self.ema_weight, self.mode_code)
        self.update_buffers(model)
        ops.step_advance(self.n_averaged)
        self.module.weights_changed()

    def copy_tail(self, model):
        """The never-trained tail [tail, total) of the flat buffer (vec / rad: raster-map stem + layer1), which the AdamW launch
        does not cover: copied when the average is attached (Engine.attach_average)."""
        L, A = model._layout, self.module._layout
        if A.tail < A.total:
            A.params[A.tail:].copy_(L.params[L.tail:])

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        return {"module": {k: v.detach().cpu().clone() for k, v in self.module.state_dict().items()},
                "n_averaged": int(self.n_averaged.item()), "mode": self.mode, "decay": self.decay, "use_buffers": self.use_buffers}

    def load_state_dict(self, state):
        if state["mode"] != self.mode:
            raise ValueError("checkpoint holds a %s average, this one is %s" % (state["mode"], self.mode))
        self.module.load_state_dict(state["module"], strict=True)
        self.n_averaged.fill_(int(state["n_averaged"]))
        self.use_buffers = bool(state.get("use_buffers", self.use_buffers))
        self.set_decay(state["decay"])
