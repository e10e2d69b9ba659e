"""AdamW over the model's flat parameter buffer, with torch.optim.AdamW's checkpoint format.

The reference trains with `optim.AdamW(model.parameters(), lr=args.lr)` (run_steps/phase2_train_net.py:256)
and saves `optimizer.state_dict()` next to the weights (`best_optim.pth`, `recent_optim.pth`, :209,216).
FusedAdamW drives mmfn_adamw_groups_f32 (one launch over all 104.8 M trained parameters, csrc/optim.hip) and reads /
writes that same state-dict layout: parameter ids in group order (one group: `model.parameters()` order), per-id
`step` (every tensor's own count: a tensor unfrozen late is behind the others, Engine.tensor_steps), `exp_avg`,
`exp_avg_sq` in checkpoint shapes (OIHW for convolutions), and no entry for the
parameters that never receive a gradient (vec/rad: the raster-map stem + layer1) -
exactly what torch's optimizer holds after a reference run.

Parameter groups: the reference also defines (and never uses) a decay / no-decay split in
`GPT.configure_optimizers` (model_vec.py:179-209).  `configure_optimizers(model)` below applies that rule to the whole
network; `FusedAdamW(model, param_groups=...)` takes such torch-style groups, each with its own lr / betas / eps /
weight_decay.  All hyper-parameters live in a small device table the kernel reads (Engine.set_hyper), so changing the
learning rate between steps costs one 512-byte copy and never re-captures a hipGraph.

amsgrad: `FusedAdamW(model, amsgrad=True)`, or "amsgrad" in a group dict, as in torch.optim.AdamW.  The running maximum
`max_exp_avg_sq` is a fifth flat buffer (FlatLayout.max_exp_avg_sq, allocated only when some group asks for it), updated inside
the same AdamW launch (mmfn_adamw_groups_ams_f32 / mmfn_adamw_rows_ams_f32); the state dict carries it in checkpoint shape.

FusedSGD is torch.optim.SGD (momentum, dampening, nesterov, coupled weight decay) on the same machinery - groups, hyper table,
frozen masks, per-tensor counts, clipping, the guard, the average, captured steps - through mmfn_sgd_groups_f32 /
mmfn_sgd_rows_f32, with torch.optim.SGD's checkpoint format.  The engine runs one update rule at a time (Engine.set_optimizer):
each optimizer object claims its kind where it hands over its rows, so two optimizers on one model never step through each
other's kernel.
"""
import torch
import torch.nn as nn

from . import params as P

_HYPER = ("lr", "betas", "eps", "weight_decay")


def configure_optimizers(model, weight_decay=0.01):
    """The reference's decay / no-decay rule (model_vec.py:179-209) over the whole model: weights of Linear / Conv2d
    modules (and the GRU cell / GAT matrices, which are plain weight matrices) decay; every bias, every LayerNorm /
    BatchNorm weight and the GPT position embeddings do not.  Returns torch-style param groups, names sorted as the
    reference sorts them."""
    decay, no_decay = set(), set()
    for mn, m in model.named_modules():
        for pn, p in m.named_parameters(recurse=False):
            fpn = "%s.%s" % (mn, pn) if mn else pn
            if pn.endswith("bias") or pn.startswith("bias"):                     # Linear/LN/BN biases, GRUCell bias_ih / bias_hh
                no_decay.add(fpn)
            elif isinstance(m, (nn.LayerNorm, nn.BatchNorm2d)) or pn == "pos_emb":
                no_decay.add(fpn)
            else:
                decay.add(fpn)
    named = dict(model.named_parameters())
    assert decay | no_decay == set(named) and not decay & no_decay
    return [{"params": [named[n] for n in sorted(decay)], "weight_decay": weight_decay},
            {"params": [named[n] for n in sorted(no_decay)], "weight_decay": 0.0}]


class _FusedOptimizer(object):
    """What FusedAdamW and FusedSGD share: torch-style parameter groups over the flat buffer, the per-tensor step counts, the
    step itself.  A subclass names its update rule (KIND, Engine.set_optimizer) and hands over its rows (hyper_rows)."""
    KIND = None

    def _build_groups(self, model, param_groups, normalise):
        """param_groups (None: one group of every parameter) completed from self.defaults, each passed through normalise()."""
        self.model = model
        if param_groups is None:
            param_groups = [{"params": list(model.parameters())}]
        self.param_groups = []
        for g in param_groups:
            full = dict(self.defaults)
            full.update({k: v for k, v in g.items() if k != "params"})
            normalise(full)
            full["params"] = list(g["params"])
            self.param_groups.append(full)
        by_id = {id(p): n for n, p in model.named_parameters()}
        self._group_names = []
        seen = set()
        for g in self.param_groups:
            names = []
            for p in g["params"]:
                n = by_id.get(id(p))
                if n is None:
                    raise ValueError("param_groups holds a tensor that is not a parameter of the model")
                if n in seen:
                    raise ValueError("parameter %s appears in more than one group" % n)
                seen.add(n)
                names.append(n)
            self._group_names.append(names)
        # parameters in no group: allowed while they are frozen - optim.AdamW(filter(lambda p: p.requires_grad, ...)) - and
        # checked again at every step (a parameter unfrozen later has no hyper-parameters to step with)
        self._ungrouped = {n: p for n, p in model.named_parameters() if n not in seen}
        self._check_ungrouped()
        if len(self.param_groups) > 16:
            raise ValueError("at most 16 parameter groups")
        self._install_groups()

    def _check_ungrouped(self):
        missing = [n for n, p in self._ungrouped.items() if p.requires_grad]
        if missing:
            raise ValueError("param_groups must cover every parameter of the model (missing e.g. %s)" % sorted(missing)[:3])

    def group_table(self):
        """The effective group table of the AdamW launch (params.FlatLayout.group_table): the group ids with 255 over the float4s
        of the frozen parameters.  Built on the host; the engine builds the same on the device when something is frozen."""
        L = self.model._layout
        gid = torch.zeros(L.total // 4, dtype=torch.uint8)
        for gi, names in enumerate(self._group_names):
            for n in names:
                b, e = L.span(n)
                gid[b // 4:e // 4] = gi
        return L.group_table(L.frozen_names(), gid)

    def _install_groups(self):
        """One group id per float4 of the flat buffer (tensors are 16-byte aligned in it), handed to the engine."""
        L = self.model._layout
        self._group_of = None
        if len(self.param_groups) > 1:
            gid = torch.zeros(L.total // 4, dtype=torch.uint8)
            for gi, names in enumerate(self._group_names):
                for n in names:
                    off, cnt = L.offsets[n]
                    gid[off // 4:(off + cnt + 3) // 4] = gi
            self._group_of = gid.to(L.device)
        if L.device.type == "cuda":
            self.model._engine_for().set_param_groups(self._group_of)
        self._claim()

    def zero_grad(self, set_to_none=True):
        for p in self.model.parameters():
            p.grad = None  # the flat gradient buffer is overwritten, never accumulated, by every backward

    def step(self, grad_scale=1.0):
        rows = self.hyper_rows()   # (first: a parameter unfrozen outside every group raises before anything is launched)
        self.model._engine_for().optimizer_step(grad_scale=grad_scale, groups=rows)

    def _engine(self):
        """The engine of a module on a GPU; None for a module built on the CPU (its counts then live in the layout alone)."""
        return self.model._engine_for() if self.model._layout.device.type == "cuda" else None

    def tensor_steps(self):
        """{name: step count} of every trained tensor: torch's state[p]["step"] (Engine.tensor_steps)."""
        L, eng = self.model._layout, self._engine()
        steps = eng.tensor_steps().tolist() if eng is not None else L.step_classes.host_steps()
        return dict(zip(L.step_classes.names, steps))

    def _views(self):
        """(name, view, group index) in torch's parameter-id order, group by group; view(flat) is the tensor's window of a flat
        buffer in checkpoint shape (OIHW for convolutions)."""
        L = self.model._layout
        named = dict(self.model.named_parameters())
        out = []
        for gi, names in enumerate(self._group_names):
            for name in names:
                off, n = L.offsets[name]
                p = named[name]
                if P._is_conv_weight(p):
                    o, i, kh, kw = p.shape
                    view = lambda flat, off=off, n=n, o=o, i=i, kh=kh, kw=kw: flat[off:off + n].view(o, kh, kw, i).permute(0, 3, 1, 2)
                else:
                    view = lambda flat, off=off, n=n, shp=p.shape: flat[off:off + n].view(shp)
                out.append((name, view, gi))
        return out

    def _set_steps(self, steps, absent):
        """Per-tensor counts {name: count} of a loaded state into the engine (or, for a module on the CPU, the layout)."""
        L, eng = self.model._layout, self._engine()
        vec = [steps.get(n, 0) for n in L.step_classes.names]
        top = max(vec) if vec else 0
        if eng is None:
            L.step_classes.set_steps(vec, top)
            return
        eng.never_stepped = frozenset(absent) if steps else None
        eng.set_tensor_steps(vec, step_count=top)   # (step_count: the count of optimizer steps, the largest per-tensor one)


class FusedAdamW(_FusedOptimizer):
    KIND = "adamw"

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, param_groups=None, amsgrad=False):
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad))

        def normalise(full):
            full["betas"] = tuple(full["betas"])
            full["amsgrad"] = bool(full["amsgrad"])

        self._build_groups(model, param_groups, normalise)

    def _claim(self):
        self.sync_amsgrad()

    def amsgrad_flags(self):
        """(amsgrad,) per group - what Engine.set_amsgrad takes, beside hyper_rows()."""
        return tuple(bool(g.get("amsgrad", False)) for g in self.param_groups)

    def sync_amsgrad(self):
        """The groups' amsgrad flags as they stand (torch lets a caller assign param_groups[i]["amsgrad"]) reach the engine, and
        max_exp_avg_sq exists once a group asks for it: at construction, in front of every step and after load_state_dict."""
        flags = self.amsgrad_flags()
        L = self.model._layout
        if L.device.type == "cuda":
            eng = self.model._engine_for()
            eng.set_optimizer(self.KIND)   # (this optimizer's rows step through its own launch: a FusedSGD may have held the kind)
            eng.set_amsgrad(flags)
        elif any(flags):
            L.ensure_max_exp_avg_sq()

    # ------------------------------------------------------------------ stepping
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def hyper_rows(self):
        """[(lr, beta1, beta2, eps, weight_decay)] per group - what Engine.optimizer_step(groups=...) takes."""
        self._check_ungrouped()
        self.sync_amsgrad()   # (the flags travel beside the rows: the engine writes them into the same device table)
        return [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in self.param_groups]

    # ------------------------------------------------------------------ torch.optim.AdamW-format state
    def _moment_views(self):
        """(name, exp_avg view, exp_avg_sq view, max_exp_avg_sq view or None, group index) in torch's parameter-id order: group
        by group."""
        L = self.model._layout
        return [(name, view(L.exp_avg), view(L.exp_avg_sq), None if L.max_exp_avg_sq is None else view(L.max_exp_avg_sq), gi)
                for name, view, gi in self._views()]

    def state_dict(self):
        L = self.model._layout
        steps = self.tensor_steps()
        state = {}
        # a tensor that never took a step (frozen at every optimizer step so far, or no step yet): torch holds no state for it either
        self.sync_amsgrad()
        for idx, (name, m, v, vmax, gi) in enumerate(self._moment_views()):
            if name in L.unused or steps[name] == 0:
                continue
            state[idx] = {"step": torch.tensor(float(steps[name])), "exp_avg": m.clone().contiguous(),
                          "exp_avg_sq": v.clone().contiguous()}
            if self.param_groups[gi]["amsgrad"]:   # torch keeps max_exp_avg_sq for the parameters of an amsgrad group only
                state[idx]["max_exp_avg_sq"] = vmax.clone().contiguous()
        groups = []
        start = 0
        for g, names in zip(self.param_groups, self._group_names):
            d = {k: v for k, v in g.items() if k != "params"}
            d.update(maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
            d["params"] = list(range(start, start + len(names)))
            start += len(names)
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """Per-parameter `step` values may differ (a torch run that unfroze tensors late): every tensor keeps its own count.  An
        id without an entry has count 0 and zero moments; a trained tensor outside this optimizer's groups likewise.  amsgrad comes
        from the checkpoint's groups, as torch takes its groups from the checkpoint: max_exp_avg_sq is filled from the entries of
        the amsgrad groups (zero elsewhere); an entry of such a group without it is a ValueError."""
        L = self.model._layout
        eng = self._engine()
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("optimizer state has %d parameter groups, this optimizer %d" % (len(sd["param_groups"]), len(self.param_groups)))
        get = lambda idx: sd["state"].get(idx, sd["state"].get(str(idx)))
        start = 0
        for names, theirs in zip(self._group_names, sd["param_groups"]):   # (checked before anything is changed)
            if len(theirs["params"]) != len(names):
                raise ValueError("optimizer state holds %d parameters in a group, the model has %d" % (len(theirs["params"]), len(names)))
            if theirs.get("amsgrad", False):
                for idx in range(start, start + len(names)):
                    if get(idx) is not None and "max_exp_avg_sq" not in get(idx):
                        raise ValueError("optimizer state: parameter %d (%s) belongs to a group with amsgrad=True but its entry holds "
                                         "no max_exp_avg_sq" % (idx, names[idx - start]))
            start += len(names)
        for mine, theirs in zip(self.param_groups, sd["param_groups"]):
            for k in _HYPER:
                if k in theirs:
                    mine[k] = tuple(theirs[k]) if k == "betas" else theirs[k]
            mine["amsgrad"] = bool(theirs.get("amsgrad", False))
        self.sync_amsgrad()
        steps = {}
        absent = set()
        L.exp_avg.zero_()
        L.exp_avg_sq.zero_()
        if L.max_exp_avg_sq is not None:
            L.max_exp_avg_sq.zero_()
        for idx, (name, m, v, vmax, gi) in enumerate(self._moment_views()):
            st = get(idx)
            if st is None:
                absent.add(name)
                continue
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            if self.param_groups[gi]["amsgrad"]:
                vmax.copy_(st["max_exp_avg_sq"])
            steps[name] = int(float(st["step"]))
        self._set_steps(steps, absent)


_SGD_HYPER = ("lr", "momentum", "dampening", "weight_decay", "nesterov")


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD (momentum, dampening, nesterov, coupled weight decay) on the fused, captured training step:
    mmfn_sgd_groups_f32 / mmfn_sgd_rows_f32 over the same flat buffers, hyper table, groups, frozen masks, step classes, clip
    coefficient, guard flag and in-launch average as FusedAdamW.  The momentum buffer is the layout's exp_avg.  torch's
    `momentum_buffer is None` is "the tensor's step count is 0": the step that takes a tensor's count to 1 copies d into the
    buffer without dampening.  (torch keeps no buffer while a group's momentum is 0; here the tensor's count still advances, so a
    group whose momentum is switched on later blends into a zero buffer instead of copying - the two differ only with dampening.)

    Handing over from AdamW (the SWA phase): exp_avg then holds Adam's first moment and the counts are non-zero, so constructing
    a FusedSGD over tensors that have stepped raises unless reset_state=True, which zeroes exp_avg, exp_avg_sq (and
    max_exp_avg_sq), every per-tensor count and step_count.  An attached average is not touched.  `maximize` is not supported."""
    KIND = "sgd"

    def __init__(self, model, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, param_groups=None, reset_state=False):
        self.defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov))
        self._validate(self.defaults)
        L = model._layout
        eng = model._engine_for() if L.device.type == "cuda" else None
        stepped = any((eng.tensor_steps().tolist() if eng is not None else L.step_classes.host_steps()))
        if stepped and not reset_state and not (eng is not None and eng.opt_kind == self.KIND):
            raise RuntimeError("the model's tensors have taken optimizer steps: exp_avg holds another optimizer's state and a "
                               "non-zero count skips SGD's first-step rule; pass reset_state=True to zero the optimizer state "
                               "and every step count (or load_state_dict() a torch.optim.SGD state afterwards)")

        def normalise(full):
            full["nesterov"] = bool(full["nesterov"])
            self._validate(full)

        if reset_state and eng is not None and eng.accum_pending:
            raise RuntimeError("reset_state=True while %d accumulated micro-step(s) are pending" % eng.accum_pending)
        self._build_groups(model, param_groups, normalise)
        if reset_state:   # (after the groups were checked: a refused construction changes nothing)
            L.exp_avg.zero_()
            L.exp_avg_sq.zero_()
            if L.max_exp_avg_sq is not None:
                L.max_exp_avg_sq.zero_()
            self._set_steps({}, ())

    @staticmethod
    def _validate(g):
        """torch.optim.SGD's checks and messages."""
        if "maximize" in g and g["maximize"]:
            raise ValueError("maximize=True is not supported by FusedSGD")
        if g["lr"] < 0.0:
            raise ValueError("Invalid learning rate: %s" % (g["lr"],))
        if g["momentum"] < 0.0:
            raise ValueError("Invalid momentum value: %s" % (g["momentum"],))
        if g["weight_decay"] < 0.0:
            raise ValueError("Invalid weight_decay value: %s" % (g["weight_decay"],))
        if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def _claim(self):
        """This optimizer's rows step through the SGD launch: the kind (and with it the end of any amsgrad flags a FusedAdamW
        left) reaches the engine at construction, in front of every step and after load_state_dict."""
        if self.model._layout.device.type == "cuda":
            eng = self.model._engine_for()
            if eng.opt_kind != self.KIND:
                eng.set_amsgrad(())
                eng.set_optimizer(self.KIND)

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    def hyper_rows(self):
        """[(lr, momentum, dampening, nesterov, weight_decay)] per group - what Engine.optimizer_step(groups=...) takes."""
        self._check_ungrouped()
        for g in self.param_groups:   # (torch lets a caller assign param_groups[i][...]: checked where they are read)
            self._validate(g)
        self._claim()
        return [(g["lr"], g["momentum"], g["dampening"], 1.0 if g["nesterov"] else 0.0, g["weight_decay"]) for g in self.param_groups]

    # ------------------------------------------------------------------ torch.optim.SGD-format state
    def state_dict(self):
        """Exactly what torch.optim.SGD holds: state[idx] = {"momentum_buffer"} in checkpoint shape for the tensors that have
        stepped in a group with momentum; no entry otherwise."""
        L = self.model._layout
        steps = self.tensor_steps()
        state = {}
        for idx, (name, view, gi) in enumerate(self._views()):
            if name in L.unused or steps[name] == 0 or self.param_groups[gi]["momentum"] == 0:
                continue
            state[idx] = {"momentum_buffer": view(L.exp_avg).clone().contiguous()}
        groups = []
        start = 0
        for g, names in zip(self.param_groups, self._group_names):
            d = {k: g[k] for k in _SGD_HYPER}
            d.update(maximize=False, foreach=None, differentiable=False, fused=None)
            d["params"] = list(range(start, start + len(names)))
            start += len(names)
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """torch.optim.SGD's state dict.  torch stores no step for SGD and only "has stepped" matters: an entry sets the tensor's
        count to 1, a missing entry (or a None buffer) count 0 and a zero buffer.  Group hyper-parameters come from the checkpoint."""
        L = self.model._layout
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("optimizer state has %d parameter groups, this optimizer %d" % (len(sd["param_groups"]), len(self.param_groups)))
        get = lambda idx: sd["state"].get(idx, sd["state"].get(str(idx)))
        for names, theirs in zip(self._group_names, sd["param_groups"]):   # (checked before anything is changed)
            if len(theirs["params"]) != len(names):
                raise ValueError("optimizer state holds %d parameters in a group, the model has %d" % (len(theirs["params"]), len(names)))
            if theirs.get("maximize", False):
                raise ValueError("optimizer state: a group with maximize=True, which FusedSGD does not support")
            if "momentum" not in theirs:
                raise ValueError("optimizer state: the groups hold no momentum - not a torch.optim.SGD state")
            self._validate(dict({k: theirs.get(k, self.defaults[k]) for k in _SGD_HYPER}))
        for mine, theirs in zip(self.param_groups, sd["param_groups"]):
            for k in _SGD_HYPER:
                if k in theirs:
                    mine[k] = bool(theirs[k]) if k == "nesterov" else theirs[k]
        self._claim()
        steps, absent = {}, set()
        L.exp_avg.zero_()
        L.exp_avg_sq.zero_()
        for idx, (name, view, gi) in enumerate(self._views()):
            st = get(idx)
            if st is None or st.get("momentum_buffer") is None:
                absent.add(name)
                continue
            view(L.exp_avg).copy_(st["momentum_buffer"])
            steps[name] = 1
        self._set_steps(steps, absent)
