"""The argument contract of the six optimizer-step entry points (mmfn_adamw_groups_f32, mmfn_adamw_rows_f32, their _ams forms,
mmfn_sgd_groups_f32, mmfn_sgd_rows_f32), which share one launcher in mmfn_amd/csrc/optim.hip: a variant that is not built, a NULL
or misaligned pointer the launch would read, or a count out of range returns MMFN_EINVAL before anything is launched, so every
buffer keeps its bits; n = 0 returns 0 whatever else is passed.  What the launches compute is the subject of test_amsgrad_gpu.py,
test_sgd_gpu.py, test_tensor_steps_gpu.py and test_frozen_params_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1024
EINVAL = -1
COEF, AVG, GUARD, MASK = 1, 2, 4, 8
STATE = {"adamw": ("m", "v"), "adamw_ams": ("m", "v", "vmax"), "sgd": ("buf",)}
SLOTS = {"groups": ("slot_of", "hyper", "n_groups", "steps"),
         "rows": ("slot_of", "hyper", "n_groups", "rows", "n_rows", "steps", "n_classes")}
TAIL = ("variant", "coef", "avg", "n_averaged", "ema_w", "avg_mode", "ok", "stream")
ENTRY_POINTS = {"mmfn_adamw_groups_f32": ("adamw", "groups"), "mmfn_adamw_rows_f32": ("adamw", "rows"),
                "mmfn_adamw_groups_ams_f32": ("adamw_ams", "groups"), "mmfn_adamw_rows_ams_f32": ("adamw_ams", "rows"),
                "mmfn_sgd_groups_f32": ("sgd", "groups"), "mmfn_sgd_rows_f32": ("sgd", "rows")}


class Launch(object):
    """One entry point with a full set of valid arguments; call(name=value, ...) replaces some and returns the C return code."""

    def __init__(self, name):
        from mmfn_amd import _lib, ops
        rule, self.slots = ENTRY_POINTS[name]
        self.fn = getattr(_lib.lib(), name)
        self.order = ("p", "g") + STATE[rule] + ("n",) + SLOTS[self.slots] + TAIL
        self.state = STATE[rule]
        gen = torch.Generator().manual_seed(7)
        self.buffers = {k: torch.randn(N, generator=gen).to(DEV) for k in ("p", "g", "avg") + self.state}
        if "v" in self.buffers:
            self.buffers["v"].square_()
        if "vmax" in self.buffers:
            self.buffers["vmax"].square_()
        hyper = torch.zeros(16, 8)
        hyper[:2] = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 0.0, 0.0]) if rule != "sgd" else \
            torch.tensor([1e-2, 0.9, 0.0, 0.0, 1e-2, 1.0, 0.0, 0.0])
        self.buffers.update(hyper=hyper.to(DEV), slot_of=torch.zeros(N // 4, dtype=torch.uint8, device=DEV),
                            steps=torch.full((4,), 3, dtype=torch.int64, device=DEV), coef=torch.ones(1, device=DEV),
                            n_averaged=torch.full((1,), 2, dtype=torch.int64, device=DEV), ema_w=torch.full((1,), 0.25, device=DEV),
                            ok=torch.ones(1, dtype=torch.int32, device=DEV))
        self.buffers["slot_of"][N // 8:] = 1
        self.rows = torch.tensor([[0, 0], [1, 1]], dtype=torch.int32)   # host memory: (group, class)
        self.args = {k: v.data_ptr() for k, v in self.buffers.items()}
        self.args.update(n=N, n_groups=2, rows=self.rows.data_ptr(), n_rows=2, n_classes=2, variant=0, avg_mode=ops.AVG_EMA,
                         stream=ops.stream())
        torch.cuda.synchronize()
        self.before = {k: v.clone() for k, v in self.buffers.items()}

    def call(self, **replace):
        a = dict(self.args, **replace)
        return self.fn(*[a[k] for k in self.order])

    def untouched(self):
        torch.cuda.synchronize()
        return [k for k, v in self.buffers.items() if not torch.equal(v.view(torch.uint8), self.before[k].view(torch.uint8))]

    @property
    def full(self):
        """The variant that makes every optional pointer mandatory."""
        return COEF | AVG | GUARD | (MASK if self.slots == "groups" else 0)


@pytest.fixture(params=sorted(ENTRY_POINTS))
def launch(request):
    return Launch(request.param)


def test_valid_arguments_launch(launch):
    """(the control: the arguments the other tests start from are accepted, plain and with every variant bit, and the step is taken)"""
    assert launch.call() == 0
    assert launch.call(variant=launch.full) == 0
    assert set(launch.untouched()) == {"p", "avg"} | set(launch.state) - {"vmax"}   # (no amsgrad flag in the hyper rows)


def test_invalid_variants(launch):
    bad = [-1, GUARD, GUARD | AVG] + ([GUARD | MASK, GUARD | AVG | MASK, 16, 16 | COEF] if launch.slots == "groups" else
                                      [MASK, MASK | COEF, MASK | COEF | AVG | GUARD, 16, 1 << 10])
    for variant in bad:
        assert launch.call(variant=variant) == EINVAL, variant
    assert launch.untouched() == []


def test_null_pointers(launch):
    always = ("p", "g") + launch.state + ("hyper", "steps") + (("slot_of", "rows") if launch.slots == "rows" else ())
    for name in always:
        assert launch.call(**{name: None}) == EINVAL, name
    for name in always + ("slot_of", "coef", "avg", "n_averaged", "ema_w", "ok"):
        assert launch.call(variant=launch.full, **{name: None}) == EINVAL, name
    assert launch.untouched() == []


def test_misaligned_step_counter(launch):
    for variant in (0, launch.full):
        assert launch.call(variant=variant, steps=launch.args["steps"] + 4) == EINVAL
    assert launch.untouched() == []


@pytest.mark.parametrize("name", sorted(k for k, v in ENTRY_POINTS.items() if v[1] == "rows"))
def test_rows_out_of_range(name):
    launch = Launch(name)
    assert launch.call(n_rows=0) == EINVAL
    many = torch.zeros(255, 2, dtype=torch.int32)
    assert launch.call(rows=many.data_ptr(), n_rows=255) == EINVAL
    for row in ([2, 0], [0, 2], [-1, 0], [0, -1]):   # group n_groups, class n_classes, and below the tables
        rows = torch.tensor([[0, 0], row], dtype=torch.int32)
        assert launch.call(rows=rows.data_ptr()) == EINVAL, row
    assert launch.untouched() == []


def test_empty_range_needs_no_pointers(launch):
    nothing = {k: None for k in launch.buffers}
    assert launch.call(n=0, rows=None, **nothing) == 0
    assert launch.untouched() == []
