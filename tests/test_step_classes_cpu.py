"""Per-tensor AdamW step counts, host side (params.StepClasses): the partition of the trained tensors into step classes under a
sequence of requires_grad flag sets and step launches, the row table of the AdamW launch, the grouping of loaded counts by
value, the 254-row limit, and the optimizer's checkpoint with differing counts on a module built on the CPU."""
import pytest
import torch

from mmfn_amd.config import GlobalConfig


@pytest.fixture(scope="module")
def vec_model():
    from mmfn_amd.model import MMFN
    torch.manual_seed(0)
    return MMFN(GlobalConfig(), "cpu")


def _fresh(model):
    from mmfn_amd.params import StepClasses
    L = model._layout
    return StepClasses([n for n in L.offsets if n not in L.unused])


TRUNK = "encoder.lidar_encoder."
ONE = "join.0.bias"


def test_one_class_until_flags_diverge_then_classes_split_and_follow_the_launches(vec_model):
    L = vec_model._layout
    C = _fresh(vec_model)
    names = C.names
    assert names == [n for n in L.offsets if n not in L.unused] and len(names) > 300
    assert not any(n in L.unused for n in names)
    # nothing ever frozen: one class, the shared counter serves it, and launches change nothing
    assert C.install(frozenset()) == [] and C.epoch == 0
    for _ in range(3):
        C.launched()
    assert C.n_classes == 1 and C.uniform() and C.synced == [True] and C.active == [True] and set(C.cls) == {0}
    # a trunk and one bias freeze: class 0 splits, the frozen tensors form class 1 with a copy of the count
    trunk = frozenset(n for n in names if n.startswith(TRUNK)) | {ONE}
    assert C.install(trunk) == [(1, 0)] and C.epoch == 1
    assert C.members()[1] == [n for n in names if n in trunk] and C.active == [True, False]
    assert C.uniform()                      # the class that steps still carries the shared count
    assert C.install(trunk) == [] and C.epoch == 1          # the same flags again: nothing happens
    C.launched()
    C.launched()
    assert C.synced == [True, False] and C.uniform()        # the frozen class fell behind; nobody who steps did
    # the bias alone comes back: it stays in class 1 with the trunk (same launches so far), class 1 splits
    assert C.install(trunk - {ONE}) == [(2, 1)]
    assert C.members()[1] == [ONE] and C.members()[2] == [n for n in names if n.startswith(TRUNK)]
    assert C.active == [True, True, False] and C.synced == [True, False, False]
    assert not C.uniform()                  # a tensor that steps has a count of its own: the launch with step classes
    e = C.epoch
    C.launched()
    # everything trains again: no split, three classes stay (equal counts are not merged)
    assert C.install(frozenset()) == [] and C.n_classes == 3 and C.active == [True] * 3 and C.epoch == e + 1
    assert not C.uniform()
    # freezing across classes splits every class that is cut
    cut = frozenset([names[0], ONE] + [n for n in names if n.startswith(TRUNK)][:2])
    splits = C.install(cut)
    assert sorted(src for _, src in splits) == [0, 2]       # class 1 (the bias alone) freezes as a whole: no split
    assert C.n_classes == 5 and C.active[1] is False
    for c, members in enumerate(C.members()):
        assert members and len({n in cut for n in members}) == 1, c     # a class never mixes frozen and trainable tensors
        assert C.active[c] == (members[0] not in cut)
    assert sorted(n for m in C.members() for n in m) == sorted(names)


def test_row_table_has_255_over_frozen_spans_and_one_row_per_group_and_class(vec_model):
    from mmfn_amd.optim import FusedAdamW, configure_optimizers
    L = vec_model._layout
    C = _fresh(vec_model)
    names = C.names
    trunk = frozenset(n for n in names if n.startswith(TRUNK)) | {ONE}
    C.install(trunk)
    C.launched()
    frozen = frozenset(["encoder.transformer2.pos_emb", "output.bias"])     # (output.bias holds 2 floats: its span ends on padding)
    C.install(frozen)
    assert C.n_classes == 3 and not C.uniform()
    # one optimizer group: rows = the classes that step, in layout order of their first tensor
    tab, rows = C.row_table(L, frozen)
    assert tab.dtype == torch.uint8 and tab.numel() == L.total // 4 and rows.dtype == torch.int32 and rows.shape == (2, 2)
    assert rows[:, 0].tolist() == [0, 0] and sorted(rows[:, 1].tolist()) == [0, 1]
    # two groups (decay / no decay): distinct (group, class) pairs, each once
    opt = FusedAdamW(vec_model, param_groups=configure_optimizers(vec_model))
    gid = opt.group_table()
    tab, rows = C.row_table(L, frozen, gid)
    pairs = [tuple(r) for r in rows.tolist()]
    assert len(set(pairs)) == len(pairs) == 4 and set(pairs) == {(g, c) for g in (0, 1) for c in (0, 1)}
    cls = dict(zip(names, C.cls))
    covered = torch.zeros(L.total // 4, dtype=torch.bool)
    for n in names:
        b, e = L.span(n)
        assert e % 4 == 0 and b % 4 == 0 and e - b >= L.offsets[n][1]       # the span ends on the float4 the next tensor starts at
        got = tab[b // 4:e // 4]
        covered[b // 4:e // 4] = True
        if n in frozen:
            assert bool((got == 255).all()), n
        else:
            assert len(set(got.tolist())) == 1 and pairs[int(got[0])] == (int(gid[b // 4]), cls[n]), n
    assert L.offsets["output.bias"][1] % 4 != 0                            # (the padded float4 belongs to the frozen span)
    assert bool((tab[~covered] == 255).all())                              # never-trained tensors: no row
    assert int((tab == 255).sum()) == int((~covered).sum()) + sum((L.offsets[n][1] + 3) // 4 for n in frozen)


def test_set_steps_groups_the_tensors_by_distinct_value(vec_model):
    C = _fresh(vec_model)
    names = C.names
    steps = [7] * len(names)
    for i, n in enumerate(names):
        if n.startswith(TRUNK):
            steps[i] = 3
    steps[names.index(ONE)] = 0
    C.set_steps(steps)
    assert C.n_classes == 3 and C.values == [7, 3, 0] and C.synced == [True, False, False] and not C.uniform()
    assert C.host_steps() == steps
    assert C.members()[2] == [ONE] and C.members()[1] == [n for n in names if n.startswith(TRUNK)]
    # one common value: one class again, and the shared counter serves it
    C.set_steps([5] * len(names))
    assert C.n_classes == 1 and C.uniform() and C.host_steps() == [5] * len(names)
    # ... unless the engine's step count is another one
    C.set_steps([5] * len(names), step_count=9)
    assert C.n_classes == 1 and not C.uniform()
    # frozen tensors of a loaded state split off as usual, and a class that does not step does not count against uniform()
    C.set_steps(steps)
    C.install(frozenset(n for n in names if n.startswith(TRUNK)) | {ONE})
    assert C.n_classes == 3 and C.active == [True, False, False] and C.uniform()
    C.launched()
    with pytest.raises(RuntimeError, match="device"):
        C.host_steps()
    with pytest.raises(ValueError):
        C.set_steps([1, 2, 3])
    with pytest.raises(ValueError):
        C.set_steps([-1] * len(names))


def test_more_than_254_rows_is_refused_by_count(vec_model):
    L = vec_model._layout
    C = _fresh(vec_model)
    n = len(C.names)
    assert n > 255
    C.set_steps(list(range(1, 255)) + [254] * (n - 254))          # 254 distinct counts: the limit itself
    tab, rows = C.row_table(L, frozenset())
    assert rows.shape == (254, 2) and int(tab[:L.tail // 4].max()) == 253
    C.set_steps(list(range(1, 256)) + [255] * (n - 255))          # 255
    with pytest.raises(ValueError, match="255"):
        C.row_table(L, frozenset())
    C.install(frozenset(C.names[:1]))                             # one of them frozen: 254 rows step, accepted
    assert C.row_table(L, frozenset(C.names[:1]))[1].shape == (254, 2)


def test_checkpoint_with_per_tensor_counts_on_a_cpu_module():
    from mmfn_amd.model import MMFN
    from mmfn_amd.optim import FusedAdamW
    torch.manual_seed(1)
    model = MMFN(GlobalConfig(), "cpu")
    L = model._layout
    opt = FusedAdamW(model, lr=1e-3)
    assert opt.state_dict()["state"] == {}                        # no step yet: no entry, as torch
    all_names = [n for n, _ in model.named_parameters()]
    # a torch-style state with three different counts: absent, 2 and 4
    want = {}
    state = {}
    gen = torch.Generator().manual_seed(3)
    for idx, (n, p) in enumerate(model.named_parameters()):
        if n in L.unused or n == ONE:
            continue
        want[n] = 2 if n.startswith(TRUNK) else 4
        state[idx] = {"step": torch.tensor(float(want[n])), "exp_avg": torch.randn(p.shape, generator=gen),
                      "exp_avg_sq": torch.rand(p.shape, generator=gen)}
    sd = opt.state_dict()
    sd["state"] = state
    opt.load_state_dict(sd)                                       # (differing counts used to raise)
    steps = opt.tensor_steps()
    assert steps[ONE] == 0 and all(steps[n] == want[n] for n in want) and set(steps) == set(want) | {ONE}
    out = opt.state_dict()
    assert sorted(out["state"]) == sorted(state)
    for idx, st in state.items():
        got = out["state"][idx]
        assert float(got["step"]) == float(st["step"]), all_names[idx]
        assert torch.equal(got["exp_avg"], st["exp_avg"]) and torch.equal(got["exp_avg_sq"], st["exp_avg_sq"]), all_names[idx]
    # the id layout is torch's: the state loads into torch.optim.AdamW over the same parameters
    ref = torch.optim.AdamW(model.parameters(), lr=1e-3)
    ref.load_state_dict(out)
    params = list(model.parameters())
    assert all(float(ref.state[params[idx]]["step"]) == float(st["step"]) for idx, st in state.items())
    assert params[all_names.index(ONE)] not in ref.state
