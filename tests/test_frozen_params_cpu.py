"""Frozen parameters (requires_grad = False), host side: freeze / unfreeze / trainable_names, the optimizer's rules for groups that
omit frozen parameters, and the effective group table of the masked AdamW launch - all without a GPU."""
import pytest
import torch

from mmfn_amd.config import GlobalConfig


@pytest.fixture()
def rad_model():
    from mmfn_amd.model import MMFNRad
    torch.manual_seed(0)
    return MMFNRad(GlobalConfig(), "cpu")


def test_freeze_returns_the_prefixed_names_and_flips_their_flags(rad_model):
    m = rad_model
    names = [n for n, _ in m.named_parameters()]
    assert len(m.trainable_names()) == len(names)
    want = [n for n in names if n.startswith("encoder.image_encoder")]
    got = m.freeze("encoder.image_encoder")
    assert got == want and len(want) > 100
    for n, p in m.named_parameters():
        assert p.requires_grad == (n not in set(want)), n
    assert m.trainable_names() == [n for n in names if n not in set(want)]
    # two prefixes, one of them overlapping what is frozen already; then everything back
    both = m.freeze("encoder.image_encoder.features.layer1", "join.")
    assert both == [n for n in names if n.startswith("encoder.image_encoder.features.layer1")] + [n for n in names if n.startswith("join.")]
    assert m.unfreeze("encoder.image_encoder") == want
    assert m.trainable_names() == [n for n in names if not n.startswith("join.")]
    assert m.freeze() == names and m.trainable_names() == []
    assert m.unfreeze() == names and m.trainable_names() == names


def test_unknown_prefix_raises_and_changes_nothing(rad_model):
    m = rad_model
    with pytest.raises(ValueError, match="no parameter name starts with"):
        m.freeze("encoder.image_encoder", "encoder.no_such_module")
    with pytest.raises(ValueError):
        m.unfreeze("nope")
    assert all(p.requires_grad for p in m.parameters())


def test_optimizer_takes_groups_without_the_frozen_parameters(rad_model):
    from mmfn_amd.optim import FusedAdamW
    m = rad_model
    m.freeze("encoder.image_encoder", "encoder.radar_encoder")
    opt = FusedAdamW(m, param_groups=[{"params": [p for p in m.parameters() if p.requires_grad]}])   # the torch idiom
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == len(m.trainable_names())
    assert opt.hyper_rows() == [(1e-3, 0.9, 0.999, 1e-8, 1e-2)]
    # a parameter unfrozen later that sits in no group: the next step has no hyper-parameters for it
    m.unfreeze("encoder.radar_encoder.mlp_1")
    with pytest.raises(ValueError, match="must cover every parameter"):
        opt.hyper_rows()
    with pytest.raises(ValueError, match="must cover every parameter"):
        opt.step()


def test_omitting_a_trainable_parameter_still_raises(rad_model):
    from mmfn_amd.optim import FusedAdamW
    m = rad_model
    m.freeze("encoder.image_encoder")
    params = [p for p in m.parameters() if p.requires_grad]
    with pytest.raises(ValueError, match="must cover every parameter"):
        FusedAdamW(m, param_groups=[{"params": params[1:]}])
    with pytest.raises(ValueError, match="must cover every parameter"):
        FusedAdamW(m, param_groups=[{"params": params[:-1]}])


def test_group_table_holds_255_over_frozen_float4s_and_the_group_id_beside_them(rad_model):
    from mmfn_amd.optim import FusedAdamW, configure_optimizers
    m = rad_model
    L = m._layout
    frozen = ["encoder.transformer2.pos_emb", "encoder.lidar_encoder._model.layer3.1.conv2.weight",
              "encoder.transformer1.blocks.0.attn.key.weight", "join.0.bias", "encoder.radar_encoder.attention_0.W"]
    for n in frozen:
        assert m.freeze(n) == [n]
    groups = configure_optimizers(m)   # decay = group 0, no decay = group 1
    gid_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    named = dict(m.named_parameters())
    # the filter idiom on top of the two groups
    opt = FusedAdamW(m, param_groups=[dict(g, params=[p for p in g["params"] if p.requires_grad]) for g in groups])
    tab = opt.group_table()
    assert tab.dtype == torch.uint8 and tab.device.type == "cpu" and tab.numel() == L.total // 4
    order = sorted((off, n, name) for name, (off, n) in L.offsets.items())
    for i, (off, n, name) in enumerate(order):
        first, last = off // 4, (off + n - 1) // 4
        if name in frozen:
            assert int(tab[first]) == 255 and int(tab[last]) == 255, name
            assert bool((tab[first:last + 1] == 255).all())
            for j in (i - 1, i + 1):   # the trainable neighbours in storage keep their optimizer group
                if 0 <= j < len(order) and order[j][2] not in frozen and order[j][2] not in L.unused:
                    o2, n2, nb = order[j]
                    want = gid_of[id(named[nb])]
                    assert int(tab[o2 // 4]) == want and int(tab[(o2 + n2 - 1) // 4]) == want, (name, nb)
        elif name not in L.unused:
            want = gid_of[id(named[name])]
            assert int(tab[first]) == want and int(tab[last]) == want, name
    assert int((tab == 255).sum()) == sum((L.offsets[n][1] + 3) // 4 for n in frozen)
    # one group (the engine passes no table at all then): zeros beside 255
    one = L.group_table(L.frozen_names())
    assert sorted(set(one.tolist())) == [0, 255] and torch.equal(one == 255, tab == 255)
    # adjacent frozen tensors merge into one range of whole float4s
    pair = ["encoder.transformer1.blocks.0.attn.key.weight", "encoder.transformer1.blocks.0.attn.query.weight"]
    (b, cnt), = L.merged_ranges(pair)
    assert b == L.offsets[pair[0]][0] and cnt == 2 * 64 * 64 and cnt % 4 == 0
