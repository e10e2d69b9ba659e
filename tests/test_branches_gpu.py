"""The VectorNet and radar-GAT branches inside the engine, each alone against its oracle sub-module in float64.

The end-to-end gradient tests judge these branches through 85 train-mode BatchNorms at a small batch, where fp32 itself is tens
of percent off.  Here the engine runs a whole "rad" training step, the branch's inputs, output and upstream gradient are recorded
at the branch boundary, and the oracle's sub-module (a float64 copy, same weights) is run on exactly those: VectorNet has only
LayerNorms and the GAT no normalisation at all, so the comparison holds the branch's own parameter gradients to fp32 accuracy.

Per tensor:  |g_gpu - g64| <= 4 * max(e_cpu, med_cpu * |g64|) + 2e-5 * |g64|     (L2 norms)
e_cpu is the fp32 CPU oracle's error against float64 on the same tensor and inputs, med_cpu the median relative oracle error over
the branch's tensors (test_train_step_matches_oracle's construction with 4x for 12x: another summation order may differ from the
CPU's by a small factor); 2e-5 is the fp32 kernel tolerance of test_kernels_gpu.py.  Figures: profiles/branch_tests_err.txt."""
import copy
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3


def _close(got, ref, tol=2e-5, what=""):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    scale = ref.abs().max().item() + 1e-6
    err = (got - ref).abs().max().item()
    print("branch-err branch | %s | err/scale %.3g | tol %.3g" % (what, err / scale, tol))
    assert err <= tol * scale, "%s max err %g vs scale %g" % (what, err, scale)


def _g(seed):
    return torch.Generator().manual_seed(seed)


_models = {}


def _model(dropout=0.0):
    """The "rad" model (it holds both branches) and its oracle, built once per dropout rate."""
    if dropout not in _models:
        from test_e2e_gpu import _dev_args, _setup
        oracle, net, batch, args = _setup("rad", B=B, dropout=dropout)
        net.train()
        _models[dropout] = (oracle, net, net._pack(*_dev_args(args)), batch["gt_wp"].to(DEV))
    return _models[dropout]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _models.clear()


def _lanes(L, counts, seed):
    """[B, L, 10, 5] lane nodes as fixtures.synthetic_batch draws them, rows >= the sample's count zero as pad_sequence leaves them."""
    g = _g(seed)
    lane = torch.zeros(B, L, 10, 5)
    lane[..., 0:2] = torch.randn(B, L, 10, 2, generator=g) * 8.0
    lane[..., 2:5] = torch.randint(0, 2, (B, L, 10, 3), generator=g).float()
    for b, n in enumerate(counts):
        lane[b, n:] = 0.0
    return lane.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


def _adjacency(seed):
    """Random 0/1 adjacency whose rows 60..80 are empty, as a short radar list leaves them."""
    adj = torch.randint(0, 2, (B, 81, 81), generator=_g(seed)).float()
    adj[:, 60:] = 0.0
    return adj.to(DEV)


def _record(monkeypatch, branch):
    """Wrap branch.fwd / branch.bwd: clones of the inputs, the output and the upstream gradient the engine hands over."""
    rec = {}
    fwd, bwd = branch.fwd, branch.bwd

    def fwd_rec(ctx, *inputs):
        rec["in"] = [t.clone() for t in inputs]
        out = fwd(ctx, *inputs)
        rec["out"] = out.clone()
        return out

    def bwd_rec(ctx, g_out):
        rec["g"] = g_out.clone()
        return bwd(ctx, g_out)

    monkeypatch.setattr(branch, "fwd", fwd_rec)
    monkeypatch.setattr(branch, "bwd", bwd_rec)
    return rec


def _step(net, inp, gt, monkeypatch, **replace):
    eng = net._engine_for()
    recs = {"vec": _record(monkeypatch, eng.vec), "rad": _record(monkeypatch, eng.rad)}
    inp = dict(inp, **replace)
    state = eng.rng_state.clone()
    eng.forward(inp, True, gt)
    eng.backward()
    torch.cuda.synchronize()
    assert torch.equal(state, eng.rng_state), "forward and backward leave the dropout counter alone"
    for r in recs.values():
        for k, v in list(r.items()):
            r[k] = [t.cpu() for t in v] if isinstance(v, list) else v.cpu()
    return recs, state


def _reference(sub, run, g_out, dtype):
    """Gradients of the oracle sub-module `sub` in `dtype`: out = run(copy of sub), out.backward(g_out)."""
    m = copy.deepcopy(sub).to(dtype).train()
    for p in m.parameters():
        p.grad = None
    out = run(m)
    out.backward(g_out.to(dtype))
    return out.detach(), {n: p.grad.detach().double() for n, p in m.named_parameters()}


def _judge(case, net, prefix, g64, g32):
    """The per-tensor bound of the module docstring over every parameter of the branch."""
    names = [n for n in g64 if g64[n].norm().item() > 0]
    rel_cpu = sorted((g32[n] - g64[n]).norm().item() / g64[n].norm().item() for n in names)
    med_cpu = rel_cpu[len(rel_cpu) // 2]
    bad = []
    for n, t in g64.items():
        got = net._layout.grad_views[prefix + n].detach().cpu().double()
        assert torch.isfinite(got).all(), n
        norm = t.norm().item()
        e_gpu, e_cpu = (got - t).norm().item(), (g32[n] - t).norm().item()
        bound = 4.0 * max(e_cpu, med_cpu * norm) + 2e-5 * norm
        print("branch-err branch | %s %s | e_gpu %.3g | e_cpu %.3g | ratio %.3g | |g64| %.3g | e_gpu/|g64| %.3g | bound/|g64| %.3g"
              % (case, n, e_gpu, e_cpu, e_gpu / max(e_cpu, 1e-300), norm, e_gpu / max(norm, 1e-300), bound / max(norm, 1e-300)))
        if not e_gpu <= bound:
            bad.append((n, e_gpu, e_cpu, norm))
    assert not bad, "%s gradient error (name, |gpu-f64|, |cpu32-f64|, |f64|): %s" % (case, bad)


# ------------------------------------------------------------------ VectorNet
@pytest.mark.parametrize("L,counts", [(9, (9, 4, 0)), (70, (70, 64, 1))])
def test_vectornet_branch_against_fp64(monkeypatch, L, counts):
    """L = 70 crosses the 64-key stride of the lane attention's wave loop; a sample without lanes and one with a single lane ride
    along.  Covers the split agent_fusion.0 weight, the single-row pos_emb gradients and L2L.to_qkv."""
    oracle, net, inp, gt = _model()
    lane, lane_num = _lanes(L, counts, seed=L)
    recs, _ = _step(net, inp, gt, monkeypatch, lane=lane, lane_num=lane_num)
    r = recs["vec"]
    lane_c, num_c = r["in"]
    assert tuple(lane_c.shape) == (B, L, 10, 5) and num_c.tolist() == list(counts)
    run = lambda m: m([[lane_c], [num_c], L])
    g_out = r["g"].float().permute(0, 3, 1, 2)   # NHWC -> the oracle's [B, 64, 64, 64] = (n, d, a)
    out64, g64 = _reference(oracle.encoder.vectornet_encoder, run, g_out, torch.float64)
    _, g32 = _reference(oracle.encoder.vectornet_encoder, run, g_out, torch.float32)
    case = "vectornet L=%d lanes=%s" % (L, counts)
    _close(r["out"].float().permute(0, 3, 1, 2), out64, 1e-5, case + " output")
    assert g64["pos_emb.0.weight"].abs().max().item() == 0.0
    assert (net._layout.grad_views["encoder.vectornet_encoder.pos_emb.0.weight"] == 0).all(), "pos_emb sees zeros: no weight gradient"
    assert {"agent_fusion.0.weight", "pos_emb.3.bias", "pos_emb.1.weight", "L2L.to_qkv.weight"} <= set(g64)
    _judge(case, net, "encoder.vectornet_encoder.", g64, g32)


# ------------------------------------------------------------------ radar GAT
def _spgat(mod, x, adj, masks):
    """_SpGAT.forward / _GATLayer.forward with every F.dropout replaced by the given keep-scale mask (stream id -> tensor)."""
    m = lambda sid, t: t * masks[sid].to(t.dtype).view(t.shape)
    x = m(900, x)
    heads = []
    for i in range(mod.nheads):
        layer = getattr(mod, "attention_%d" % i)
        wh = x @ layer.W
        e = F.leaky_relu(wh @ layer.a, layer.alpha)
        att = torch.softmax(torch.where(adj > 0, e, torch.full_like(e, -9e15)), dim=-1)
        heads.append(F.elu(m(901 + i, att) @ wh))
    x = m(904, torch.cat(heads, dim=1))
    x = m(905, mod.mlp_1[0](F.elu(x)))
    x = m(906, mod.mlp_2[0](x.transpose(1, 2)))
    return F.log_softmax(x.reshape(x.shape[0], 8, 8, 512).transpose(1, 3), dim=1)


def test_radar_gat_branch_against_fp64(monkeypatch):
    oracle, net, inp, gt = _model()
    recs, _ = _step(net, inp, gt, monkeypatch, radar_adj=_adjacency(5))
    r = recs["rad"]
    radar, adj = r["in"]
    assert (adj[:, 60:] == 0).all() and set(adj.unique().tolist()) == {0.0, 1.0}
    g_out = r["g"].float().permute(0, 3, 1, 2)   # NHWC [B, 8, 8, 512] -> the oracle's [B, 512, 8, 8]
    run = lambda m: m(radar.to(m.mlp_1[0].weight.dtype), adj.to(m.mlp_1[0].weight.dtype))
    out64, g64 = _reference(oracle.encoder.radar_encoder, run, g_out, torch.float64)
    _, g32 = _reference(oracle.encoder.radar_encoder, run, g_out, torch.float32)
    assert len(g64) == 8
    _close(r["out"].float().permute(0, 3, 1, 2), out64, 1e-5, "radar GAT output")
    _judge("radar GAT", net, "encoder.radar_encoder.", g64, g32)


def test_radar_gat_branch_with_dropout_against_fp64(monkeypatch):
    """Dropout 0.1 at the branch's dropout sites: the input (stream 900), the two heads' attention (901, 902), the concatenated
    heads (904), mlp_1's and mlp_2's outputs (905, 906).  The masks are rebuilt with ops.dropout_apply from the engine's counter
    state and put into a float64 functional copy of the oracle's forward: this pins the stream id, the flat index and the
    1 / (1 - p) scaling of every site in the forward and in the backward, which regenerates each mask instead of storing it."""
    from mmfn_amd import ops
    oracle, net, inp, gt = _model(dropout=0.1)
    assert net._engine_for().rad.p == pytest.approx(0.1)
    recs, state = _step(net, inp, gt, monkeypatch, radar_adj=_adjacency(6))
    r = recs["rad"]
    radar, adj = r["in"]
    sizes = {900: B * 81 * 5, 901: B * 81 * 81, 902: B * 81 * 81, 903: B * 81 * 81, 904: B * 162 * 162, 905: B * 162 * 256,
             906: B * 256 * 128}
    masks = {}
    for sid, n in sizes.items():
        ones = torch.ones(n, device=DEV)
        masks[sid] = ops.dropout_apply(ones, torch.full_like(ones, float("nan")), 0.1, state, sid).cpu()
        kept = (masks[sid] > 0).float().mean().item()
        assert abs(kept - 0.9) <= 0.03 and masks[sid].max().item() == pytest.approx(1.0 / 0.9, rel=1e-6), (sid, kept)
    # independent Bernoulli(0.9) masks agree on 0.81 + 0.01 = 0.82 of their entries (903 is the stream a third head would take)
    for a in sizes:
        for b in sizes:
            if a < b:
                n = min(sizes[a], sizes[b])
                agree = ((masks[a][:n] > 0) == (masks[b][:n] > 0)).float().mean().item()
                assert agree <= 0.9, (a, b, agree)
    g_out = r["g"].float().permute(0, 3, 1, 2)
    shaped = {900: (B, 81, 5), 901: (B, 81, 81), 902: (B, 81, 81), 904: (B, 162, 162), 905: (B, 162, 256), 906: (B, 256, 128)}
    mk = {sid: masks[sid].view(shape) for sid, shape in shaped.items()}
    run = lambda m: _spgat(m, radar.to(m.mlp_1[0].weight.dtype), adj.to(m.mlp_1[0].weight.dtype), mk)
    out64, g64 = _reference(oracle.encoder.radar_encoder, run, g_out, torch.float64)
    _, g32 = _reference(oracle.encoder.radar_encoder, run, g_out, torch.float32)
    assert len(g64) == 8
    _close(r["out"].float().permute(0, 3, 1, 2), out64, 1e-5, "radar GAT dropout 0.1 output")
    _judge("radar GAT dropout 0.1", net, "encoder.radar_encoder.", g64, g32)


def test_radar_gat_refuses_a_head_count_that_shares_dropout_streams():
    """Head h draws its attention mask from stream 900 + 1 + h and the later sites use 904, 905 and 906: a fourth head would share
    904 with the concatenated heads' dropout."""
    from mmfn_amd import engine
    mod = types.SimpleNamespace(nheads=4, alpha=0.2, dropout=0.1)
    with pytest.raises(ValueError, match="stream"):
        engine.RadarGAT("rad", None, "encoder.radar_encoder", mod)
