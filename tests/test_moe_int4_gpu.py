"""MFMA grouped-expert decode pair for int4 banks (moe_int4.hip.cpp,
reached through ops.moe_gateup / ops.moe_down) against fp64 references
over the contract weights bf16(q*s) of tests/gemm_reference.py.

E = 5, top-2: expert 2 is never routed and, from M = 3 up, token 1 has an
all-zero ``we`` row. M = 1..32 run with four waves per column strip at
these sizes, so every case also runs with one (``ks``); M > 32 always runs
one. Every case prints its worst err/tol ratio (1.0 is the limit).
"""
import functools

import pytest
import torch

import gemm_reference as gr
import dnet_amd.ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F64 = torch.bfloat16, torch.float64
E, TOPK, DEAD = 5, 2, 2
ALPHA, LIMIT = 1.702, 7.0
MS = [1, 3, 16, 17, 33, 64]
KS = [0, 1]          # waves per strip: by shape (4 up to M = 32), forced 1


@pytest.fixture(autouse=True)
def _ks_by_shape():
    yield
    ops.moe_int4_force_ks(0)


def make_we(m: int, seed: int = 7) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed * 100 + m)
    live = torch.tensor([e for e in range(E) if e != DEAD])
    we = torch.zeros(m, E)
    for t in range(m):
        idx = live[torch.randperm(E - 1, generator=gen)[:TOPK]]
        we[t, idx] = torch.rand(TOPK, generator=gen) * 0.9 + 0.1
    if m >= 3:
        we[1] = 0.0
    return we


def make_bank(n, k, g, gen):
    """(packed nibbles [E, n, k/2], scales, fp64 contract weights); the
    never-routed expert's scales are NaN."""
    ws = [gr.make_weights("int4", n, k, g, gen) for _ in range(E)]
    sc = torch.stack([w["scales"] for w in ws])
    sc[DEAD] = float("nan")
    return (torch.stack([w["packed"] for w in ws]), sc,
            torch.stack([gr.contract_weights(w) for w in ws]))


def dev(t):
    return None if t is None else t.to(DEV)


def _report(name, r):
    print(f"[err/tol] {name}: {r:.3f}")
    assert r <= 1.0, f"{name}: err/tol = {r:.3f} > 1"


@functools.lru_cache(maxsize=None)
def gateup_inputs(m, k, g, i):
    gen = torch.Generator().manual_seed(1000 + m + k + i)
    c = dict(x=torch.randn(m, k, generator=gen).to(BF16), we=make_we(m),
             gb=torch.randn(E, 2 * i, generator=gen).to(BF16))
    c["gw"], c["gs"], c["gw64"] = make_bank(2 * i, k, g, gen)
    return c


def gateup_ratio(c, act, k, i, glu, bias):
    worst = 0.0
    for e in (c["we"] != 0).any(0).nonzero().flatten().tolist():
        bg, bu = (c["gb"][e, :i], c["gb"][e, i:]) if bias else (None, None)
        gv, ag = gr.gemm_ref(c["x"], c["gw64"][e, :i], bg)
        uv, au = gr.gemm_ref(c["x"], c["gw64"][e, i:], bu)
        dg, du = gr.gemm_acc(ag, k), gr.gemm_acc(au, k)
        if glu == 1:        # clamps are 1-Lipschitz; |d(g sig(a g))| <= 1.1
            gv, uv = gv.clamp(max=LIMIT), uv.clamp(-LIMIT, LIMIT) + 1.0
            s = gv * torch.sigmoid(ALPHA * gv)
            y = uv * s
        else:
            y, s = gr.swiglu_ref(gv, uv)
        worst = max(worst, gr.ratio(act[e], y, gr.swiglu_tol(y, uv, s, dg, du)))
    return worst


@pytest.mark.parametrize("ks", KS)
@pytest.mark.parametrize("glu,bias", [(0, False), (0, True), (1, False),
                                      (1, True)])
@pytest.mark.parametrize("i", [128, 384])
@pytest.mark.parametrize("k,g", [(128, 128), (384, 128), (512, 256)])
@pytest.mark.parametrize("m", MS)
def test_gateup_vs_fp64(m, k, g, i, glu, bias, ks):
    c = gateup_inputs(m, k, g, i)
    ops.moe_int4_force_ks(ks)
    act = ops.moe_gateup(dev(c["x"]), dev(c["gw"]), dev(c["gs"]),
                         dev(c["gb"]) if bias else None, dev(c["we"]), g,
                         True, glu, ALPHA, LIMIT).cpu()
    _report(f"gateup M{m} K{k} G{g} I{i} glu{glu} bias{int(bias)} ks{ks}",
            gateup_ratio(c, act, k, i, glu, bias))


@functools.lru_cache(maxsize=None)
def down_inputs(m, i, h):
    gen = torch.Generator().manual_seed(2000 + m + i + h)
    c = dict(act=torch.randn(E, m, i, generator=gen).to(BF16), we=make_we(m),
             db=torch.randn(E, h, generator=gen).to(BF16))
    c["act"][DEAD] = float("nan")     # a skipped expert's rows: never read
    c["dw"], c["ds"], c["dw64"] = make_bank(h, i, 128, gen)
    return c


def down_ratio(c, out, i, bias=True):
    """fp64 down over the routed (token, expert) pairs only."""
    we = c["we"].to(F64)
    want = torch.zeros(out.shape, dtype=F64)
    mag = torch.zeros(out.shape, dtype=F64)
    for e in range(E):
        toks = (we[:, e] != 0).nonzero().flatten()
        if not len(toks):
            continue
        d, ad = gr.gemm_ref(c["act"][e, toks], c["dw64"][e],
                            c["db"][e] if bias else None)
        want[toks] += we[toks, e, None] * d
        mag[toks] += we[toks, e, None].abs() * ad
    # one f32 ulp of the magnitude sum per step: I products, the bias, the
    # routing weight, topk adds; the output is f32 (no bf16 term)
    return gr.ratio(out, want, (i + TOPK + 2) * 2.0 ** -23 * mag)


def run_down(c, we, bias=True):
    return ops.moe_down(dev(c["act"]), dev(c["dw"]), dev(c["ds"]),
                        dev(c["db"]) if bias else None, dev(we), 128,
                        True).cpu()


@pytest.mark.parametrize("ks", KS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("h", [16, 80, 256])
@pytest.mark.parametrize("i", [128, 384])
@pytest.mark.parametrize("m", MS)
def test_down_vs_fp64(m, i, h, bias, ks):
    c = down_inputs(m, i, h)
    ops.moe_int4_force_ks(ks)
    out = run_down(c, c["we"], bias)
    if m >= 3:
        assert not out[1].any()
    _report(f"down M{m} I{i} H{h} bias{int(bias)} ks{ks}",
            down_ratio(c, out, i, bias))


@pytest.mark.parametrize("m", [16, 33])
def test_bits_repeat_and_ignore_other_tokens(m):
    c = down_inputs(m, 384, 80)
    out = run_down(c, c["we"])
    assert torch.equal(run_down(c, c["we"]), out)
    # every token but 0 and 2 gets another routing (other live experts,
    # other weights); the dead expert's act rows stay NaN and unrouted
    we2 = make_we(m, seed=8)
    assert not torch.equal(we2[3:], c["we"][3:])
    we2[0], we2[2] = c["we"][0], c["we"][2]
    out2 = run_down(c, we2)
    assert torch.equal(out2[0], out[0]) and torch.equal(out2[2], out[2])
    assert not torch.equal(out2[3:], out[3:])


def test_routing_and_graph_replay_follows_we():
    """The pair end to end: the never-routed expert's NaN scales reach
    nothing, a token without experts gets exact zeros, and a captured
    graph follows ``we`` rewritten in place."""
    m, k, g, i, h = 17, 384, 128, 384, 80
    c, d = gateup_inputs(m, k, g, i), down_inputs(m, i, h)
    x, gw, gs, gb = dev(c["x"]), dev(c["gw"]), dev(c["gs"]), dev(c["gb"])
    dw, ds, db = dev(d["dw"]), dev(d["ds"]), dev(d["db"])

    def pair(we):
        act = ops.moe_gateup(x, gw, gs, gb, we, g, True, 0)
        return ops.moe_down(act, dw, ds, db, we, 128, True)

    we = dev(c["we"]).clone()
    out0 = pair(we).cpu()                        # also the warm-up
    assert torch.isnan(gs[DEAD].float()).all() and not c["we"][1].any()
    assert torch.isfinite(out0).all() and not out0[1].any() and out0[0].any()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pair(we)
    for seed in (8, 9, 7):
        we_new = dev(make_we(m, seed=seed))
        we.copy_(we_new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, pair(we_new)), f"replay with routing {seed}"


def _new_vs_loop(fn, monkeypatch):
    calls, gateup = [], ops.moe_gateup
    monkeypatch.setattr(ops, "moe_gateup",
                        lambda *a: calls.append(1) or gateup(*a))
    new = fn()
    assert calls == [1], "the first run did not take the grouped pair"
    monkeypatch.setenv("DNET_MOE_INT4", "0")
    loop = fn()
    assert calls == [1], "the second run did not take the loop"
    diff = float((new.float() - loop.float()).abs().max())
    print(f"[int4 pair vs loop] max |diff| = {diff:.4g}, "
          f"max |out| = {float(loop.float().abs().max()):.4g}")
    assert torch.allclose(new.float(), loop.float(), atol=4e-2, rtol=4e-2)


TINY = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=4,
            vocab_size=128, num_experts_per_tok=2, rope_theta=10000.0)
MODELS = {      # every K is a multiple of 128
    "mixtral": dict(TINY, num_hidden_layers=1, intermediate_size=128,
                    num_local_experts=8),
    "deepseek_v2": dict(TINY, num_hidden_layers=2, intermediate_size=256,
                        kv_lora_rank=128, qk_nope_head_dim=64,
                        qk_rope_head_dim=64, v_head_dim=64,
                        n_routed_experts=8, n_shared_experts=1,
                        moe_intermediate_size=128, first_k_dense_replace=1,
                        routed_scaling_factor=2.5)}


@pytest.mark.parametrize("mt,rows", [("mixtral", 1), ("deepseek_v2", 3)])
def test_model_int4_vs_loop(mt, rows, monkeypatch):
    from dnet_amd.models import ModelConfig
    from dnet_amd.models.config import QuantConfig
    from dnet_amd.models.deepseek_v2 import DeepseekV2RingModel
    from dnet_amd.models.moe import MoERingModel
    cfg = ModelConfig.from_hf(dict(MODELS[mt], model_type=mt),
                              QuantConfig(4, 128))
    if mt == "mixtral":
        m = MoERingModel(cfg, [0], DEV, False, False)
    else:
        m = DeepseekV2RingModel(cfg, [0, 1], DEV, False, False, smax=64)
    m.init_random(seed=5)
    lw = m.layers[MODELS[mt]["num_hidden_layers"] - 1]
    eg0 = lw.experts_gateup[0]
    assert eg0.bits == 4 and eg0.packed and not eg0.mxfp4
    torch.manual_seed(3)
    y = torch.randn(rows, cfg.hidden_size, dtype=BF16, device=DEV)
    mlp = (lambda: m._mlp(y, lw)) if mt == "mixtral" else (
        lambda: m._mlp_for(1, y, lw))
    _new_vs_loop(mlp, monkeypatch)
