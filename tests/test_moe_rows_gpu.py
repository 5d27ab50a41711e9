"""Token-routed MoE path (moe_route / moe_gateup_rows / moe_down_rows)
against fp64 references built from tests/gemm_reference.py.

One hand-built ``we`` [130, 8] holds experts with 129/130, 0, exactly 64,
65 and 1 tokens and tokens with 3, 2, 1 and 0 routed experts. An expert
that owns all 130 tokens and a token without any expert exclude each
other, so ``we`` comes in two variants: ``unrouted`` clears the last
token's row (expert 0 then owns 129 tokens). Every case prints its worst
err/tol ratio (1.0 is the limit).
"""
import functools

import pytest
import torch

import gemm_reference as gr
import dnet_amd.ops as ops
from dnet_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F64 = torch.bfloat16, torch.float64
T, E, H, TOPK = 130, 8, 320, 3
ALPHA, LIMIT = 1.702, 7.0
# (format, group, K, I): int8 G = 128 needs K and I (the down stage's
# inner dim) to be multiples of 128
FORMATS = [("bf16", 0, 320, 192), ("int8", 64, 320, 192),
           ("int8", 128, 384, 384), ("mxfp4", 32, 320, 192)]
FMT_IDS = ["bf16", "int8-g64", "int8-g128", "mxfp4"]


@functools.lru_cache(maxsize=None)
def make_we(unrouted: bool) -> torch.Tensor:
    gen = torch.Generator().manual_seed(7)
    we = torch.zeros(T, E)
    we[:, 0] = 1.0                  # every token; expert 1 stays empty
    we[0:64, 2] = 1.0               # exactly one full tile
    we[60:125, 3] = 1.0             # 65: a full tile and one row
    we[5, 4] = 1.0                  # a single token
    extra = torch.randint(5, 8, (T,), generator=gen)
    add = (torch.rand(T, generator=gen) < 0.5) & ((we != 0).sum(1) < TOPK)
    add[125:] = False               # tokens 125.. keep one expert
    we[add, extra[add]] = 1.0
    val = torch.rand(T, E, generator=gen) * 0.9 + 0.1
    val = val * torch.where(torch.rand(T, E, generator=gen) < 0.25, -1.0, 1.0)
    we = we * val
    if unrouted:
        we[T - 1] = 0.0
    return we


def make_bank(fmt, n, k, g, gen):
    """E stacked [n, k] matrices -> (w, scales, fp64 contract weights,
    group, packed)."""
    if fmt == "mxfp4":
        w = torch.randint(0, 256, (E, n, k // 2), generator=gen,
                          dtype=torch.int16).to(torch.uint8)
        s = torch.randint(118, 123, (E, n, k // 32), generator=gen,
                          dtype=torch.int16).to(torch.uint8)
        w64 = ref.dequant_mxfp4(w.view(E * n, -1), s.view(E * n, -1))
        return w, s, w64.to(F64).view(E, n, k), 32, False
    ws = [gr.make_weights(fmt, n, k, g, gen) for _ in range(E)]
    w64 = torch.stack([gr.contract_weights(w) for w in ws])
    sc = None if fmt == "bf16" else torch.stack([w["scales"] for w in ws])
    return torch.stack([w["packed"] for w in ws]), sc, w64, g, fmt == "int8"


def dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def run_case(fi: int, glu: int, unrouted: bool = True) -> dict:
    """Inputs, the kernels' act/out and the plan (on the CPU) of one
    format; shared by the tests and left unchanged."""
    fmt, g, K, I = FORMATS[fi]
    gen = torch.Generator().manual_seed(100 + fi)
    c = dict(K=K, I=I, we=make_we(unrouted))
    c["x"] = torch.randn(T, K, generator=gen).to(BF16)
    c["gb"] = torch.randn(E, 2 * I, generator=gen).to(BF16)
    c["db"] = torch.randn(E, H, generator=gen).to(BF16)
    gw, gs, c["gw64"], grp, packed = make_bank(fmt, 2 * I, K, g, gen)
    dw, ds, c["dw64"], _, _ = make_bank(fmt, H, I, g, gen)

    def call(x, we):
        plan = ops.moe_route(dev(we), TOPK)
        act = ops.moe_gateup_rows(dev(x), dev(gw), dev(gs), dev(c["gb"]),
                                  plan, grp, packed, glu, ALPHA, LIMIT)
        out = ops.moe_down_rows(act, dev(dw), dev(ds), dev(c["db"]), dev(we),
                                plan, grp, packed)
        return plan, act.cpu(), out.cpu()

    c["call"] = call
    plan, c["act"], c["out"] = call(c["x"], c["we"])
    c["plan"] = {k: v.cpu() if torch.is_tensor(v) else v
                 for k, v in plan.items()}
    return c


def _report(name, r):
    print(f"[err/tol] {name}: {r:.3f}")
    assert r <= 1.0, f"{name}: err/tol = {r:.3f} > 1"


@pytest.mark.parametrize("unrouted", [False, True])
def test_plan_matches_torch(unrouted):
    we = make_we(unrouted)
    plan = ops.moe_route(we.to(DEV), TOPK)
    nz = we != 0
    counts = nz.sum(0)
    offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    e_idx, t_idx = nz.t().nonzero(as_tuple=True)
    token_slots = torch.full((T, TOPK), -1)
    token_slots[t_idx, nz.cumsum(1)[t_idx, e_idx] - 1] = torch.arange(
        t_idx.numel())
    tiles = [(e, int(offsets[e]) + s, min(64, int(counts[e]) - s))
             for e in range(E) for s in range(0, int(counts[e]), 64)]
    n = t_idx.numel()
    assert sorted(set(counts.tolist()) & {0, 1, 64, 65}) == [0, 1, 64, 65]
    assert int(counts[0]) == T - unrouted
    assert set(nz.sum(1).tolist()) == {1, 2, 3} | ({0} if unrouted else set())
    assert plan["counts"].cpu().tolist() == counts.tolist()
    assert plan["offsets"].cpu().tolist() == offsets.tolist()
    assert plan["slot_token"].cpu().tolist() == (
        t_idx.tolist() + [-1] * (plan["slots_cap"] - n))
    assert plan["token_slots"].cpu().tolist() == token_slots.tolist()
    assert int(plan["ntiles"]) == len(tiles)
    assert plan["tiles"].cpu()[:len(tiles)].tolist() == [list(t) for t in tiles]


@pytest.mark.parametrize("fi,glu,unrouted", [
    (fi, glu, True) for fi in range(4) for glu in (0, 1)] + [(3, 1, False)])
def test_gateup_vs_fp64(fi, glu, unrouted):
    c = run_case(fi, glu, unrouted)
    I, off = c["I"], c["plan"]["offsets"].tolist()
    worst = 0.0
    for e in range(E):
        toks = c["plan"]["slot_token"][off[e]:off[e + 1]].long()
        if not len(toks):
            continue
        x = c["x"][toks]
        g, ag = gr.gemm_ref(x, c["gw64"][e, :I], c["gb"][e, :I])
        u, au = gr.gemm_ref(x, c["gw64"][e, I:], c["gb"][e, I:])
        dg, du = gr.gemm_acc(ag, c["K"]), gr.gemm_acc(au, c["K"])
        if glu == 1:        # clamps are 1-Lipschitz; |d(g sig(a g))| <= 1.1
            g, u = g.clamp(max=LIMIT), u.clamp(-LIMIT, LIMIT) + 1.0
            s = g * torch.sigmoid(ALPHA * g)
            y = u * s
        else:
            y, s = gr.swiglu_ref(g, u)
        tol = gr.swiglu_tol(y, u, s, dg, du)
        worst = max(worst, gr.ratio(c["act"][off[e]:off[e + 1]], y, tol))
    _report(f"gateup {FMT_IDS[fi]} glu{glu} unrouted{int(unrouted)}", worst)


@pytest.mark.parametrize("fi", range(4), ids=FMT_IDS)
def test_down_vs_fp64(fi):
    c = run_case(fi, 0, True)
    off, we = c["plan"]["offsets"].tolist(), c["we"].to(F64)
    want = torch.zeros(T, H, dtype=F64)
    mag = torch.zeros(T, H, dtype=F64)
    for e in range(E):
        toks = c["plan"]["slot_token"][off[e]:off[e + 1]].long()
        d, ad = gr.gemm_ref(c["act"][off[e]:off[e + 1]], c["dw64"][e],
                            c["db"][e])
        want[toks] += we[toks, e, None] * d
        mag[toks] += we[toks, e, None].abs() * ad
    # one f32 ulp of the magnitude sum per step: I products, the bias, the
    # routing weight, topk adds; the output is f32 (no bf16 term)
    tol = (c["I"] + TOPK + 2) * 2.0 ** -23 * mag
    assert not c["out"][T - 1].any() and not mag[T - 1].any()
    _report(f"down {FMT_IDS[fi]}", gr.ratio(c["out"], want, tol))


@pytest.mark.parametrize("fi", range(4), ids=FMT_IDS)
def test_bits_repeat_and_ignore_other_tokens(fi):
    c = run_case(fi, 0, True)
    _, act, out = c["call"](c["x"], c["we"])
    live = int(c["plan"]["offsets"][E])
    assert torch.equal(act[:live], c["act"][:live])
    assert torch.equal(out, c["out"])
    plan70, act70, out70 = c["call"](c["x"][:70], c["we"][:70])
    ts, ts70 = c["plan"]["token_slots"][:70], plan70["token_slots"].cpu()
    assert torch.equal(ts >= 0, ts70 >= 0) and int((ts >= 0).sum()) > 140
    assert torch.equal(act70[ts70[ts70 >= 0].long()],
                       c["act"][ts[ts >= 0].long()])
    assert torch.equal(out70, c["out"][:70])


@pytest.mark.parametrize("fmt,g", [("int8", 64), ("int8", 128), ("mxfp4", 32)])
def test_onehot_down_returns_contract_weights(fmt, g):
    """act = rows of I_I through expert 1 of 2 with we = 1: out[t, h] is
    the contract weight Wd[1][h, t], exactly (k and scale index mapping of
    the packed layouts; 384 = a 256-k tile and a 128-k tail, 6 row tiles)."""
    I = 384
    gen = torch.Generator().manual_seed(11)
    dw, ds, w64, grp, packed = make_bank(fmt, H, I, g, gen)
    we = torch.zeros(I, E)
    we[:, 1] = 1.0
    plan = ops.moe_route(we.to(DEV), 1)
    out = ops.moe_down_rows(torch.eye(I, dtype=BF16, device=DEV), dev(dw),
                            dev(ds), None, we.to(DEV), plan, grp, packed)
    assert torch.equal(out.cpu().to(F64), w64[1].t())


def _two_paths(cls, fn, monkeypatch):
    calls, route = [], ops.moe_route
    monkeypatch.setattr(ops, "moe_route",
                        lambda *a: calls.append(1) or route(*a))
    rows = fn()
    assert calls == [1], "the first run did not take the rows path"
    monkeypatch.setattr(cls, "ROWS_MOE_MIN_T", 1 << 30)
    loop = fn()
    assert calls == [1], "the second run did not take the loop"
    diff = float((rows.float() - loop.float()).abs().max())
    print(f"[rows vs loop] {cls.__name__}: max |diff| = {diff:.4g}, "
          f"max |out| = {float(loop.float().abs().max()):.4g}")
    assert torch.allclose(rows.float(), loop.float(), atol=4e-2, rtol=4e-2)


def test_model_gpt_oss_mxfp4_rows_vs_loop(monkeypatch):
    from dnet_amd.models import ModelConfig, PRESETS
    from dnet_amd.models.config import QuantConfig
    from dnet_amd.models.gpt_oss import GptOssRingModel
    hf = dict(PRESETS["gpt-oss-20b"])
    hf["num_hidden_layers"] = 2
    cfg = ModelConfig.from_hf(hf, QuantConfig(fmt="mxfp4"))
    m = GptOssRingModel(cfg, [0, 1], DEV, False, False)
    m.init_random(seed=5)
    assert m.layers[0].experts_gateup[0].mxfp4
    torch.manual_seed(3)
    y = torch.randn(96, cfg.hidden_size, dtype=BF16, device=DEV)
    _two_paths(GptOssRingModel, lambda: m._mlp(y, m.layers[0]), monkeypatch)


def test_model_deepseek_int8_rows_vs_loop(monkeypatch):
    """int8 banks are off by default (slower than the loop, see
    docs/KERNELS.md); the model's wiring is tested with the gate forced."""
    monkeypatch.setattr(ops, "moe_rows_supported", lambda *a: True)
    from dnet_amd.models import ModelConfig
    from dnet_amd.models.config import QuantConfig
    from dnet_amd.models.deepseek_v2 import DeepseekV2RingModel
    cfg = ModelConfig.from_hf(dict(
        model_type="deepseek_v2", hidden_size=256, num_hidden_layers=2,
        num_attention_heads=4, num_key_value_heads=4, vocab_size=128,
        intermediate_size=256, kv_lora_rank=64, qk_nope_head_dim=64,
        qk_rope_head_dim=64, v_head_dim=64, n_routed_experts=8,
        num_experts_per_tok=2, n_shared_experts=1, moe_intermediate_size=128,
        first_k_dense_replace=1, routed_scaling_factor=2.5,
        rope_theta=10000.0), QuantConfig(8, 64))
    m = DeepseekV2RingModel(cfg, [0, 1], DEV, False, False, smax=64)
    m.init_random(seed=5)
    assert m.layers[1].experts_gateup[0].packed
    torch.manual_seed(3)
    y = torch.randn(96, cfg.hidden_size, dtype=BF16, device=DEV)
    _two_paths(DeepseekV2RingModel, lambda: m._mlp_for(1, y, m.layers[1]),
               monkeypatch)
