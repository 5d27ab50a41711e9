"""Token-routed int4 expert kernels (ops.moe_gateup_rows / moe_down_rows on
uint8 banks with bf16 scales) against fp64 over the contract weights. One
hand-built ``we`` [200, 8], top-k 4: experts with 199, 0 (NaN scales), 64, 65,
1, 128, 129 and 21 tokens, tokens with 0 to 4 experts. 1.0 = the tolerance."""
import functools

import pytest
import torch

import gemm_reference as gr
import dnet_amd.ops as ops
from test_moe_int4_gpu import MODELS        # the tiny int4 model configs

pytestmark = pytest.mark.gpu
DEV, BF16, F64 = "cuda:0", torch.bfloat16, torch.float64
T, E, TOPK, ALPHA, LIMIT = 200, 8, 4, 1.702, 7.0
BANKS = [(128, 128, 384), (384, 128, 128), (512, 256, 256)]     # K, G, I
COUNTS = [199, 0, 64, 65, 1, 128, 129, 21]


def make_we() -> torch.Tensor:
    gen = torch.Generator().manual_seed(7)
    we = torch.zeros(T, E)
    for e, rows in enumerate([range(199), [], range(64), range(60, 125), [5],
                              range(70, 198), range(66, 195),
                              range(0, 42, 2)]):
        we[list(rows), e] = 1.0
    val = torch.rand(T, E, generator=gen) * 0.9 + 0.1
    return we * val * torch.where(torch.rand(T, E, generator=gen) < 0.25,
                                  -1.0, 1.0)


def make_bank(n, k, g, gen, experts=E, nan=1):
    """-> (packed nibbles, scales with NaN in expert ``nan``, fp64 w)."""
    ws = [gr.make_weights("int4", n, k, g, gen) for _ in range(experts)]
    sc = torch.stack([w["scales"] for w in ws])
    sc[nan] = float("nan")
    return (torch.stack([w["packed"] for w in ws]), sc,
            torch.stack([gr.contract_weights(w) for w in ws]))


def dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def run_case(ci: int, glu: int, H: int) -> dict:
    """One bank's inputs, act/out and plan on the CPU; shared, unchanged."""
    K, G, I = BANKS[ci]
    gen = torch.Generator().manual_seed(100 + ci)
    c = dict(K=K, I=I, we=make_we())
    c["x"] = torch.randn(T, K, generator=gen).to(BF16)
    c["gb"] = torch.randn(E, 2 * I, generator=gen).to(BF16)
    c["db"] = torch.randn(E, H, generator=gen).to(BF16)
    gw, gs, c["gw64"] = make_bank(2 * I, K, G, gen)
    dw, ds, c["dw64"] = make_bank(H, I, G, gen)

    def call(x, we):
        plan = ops.moe_route(dev(we), TOPK)
        act = ops.moe_gateup_rows(dev(x), dev(gw), dev(gs), dev(c["gb"]),
                                  plan, G, True, glu, ALPHA, LIMIT)
        out = ops.moe_down_rows(act, dev(dw), dev(ds), dev(c["db"]), dev(we),
                                plan, G, True)
        return plan, act.cpu(), out.cpu()

    c["call"] = call
    plan, c["act"], c["out"] = call(c["x"], c["we"])
    c["plan"] = {k: v.cpu() if torch.is_tensor(v) else v
                 for k, v in plan.items()}
    return c


def _report(name, r):
    print(f"[err/tol] {name}: {r:.3f}")
    assert r <= 1.0, f"{name}: err/tol = {r:.3f} > 1"


def _slots(c, e):
    sl = slice(*c["plan"]["offsets"][e:e + 2].tolist())
    return sl, c["plan"]["slot_token"][sl].long()


@pytest.mark.parametrize("glu", [0, 1])
@pytest.mark.parametrize("ci", range(3))
def test_gateup_vs_fp64(ci, glu):
    c = run_case(ci, glu, 64)
    nz = c["we"] != 0
    assert nz.sum(0).tolist() == COUNTS == c["plan"]["counts"].tolist()
    assert set(nz.sum(1).tolist()) == {0, 1, 2, 3, 4} and (c["we"] < 0).any()
    I, worst = c["I"], 0.0
    for e in range(E):
        sl, toks = _slots(c, e)
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
        worst = max(worst, gr.ratio(c["act"][sl], y,
                                    gr.swiglu_tol(y, u, s, dg, du)))
    _report(f"gateup {BANKS[ci]} glu{glu}", worst)


@pytest.mark.parametrize("H", [64, 320])
@pytest.mark.parametrize("ci", range(3))
def test_down_vs_fp64(ci, H):
    c = run_case(ci, 0, H)
    we = c["we"].to(F64)
    want = torch.zeros(T, H, dtype=F64)
    mag = torch.zeros(T, H, dtype=F64)
    for e in range(E):
        sl, toks = _slots(c, e)
        d, ad = gr.gemm_ref(c["act"][sl], c["dw64"][e], c["db"][e])
        want[toks] += we[toks, e, None] * d
        mag[toks] += we[toks, e, None].abs() * ad
    # one f32 ulp of the magnitude sum per step: I products, the bias, the
    # routing weight, topk adds (f32 output)
    tol = (c["I"] + TOPK + 2) * 2.0 ** -23 * mag
    assert not c["out"][T - 1].any() and not torch.isnan(c["out"]).any()
    _report(f"down {BANKS[ci]} H{H}", gr.ratio(c["out"], want, tol))


@pytest.mark.parametrize("ci", range(3))
def test_bits_repeat_and_ignore_other_tokens(ci):
    c = run_case(ci, 0, 320)
    _, act, out = c["call"](c["x"], c["we"])
    assert torch.equal(act[:sum(COUNTS)], c["act"][:sum(COUNTS)])
    assert torch.equal(out, c["out"])
    plan70, act70, out70 = c["call"](c["x"][:70], c["we"][:70])
    ts, ts70 = c["plan"]["token_slots"][:70], plan70["token_slots"].cpu()
    assert torch.equal(ts >= 0, ts70 >= 0) and int((ts >= 0).sum()) == 170
    assert torch.equal(act70[ts70[ts70 >= 0].long()],
                       c["act"][ts[ts >= 0].long()])
    assert torch.equal(out70, c["out"][:70])


@pytest.mark.parametrize("g", [128, 384])
def test_onehot_down_returns_contract_weights(g):
    """act = I_384 through expert 1 of 2 with we = 1 returns Wd[1] as contract
    weights exactly (nibble, quad, scale index; a stage + a tail, 6 tiles)."""
    I, H = 384, 320
    dw, ds, w64 = make_bank(H, I, g, torch.Generator().manual_seed(11), 2, 0)
    we = torch.zeros(I, 2)
    we[:, 1] = 1.0
    plan = ops.moe_route(we.to(DEV), 1)
    out = ops.moe_down_rows(torch.eye(I, dtype=BF16, device=DEV), dev(dw),
                            dev(ds), None, we.to(DEV), plan, g, True)
    assert torch.equal(out.cpu().to(F64), w64[1].t())


@pytest.mark.parametrize("mt", ["mixtral", "deepseek_v2"])
def test_model_int4_rows_vs_loop(mt, monkeypatch):
    from dnet_amd.models import ModelConfig
    from dnet_amd.models.config import QuantConfig
    from dnet_amd.models.deepseek_v2 import DeepseekV2RingModel
    from dnet_amd.models.moe import MoERingModel
    cfg = ModelConfig.from_hf(dict(MODELS[mt], model_type=mt),
                              QuantConfig(4, 128))
    m = (MoERingModel(cfg, [0], DEV, False, False) if mt == "mixtral" else
         DeepseekV2RingModel(cfg, [0, 1], DEV, False, False, smax=64))
    m.init_random(seed=5)
    lw = m.layers[MODELS[mt]["num_hidden_layers"] - 1]
    torch.manual_seed(3)
    y = torch.randn(96, cfg.hidden_size, dtype=BF16, device=DEV)
    fn = (lambda: m._mlp(y, lw)) if mt == "mixtral" else (
        lambda: m._mlp_for(1, y, lw))
    calls, route = [], ops.moe_route
    monkeypatch.setattr(ops, "moe_route",
                        lambda *a: calls.append(1) or route(*a))
    rows = fn()
    assert calls == [1], "the first run did not take the rows path"
    monkeypatch.setattr(type(m), "ROWS_MOE_MIN_T", 1 << 30)
    loop = fn()
    assert calls == [1], "the second run did not take the loop"
    assert torch.allclose(rows.float(), loop.float(), atol=4e-2, rtol=4e-2)
