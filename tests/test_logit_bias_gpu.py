"""logit_bias in the fused HIP sampler (ops.sample_rows with a bias table on
GPU tensors) against the fp64 reference of tests/sample_reference.py.

The contract adds the bias to the raw logit in f32, l' = fl32(l + bias),
before the penalties; everything after is the sampler's contract, so the
reference is sample_reference.row_reference on l' and the tolerance is
sample_reference.derive_eps, unchanged.
"""
import functools

import numpy as np
import pytest
import torch

import sample_reference as sr
import dnet_amd.ops as ops
from dnet_amd.core.sampler import DecodingConfig, RowSampler

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEAD = (-100.0, -3.5, 2.25, -0.75, None, 1.5)


@functools.lru_cache(maxsize=None)
def bias_case(V, B=sr.B):
    """Per row: the 4 largest and 2 smallest logits, then 18 random ids;
    values HEAD (slot 4: +100 on every fourth row, else 6.0), then 18 draws
    from [-4, 4). The last write wins. -> (entries per row, table [B, V])."""
    logits, params, _ = sr.case(V, B)
    g = torch.Generator().manual_seed(4321 + V)
    table = torch.zeros(B, V)
    entries = []
    for b in range(B):
        order = logits[b].float().argsort(descending=True, stable=True)
        ids = order[:4].tolist() + order[-2:].tolist() \
            + torch.randint(0, V, (18,), generator=g).tolist()
        vals = [v if v is not None else (100.0 if b % 4 == 0 else 6.0)
                for v in HEAD] \
            + (torch.rand(18, generator=g) * 8 - 4).tolist()
        for i, v in zip(ids, vals):
            table[b, i] = v
        entries.append(list(zip(ids, vals)))
    return entries, table


def biased(logits, table):
    """fl32(l + bias) as numpy f32 rows."""
    return (logits.float().numpy().astype(np.float32)
            + table.numpy().astype(np.float32)).astype(np.float32)


def _run(logits, params, u, **kw):
    temp, top_k, top_p, min_p = sr.param_tensors(params, DEV)
    tok = ops.sample_rows(logits, temp, top_k, top_p, min_p,
                          torch.as_tensor(u, dtype=torch.float32).to(DEV),
                          **kw)
    return tok.cpu().numpy()


@pytest.mark.parametrize("V", sr.SHAPES)
def test_interval_and_keep_set(V):
    logits, params, plain = sr.case(V)
    _, table = bias_case(V)
    eps = sr.derive_eps(V)
    lb = biased(logits, table)
    refs = [sr.row_reference(lb[b], *params[b]) for b in range(sr.B)]
    # what the reference alone says about this case, before the kernel
    ambiguous = sum("margin" in r and r["margin"] <= eps for r in refs)
    changed = sum(
        ("keep" in r) and not np.array_equal(r["keep"], p["keep"])
        for r, p in zip(refs, plain))
    print(f"V={V} ambiguous={ambiguous} keep sets changed={changed}")
    assert ambiguous <= 1
    assert changed >= 13               # the bias matters on most rows
    dl, dt = logits.to(DEV), table.to(DEV)
    for u in sr.uniforms(V):
        toks = _run(dl, params, u, bias=dt)
        assert ((toks >= 0) & (toks < V)).all()
        sr.check_tokens(toks, refs, u, eps, cap=1)


def test_greedy_ban_and_force():
    V, B = 4099, 4
    logits, _, _ = sr.case(V, B)
    params = [(0.0, 0, 1.0, 0.0)] * B
    lf = logits.float()
    top, low = lf.argmax(-1), lf.argmin(-1)
    table = torch.zeros(B, V)
    for b in range(B):
        table[b, top[b] if b % 2 == 0 else low[b]] = \
            -100.0 if b % 2 == 0 else 100.0
    toks = _run(logits.to(DEV), params, np.zeros(B, np.float32),
                bias=table.to(DEV))
    lb = biased(logits, table)
    for b in range(B):
        assert toks[b] == int(np.argmax(lb[b].astype(np.float64)))
        if b % 2 == 0:
            assert toks[b] != int(top[b])
        else:
            assert toks[b] == int(low[b])


def _penalty_case(V, B=8):
    """As in test_sampler_gpu: logits of both signs and a hand-built seen
    table (prompt-only, generated, both) on the largest and smallest
    logits of each row and at random."""
    g = torch.Generator().manual_seed(77 + V)
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16)
    seen = torch.zeros(B, V, dtype=torch.int32)
    order = logits.float().argsort(dim=-1, descending=True)
    for b in range(B):
        hot = torch.cat([order[b, :6], order[b, -3:],
                         torch.randint(0, V, (40,), generator=g)])
        for n, t in enumerate(hot.tolist()):
            kind = n % 3
            if kind == 0:
                seen[b, t] = sr.PROMPT_BIT
            elif kind == 1:
                seen[b, t] = 1 + (n // 3) % 3
            else:
                seen[b, t] = sr.PROMPT_BIT | (1 + (n // 3) % 2)
    # bias on seen and unseen tokens; some flip the sign the penalty sees
    table = torch.zeros(B, V)
    for b in range(B):
        ids = order[b, :8].tolist() + order[b, -2:].tolist() \
            + torch.randint(0, V, (14,), generator=g).tolist()
        vals = [-9.0, -14.0, 3.0, -11.5] + \
            (torch.rand(20, generator=g) * 16 - 8).tolist()
        for i, v in zip(ids, vals):
            table[b, i] = v
    # row 0 shows the order of the two steps: token 100 (in the prompt) is
    # 32 / 1.3 = 24.6 with the bias first and 2 / 1.3 + 30 = 31.5 with the
    # penalty first; the unseen token 200 is 28 either way
    logits[0, 100], seen[0, 100], table[0, 100] = 2.0, sr.PROMPT_BIT, 30.0
    logits[0, 200], seen[0, 200], table[0, 200] = 1.5, 0, 26.5
    return logits, seen, table


REP, PRES, FREQ = 1.3, 0.7, 0.4


def _pen_tensors(B):
    f = lambda v: torch.full((B,), v, dtype=torch.float32, device=DEV)
    return dict(rep=f(REP), pres=f(PRES), freq=f(FREQ))


def test_bias_then_penalties():
    V, B = 4099, 8
    logits, seen, table = _penalty_case(V, B)
    lb = biased(logits, table)
    eps = sr.derive_eps(V)
    for params in ([(0.0, 0, 1.0, 0.0)] * B, [(0.7, 50, 0.9, 0.0)] * B):
        refs = [sr.row_reference(
            sr.penalise(lb[b], seen[b].numpy(), REP, PRES, FREQ),
            *params[b]) for b in range(B)]
        # the order matters: penalties on the unbiased logit, bias after,
        # pick another token on row 0
        other = [sr.row_reference(
            (sr.penalise(logits[b].float().numpy(), seen[b].numpy(), REP,
                         PRES, FREQ) + table[b].numpy()).astype(np.float32),
            *params[b]) for b in range(B)]
        if params[0][0] == 0.0:
            assert (refs[0]["token"], other[0]["token"]) == (200, 100)
        for u in sr.uniforms(V, B)[:4]:
            dseen = seen.to(DEV)
            toks = _run(logits.to(DEV), params, u, seen=dseen,
                        bias=table.to(DEV), **_pen_tensors(B))
            sr.check_tokens(toks, refs, u, eps, cap=0)
            expect = seen.clone()
            expect[torch.arange(B), torch.as_tensor(toks)] += 1
            assert torch.equal(dseen.cpu(), expect)


def test_flag_off_reads_nothing():
    """A row whose flag is off: its table row holds NaN and a winning +100,
    and the tokens equal those of a call without a table, bit for bit."""
    V = 4099
    logits, params, _ = sr.case(V)
    _, table = bias_case(V)
    table = table.clone()
    on = torch.zeros(sr.B, dtype=torch.bool)
    on[::3] = True
    table[~on] = float("nan")
    table[~on, 1234] = 100.0
    dl, dt, don = logits.to(DEV), table.to(DEV), on.to(DEV)
    lb = biased(logits, torch.where(on[:, None], table,
                                    torch.zeros_like(table)))
    refs = [sr.row_reference(lb[b], *params[b]) for b in range(sr.B)]
    eps = sr.derive_eps(V)
    for u in sr.uniforms(V):
        plain = _run(dl, params, u)
        toks = _run(dl, params, u, bias=dt, bias_on=don)
        assert np.array_equal(toks[~on.numpy()], plain[~on.numpy()])
        sr.check_tokens(toks, refs, u, eps, cap=1)
    # all flags off equals no table at all
    off = torch.zeros(sr.B, dtype=torch.bool, device=DEV)
    u = sr.uniforms(V)[4]
    assert np.array_equal(_run(dl, params, u, bias=dt, bias_on=off),
                          _run(dl, params, u))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_strided_bias_table(dtype):
    """Odd row strides of the bias table against contiguous and strided
    logits: every 16-byte phase of the one relative to the other. The
    table's padding holds +100, so a read outside the row shows."""
    V, B = 4099, 8
    logits, params, _ = sr.case(V, B, dtype)
    _, table = bias_case(V, B)
    lb = biased(logits, table)
    refs = [sr.row_reference(lb[b], *params[b]) for b in range(B)]
    eps = sr.derive_eps(V)
    u = sr.uniforms(V, B)[3]
    wl = torch.full((B, V + 10), 60.0, dtype=logits.dtype, device=DEV)
    for col in range(4):
        wide = torch.full((B, V + 10), 100.0, device=DEV)
        view = wide[:, col:V + col]
        view.copy_(table.to(DEV))
        assert view.stride(0) % 4 != 0
        sr.check_tokens(_run(logits.to(DEV), params, u, bias=view), refs, u,
                        eps, cap=0)
        lview = wl[:, 5 - col:V + 5 - col]
        lview.copy_(logits.to(DEV))
        sr.check_tokens(_run(lview, params, u, bias=view), refs, u, eps,
                        cap=0)


def _cfg(p, **kw):
    return DecodingConfig(temperature=p[0], top_k=p[1], top_p=p[2],
                          min_p=p[3], **kw)


PEN = dict(repetition_penalty=REP, presence_penalty=PRES,
           frequency_penalty=FREQ)


def test_row_sampler_fused_matches_torch_path():
    """RowSampler.sample on CUDA logits, fused and with fused off
    (apply_logit_bias / apply_penalties on device): biased, penalised and
    seeded rows over several steps give the same tokens and the same
    history wherever the fp64 reference has one answer."""
    V, steps = 4099, 3
    for seed in range(4242, 4342):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(6, V, generator=g) * 3
        if all(len(torch.unique(r)) == V for r in logits):
            break
    else:
        raise AssertionError("no tie-free logits")
    order = logits.argsort(dim=-1, descending=True)

    def bias_of(b):
        d = {int(order[b, 0]): -100.0, int(order[b, 1]): -2.5,
             int(order[b, 5]): 3.0, int(order[b, -1]): 7.0,
             V + 5: 100.0}                      # out of range: dropped
        d.update({int(i): float(v) for i, v in zip(
            torch.randint(0, V, (10,), generator=g),
            torch.rand(10, generator=g) * 8 - 4)})
        return d

    rows = [((0.7, 50, 0.9, 0.0), PEN, bias_of(0)),
            ((0.0, 0, 1.0, 0.0), PEN, bias_of(1)),
            ((1.0, 0, 1.0, 0.0), {}, bias_of(2)),
            ((1.0, 0, 1.0, 0.05), PEN, None),
            ((0.0, 0, 1.0, 0.0), {}, bias_of(4)),
            ((1.3, 0, 0.5, 0.0), {}, None)]
    B = len(rows)
    prompts = [order[b, :4].tolist()
               + torch.randint(0, V, (30,), generator=g).tolist()
               for b in range(B)]
    seeds = [7 + b if rows[b][0][0] > 0 else None for b in range(B)]
    sams = []
    for fused in (True, False):
        rs = RowSampler(B, device=DEV, vocab=V)
        rs.fused = fused
        for b, (p, pen, bias) in enumerate(rows):
            rs.set_row(b, _cfg(p, logit_bias=bias, **pen), seed=seeds[b])
            rs.note_prompt(b, prompts[b])
        sams.append(rs)
    fus, tor = sams
    assert fus.bias is not None and fus.bias.shape == (B, V)
    assert fus.bias_on.tolist() == [r[2] is not None for r in rows]
    table = fus.bias.cpu()
    for b, (_, _, bias) in enumerate(rows):     # last write, ids < V only
        want = torch.zeros(V)
        for i, v in (bias or {}).items():
            if i < V:
                want[i] = v
        assert torch.equal(table[b], want)
    gens = [torch.Generator(device=DEV).manual_seed(sd or 0) for sd in seeds]
    dl = logits.to(DEV)
    eps = sr.derive_eps(V)
    lb = biased(logits, table)
    wide = 0
    for _ in range(steps):
        us = [float(torch.rand(1, 1, device=DEV, generator=g_)) for g_ in gens]
        before = fus.seen.clone().cpu().numpy()
        a = fus.sample(dl).cpu().numpy()
        t = tor.sample(dl).cpu().numpy()
        for b, (p, pen, _) in enumerate(rows):
            l = lb[b]
            if pen:
                l = sr.penalise(l, before[b], REP, PRES, FREQ)
            r = sr.row_reference(l, *p)
            if "token" in r:
                assert a[b] == r["token"] == t[b], b
            elif r["margin"] <= eps:
                continue
            else:
                assert sr.interval_ok(int(a[b]), r, us[b], eps), b
                if sr.near_step(r, us[b], eps):
                    continue
                assert a[b] == t[b], (b, us[b], a[b], t[b])
            wide += 1
            assert torch.equal(fus.seen[b], tor.seen[b]), b
        tor.seen.copy_(fus.seen)       # resync rows with two right answers
    assert wide >= steps * B - 3
    # the banned argmax never came out of a greedy biased row
    assert int(order[4, 0]) != int(a[4])
    # a freed row stops reading its bias
    fus.clear_row(4)
    assert not bool(fus.bias_on[4])
    assert int(fus.sample(dl)[4]) == int(order[4, 0])


def test_row_sampler_all_greedy_biased_batch():
    """No sampled and no penalised row: the fused launch runs for the bias
    alone."""
    V, B = 4099, 3
    logits = (torch.randn(B, V, generator=torch.Generator()
                          .manual_seed(9)) * 3).to(torch.bfloat16).to(DEV)
    top = logits.float().argmax(-1)
    outs = []
    for fused in (True, False):
        rs = RowSampler(B, device=DEV, vocab=V)
        rs.fused = fused
        rs.set_row(0, DecodingConfig(logit_bias={int(top[0]): -100.0}))
        rs.set_row(1, DecodingConfig())
        rs.set_row(2, DecodingConfig(logit_bias={17: 100.0}))
        outs.append(rs.sample(logits))
        assert rs.seen is None
    assert torch.equal(outs[0], outs[1])
    assert outs[0][0] != top[0] and outs[0][1] == top[1] and outs[0][2] == 17
