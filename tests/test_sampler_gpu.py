"""The fused HIP sampler (ops.sample_rows on GPU tensors) against the fp64
reference of tests/sample_reference.py.

The kernel works in f32 and fixed point, so a token is accepted when it
lies in the fp64 keep set and the uniform falls within eps of its fp64 cdf
interval; eps is derived from the kernel's reduction shape
(sample_reference.derive_eps). Rows whose fp64 margin to another keep set
is <= eps are skipped, at most one row in 16 per shape.
"""
import numpy as np
import pytest
import torch

import sample_reference as sr
import dnet_amd.ops as ops
from dnet_amd.core.sampler import DecodingConfig, RowSampler

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(logits, params, u, **pen):
    temp, top_k, top_p, min_p = sr.param_tensors(params, DEV)
    tok = ops.sample_rows(logits, temp, top_k, top_p, min_p,
                          torch.as_tensor(u, dtype=torch.float32).to(DEV),
                          **pen)
    return tok.cpu().numpy()


@pytest.mark.parametrize("V", sr.SHAPES)
def test_interval_and_keep_set(V):
    logits, params, refs = sr.case(V)
    eps = sr.derive_eps(V)
    assert eps <= 2.0 ** -16
    dl = logits.to(DEV)
    for u in sr.uniforms(V):
        toks = _run(dl, params, u)
        assert ((toks >= 0) & (toks < V)).all()
        skipped = sr.check_tokens(toks, refs, u, eps, cap=1)
    print(f"V={V} eps=2^{np.log2(eps):.2f} skipped={skipped}")


def test_strided_rows():
    """B = 3, V = 4099, row stride > V: rows start at every 16-byte phase."""
    V, B = 4099, 3
    logits, params, refs = sr.case(V, B)
    # odd stride; the padding holds winning logits, so a read past a row's
    # end or before its start changes the answer
    wide = torch.full((B, V + 12), 60.0, dtype=torch.bfloat16, device=DEV)
    view = wide[:, 3:V + 3]
    view.copy_(logits.to(DEV))
    assert view.stride(0) == V + 12 and view.stride(0) % 8 != 0
    eps = sr.derive_eps(V)
    for u in sr.uniforms(V, B):
        sr.check_tokens(_run(view, params, u), refs, u, eps, cap=0)


def _penalty_case(V, B=8):
    """Logits of both signs and a hand-built seen table: prompt-only
    tokens, generated tokens (count 1..3) and tokens that are both, placed
    on the largest and smallest logits of each row and at random."""
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
    return logits, seen


REP, PRES, FREQ = 1.3, 0.7, 0.4


def _pen_tensors(B):
    f = lambda v: torch.full((B,), v, dtype=torch.float32, device=DEV)
    return dict(rep=f(REP), pres=f(PRES), freq=f(FREQ))


def test_penalties_greedy_and_counts():
    V, B = 4099, 8
    logits, seen = _penalty_case(V, B)
    params = [(0.0, 0, 1.0, 0.0)] * B
    dseen = seen.to(DEV)
    toks = _run(logits.to(DEV), params, np.zeros(B, np.float32),
                seen=dseen, **_pen_tensors(B))
    checked = moved = 0
    for b in range(B):
        l64 = sr.penalise(logits[b].float().numpy(), seen[b].numpy(), REP,
                          PRES, FREQ, dtype=np.float64)
        top2 = np.sort(l64)[-2:]
        # three f32 roundings of a value below 2^5
        if top2[1] - top2[0] > 3 * 2.0 ** -24 * 32:
            assert toks[b] == int(np.argmax(l64)), b
            checked += 1
        moved += int(np.argmax(l64)) != int(logits[b].float().argmax())
    assert checked >= B - 1 and moved >= 1     # the penalties matter
    # count update: +1 at the returned token, nothing else touched
    expect = seen.clone()
    expect[torch.arange(B), torch.as_tensor(toks)] += 1
    assert torch.equal(dseen.cpu(), expect)


def test_penalties_sampled_interval():
    V, B = 4099, 8
    logits, seen = _penalty_case(V, B)
    params = [(0.7, 50, 0.9, 0.0)] * B
    eps = sr.derive_eps(V)
    refs = [sr.row_reference(
        sr.penalise(logits[b].float().numpy(), seen[b].numpy(), REP, PRES,
                    FREQ), *params[b]) for b in range(B)]
    for u in sr.uniforms(V, B)[:4]:
        dseen = seen.to(DEV)
        toks = _run(logits.to(DEV), params, u, seen=dseen, **_pen_tensors(B))
        sr.check_tokens(toks, refs, u, eps, cap=0)
        expect = seen.clone()
        expect[torch.arange(B), torch.as_tensor(toks)] += 1
        assert torch.equal(dseen.cpu(), expect)


def test_count_saturates():
    V = 1000
    logits = torch.zeros(1, V, dtype=torch.bfloat16)
    logits[0, 17] = 5.0
    seen = torch.zeros(1, V, dtype=torch.int32)
    seen[0, 17] = sr.PROMPT_BIT | sr.COUNT_MASK
    dseen = seen.to(DEV)
    toks = _run(logits.to(DEV), [(0.0, 0, 1.0, 0.0)], [0.0], seen=dseen)
    assert toks[0] == 17 and torch.equal(dseen.cpu(), seen)


@pytest.mark.parametrize("temp", [0.0, 0.8])
def test_degenerate_rows(temp):
    V = 4099
    inf, nan = float("inf"), float("nan")
    rows = torch.randn(5, V, generator=torch.Generator().manual_seed(5))
    rows[0] = nan                                   # -> 0
    rows[1, 2345] = inf                             # -> its index
    rows[1, 3000] = inf                             #    (the first one)
    rows[2] = -inf
    rows[2, 4098] = -3.0                            # -> the only value
    rows[3] = -inf
    rows[3, 77] = nan                               # nan_to_num -> 0 wins
    rows[4, ::2] = nan                              # NaN never wins
    params = [(temp, 50, 0.9, 0.05)] * 5
    for dt in (torch.bfloat16, torch.float32):
        toks = _run(rows.to(dt).to(DEV), params, [0.3] * 5)
        assert toks[:4].tolist() == [0, 2345, 4098, 77]
        assert toks[4] % 2 == 1


def test_reproducible():
    V = 152064
    logits, params, _ = sr.case(V)
    dl = logits.to(DEV)
    u = sr.uniforms(V)[5]
    a = _run(dl, params, u)
    for _ in range(3):
        assert np.array_equal(a, _run(dl, params, u))


def _seeded_uniforms(seeds, steps):
    """What RowSampler draws for seeded rows: per step one
    torch.rand(1, 1) from each row's own device generator."""
    gens = []
    for sd in seeds:
        g = torch.Generator(device=DEV)
        g.manual_seed(sd)
        gens.append(g)
    return np.array([[float(torch.rand(1, 1, device=DEV, generator=g))
                      for g in gens] for _ in range(steps)], np.float32)


def _cfg(p, **pen):
    return DecodingConfig(temperature=p[0], top_k=p[1], top_p=p[2],
                          min_p=p[3], **pen)


def test_agrees_with_sorted_torch_pipeline():
    """f32 logits without ties: the kernel returns what RowSampler's sorted
    torch pipeline (the real ``_sample_torch`` + ``_draw``, fused off)
    returns for the same u, on rows that are not within eps of another
    keep set. Every row is seeded, so the u of each draw is known; u = 0,
    where the pipeline's searchsorted may return a zero-probability token
    0, cannot be requested this way and is covered by the interval test."""
    V = 4099
    logits, params, refs = sr.case(V, dtype="f32")
    assert all(len(torch.unique(r)) == V for r in logits)
    eps = sr.derive_eps(V)
    dl = logits.to(DEV)
    rs = RowSampler(sr.B, device=DEV)
    rs.fused = False
    seeds = [1000 + b for b in range(sr.B)]
    for b, p in enumerate(params):
        rs.set_row(b, _cfg(p), seed=seeds[b])
    compared = 0
    for u in _seeded_uniforms(seeds, 6):
        want = rs.sample(dl).cpu().numpy()
        toks = _run(dl, params, u)
        for b, r in enumerate(refs):
            if "token" in r or r["margin"] <= eps:
                continue
            assert toks[b] == want[b], (b, float(u[b]), toks[b], want[b])
            compared += 1
    assert compared >= 6 * 12


def _row_samplers(V, rows, seeds, prompts, batch=None):
    out = []
    for fused in (True, False):
        rs = RowSampler(batch or len(rows), device=DEV, vocab=V)
        rs.fused = fused
        for b, (p, pen) in enumerate(rows):
            rs.set_row(b, _cfg(p, **pen), seed=seeds[b])
            rs.note_prompt(b, prompts[b])
        out.append(rs)
    return out


PEN = dict(repetition_penalty=REP, presence_penalty=PRES,
           frequency_penalty=FREQ)


def test_row_sampler_fused_matches_torch_path():
    """RowSampler.sample on CUDA logits, fused and with fused off (the
    DNET_FUSED_SAMPLER=0 path: apply_penalties / count_tokens on device):
    seeded and penalised rows over several steps give the same tokens and
    the same history wherever the fp64 reference has one answer."""
    V, steps = 4099, 3
    rows = [((0.7, 50, 0.9, 0.0), PEN), ((0.0, 0, 1.0, 0.0), PEN),
            ((1.0, 0, 1.0, 0.0), {}), ((1.0, 0, 1.0, 0.05), PEN),
            ((0.0, 0, 1.0, 0.0), {}), ((1.3, 0, 0.5, 0.0), PEN)]
    B = len(rows)
    # f32 without ties: the torch path cuts top-k by rank, so it equals
    # the contract's value thresholds only where no tie sits on one
    for seed in range(4242, 4342):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(B, V, generator=g) * 3
        if all(len(torch.unique(r)) == V for r in logits):
            break
    else:
        raise AssertionError("no tie-free logits")
    prompts = [logits[b].float().argsort(descending=True)[:4].tolist()
               + torch.randint(0, V, (30,), generator=g).tolist()
               for b in range(B)]
    seeds = [7 + b if rows[b][0][0] > 0 else None for b in range(B)]
    fus, tor = _row_samplers(V, rows, seeds, prompts)
    big = _row_samplers(V, rows, seeds, prompts, batch=B + 2)[0]
    assert fus.seen is not None and fus.seen.shape == (B, V)
    us = _seeded_uniforms([sd if sd is not None else 0 for sd in seeds],
                          steps)
    dl = logits.to(DEV)
    eps = sr.derive_eps(V)
    wide = 0
    for u in us:
        before = fus.seen.clone().cpu().numpy()
        a = fus.sample(dl).cpu().numpy()
        t = tor.sample(dl).cpu().numpy()
        assert np.array_equal(a, big.sample(dl).cpu().numpy())
        for b, (p, pen) in enumerate(rows):
            l = logits[b].float().numpy()
            if pen:
                l = sr.penalise(l, before[b], REP, PRES, FREQ)
            r = sr.row_reference(l, *p)
            if "token" in r:
                assert a[b] == r["token"] == t[b], b
            elif r["margin"] <= eps:
                continue
            else:
                assert sr.interval_ok(int(a[b]), r, float(u[b]), eps), b
                if sr.near_step(r, float(u[b]), eps):
                    continue
                assert a[b] == t[b], (b, float(u[b]), a[b], t[b])
            wide += 1
            assert torch.equal(fus.seen[b], tor.seen[b]), b
        tor.seen.copy_(fus.seen)       # resync rows with two right answers
    assert wide >= steps * B - 3
    # counted: one per step and row, prompt marks kept
    assert int((fus.seen & sr.COUNT_MASK).sum()) == steps * B
    assert int(((fus.seen & sr.PROMPT_BIT) != 0).sum()) == sum(
        len(set(pr)) for pr, (_, pen) in zip(prompts, rows) if pen)


def test_row_sampler_all_greedy_penalised_batch():
    """No sampled row: the fused path runs for the penalties alone."""
    V, B = 4099, 4
    logits = (torch.randn(B, V, generator=torch.Generator()
                          .manual_seed(9)) * 3).to(torch.bfloat16).to(DEV)
    rows = [((0.0, 0, 1.0, 0.0), PEN)] * B
    prompts = [[1, 2, 3]] * B
    fus, tor = _row_samplers(V, rows, [None] * B, prompts)
    seq = []
    for _ in range(5):
        a, t = fus.sample(logits), tor.sample(logits)
        assert torch.equal(a, t) and torch.equal(fus.seen, tor.seen)
        seq.append(a.cpu())
    seq = torch.stack(seq)                          # [steps, B]
    assert (seq[0] == logits.float().argmax(-1).cpu()).all()
    assert any(len(set(seq[:, b].tolist())) > 1 for b in range(B))


def test_all_filters_off_and_v1():
    """V = 1 and tiny V (shorter than one 16-byte slot, than a wave)."""
    for V in (1, 5, 63, 129):
        logits = (torch.randn(4, V, generator=torch.Generator()
                              .manual_seed(V)) * 3).to(torch.bfloat16)
        params = [(1.0, 0, 1.0, 0.0), (0.0, 0, 1.0, 0.0),
                  (0.7, 3, 0.9, 0.0), (1.3, 0, 0.5, 0.05)]
        refs = [sr.row_reference(logits[b].float().numpy(), *params[b])
                for b in range(4)]
        for uu in (0.0, 0.37, sr.U_MAX):
            u = np.full(4, uu, np.float32)
            sr.check_tokens(_run(logits.to(DEV), params, u), refs, u,
                            sr.derive_eps(V), cap=0)
