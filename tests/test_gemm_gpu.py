"""Decode GEMMs (gemm_m16, scalar gemv, dequant) and their elementwise and
deferred-combine consumers against fp64 references
(tests/gemm_reference.py) with derived bounds.

Every checker takes a ``device``: "cuda" runs the HIP kernels (marked
``gpu``), "cpu" runs dnet_amd.ops' fp32 reference path through the same
inputs, reference and bound. Each case prints its worst err/tol ratio
(1.0 is the limit).

Two int8 weight contracts exist and each path is held to its own: the
MFMA kernels, dequant_* and the CPU path multiply by bf16(q*s); the scalar
gemv_int8 kernel (GPU, M <= 2 or unpacked weights) multiplies by the
unrounded q*s.
"""
import functools
import itertools
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import gemm_reference as gr
import dnet_amd.ops as ops

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
CUDA_ONLY = [pytest.param("cuda", marks=pytest.mark.gpu)]
BF16 = torch.bfloat16
F64 = torch.float64


def _report(name, ratio):
    print(f"[err/tol] {name}: {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err/tol = {ratio:.3f} > 1"


# ------------------------------------------------- A. exact one-hot sweep

ONEHOT_CASES = gr.onehot_cases()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", ONEHOT_CASES, ids=gr.case_id)
def test_onehot_sweep_is_exact(case, device):
    """x = rows of I_K: every k of every row of W comes back as
    bf16(w_contract[n, k]), exactly, and the zero padding rows as zeros."""
    bad, got = gr.run_onehot(case, device)
    print(f"[err/tol] onehot {gr.case_id(case)}: "
          f"{'0.000' if bad == 0 else 'inf'} ({bad} of {got.numel()} differ)")
    assert bad == 0, f"{bad} of {got.numel()} elements differ"


@pytest.mark.parametrize("device", CUDA_ONLY)
def test_onehot_sweep_reaches_split_k(device):
    """The sweep proves less than it claims unless some swept shape of
    each format really splits K (and some does not)."""
    for fmt in ("bf16", "int8", "int4"):
        cs = [c for c in ONEHOT_CASES if c["fmt"] == fmt and gr.via_gemm_m16(c)]
        split = [gr.case_id(c) for c in cs if gr.splits_k(c)]
        print(f"[onehot] {fmt}: {len(split)} of {len(cs)} shapes split K")
        assert split, fmt
        assert len(split) < len(cs), fmt
    # the case the issue names: 17 pairs -> sk = 4 with a 5-pair last split
    scratch = ops._get_scratch(torch.device(device, 0)).numel()
    assert ops._will_defer(16, 72, 1088, 64, 8, scratch)
    assert ops._will_defer(16, 72, 1280, 128, 8, scratch)
    assert ops._will_defer(16, 72, 1280, 128, 4, scratch)


# ------------------------------------------------ B. random-data matrix

MATRIX_CASES = gr.matrix_cases()


def test_gemm_case_matrix_covers_the_axes():
    """Every pair of axis values that some valid row can hold is held by a
    chosen row; about 150 cases with the fixed ones."""
    cs = MATRIX_CASES
    assert 90 <= len(cs) <= 150, len(cs)
    keys, vals = gr.MAT_KEYS, gr.MAT_AXES
    valid = [r for r in itertools.product(*vals) if gr.matrix_row_valid(*r)]
    for i, j in itertools.combinations(range(len(keys)), 2):
        if "G" in (keys[i], keys[j]):
            feasible = {(r[i], r[j]) for r in valid if r[0] != "bf16"}
        else:
            feasible = {(r[i], r[j]) for r in valid}
        for a, b in feasible:
            assert any(c[keys[i]] == a and c[keys[j]] == b for c in cs), \
                (keys[i], a, keys[j], b)
    # nothing was forced out by a DNET_CHECK: the smallest N and K are in
    assert any(c["N"] == 8 for c in cs) and any(c["K"] == 64 for c in cs)
    assert sum(bool(c.get("quantizer")) for c in cs) == 2
    assert len({c["seed"] for c in cs}) == len(cs)
    total = (len(cs) + len(gr.scalar_bf16_cases())
             + len(gr.scalar_int8_cases()))
    assert total <= 200, total


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", MATRIX_CASES, ids=gr.case_id)
def test_gemm_matrix(case, device):
    r, got = gr.run_case(case, device)
    assert got.shape == (case["M"], case["N"]) and got.dtype == BF16
    _report(gr.case_id(case), r)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", gr.scalar_bf16_cases(), ids=gr.case_id)
def test_scalar_gemv_bf16(case, device):
    """K % 64 != 0 is the only way into the scalar gemv_bf16 kernel."""
    assert case["K"] % 64 and not gr.via_gemm_m16(case)
    r, _ = gr.run_case(case, device)
    _report("scalar " + gr.case_id(case), r)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", gr.scalar_int8_cases(), ids=gr.case_id)
def test_scalar_gemv_int8_unpacked(case, device):
    """Unpacked int8 runs the scalar kernel at every M; on the GPU it is
    held to the exact q*s contract, on the CPU to bf16(q*s)."""
    assert gr.exact_contract(case, device) == (device != "cpu")
    r, _ = gr.run_case(case, device)
    _report("scalar " + gr.case_id(case), r)


@pytest.mark.parametrize("device", DEVICES)
def test_combine_grid_stride_with_bias(device):
    """M * N > 2048 * 256: the f32 -> bf16 combine kernel loops."""
    c = gr.GRID_STRIDE_CASE
    assert c["M"] * c["N"] > 2048 * 256
    if device != "cpu":
        assert gr.splits_k(c), "shape no longer splits K"
    r, _ = gr.run_case(c, device)
    _report("grid-stride " + gr.case_id(c), r)


@pytest.mark.parametrize("device", DEVICES)
def test_scratch_hygiene_across_sizes(device):
    """Large plain split-k GEMM, then a small one, then a larger one: the
    stale partials beyond the small one's M*N must not reach the third."""
    for i, c in enumerate(gr.HYGIENE_CASES):
        if device != "cpu":
            assert gr.splits_k(c), gr.case_id(c)
        r, _ = gr.run_case(c, device)
        _report(f"hygiene {i} {gr.case_id(c)}", r)


@pytest.fixture
def reproducible_mode():
    ops.set_reproducible(True)
    try:
        yield
    finally:
        ops.set_reproducible(False)


def _repro_cases():
    cs = []
    for k in (576, 1088, 2048):
        cs.append(next(c for c in MATRIX_CASES if c["K"] == k
                       and c["fmt"] != "bf16" and 3 <= c["M"] <= 64
                       and not c.get("quantizer")))
    return cs


@pytest.mark.parametrize("device", CUDA_ONLY)
@pytest.mark.parametrize("case", _repro_cases(), ids=gr.case_id)
def test_reproducible_mode(case, device, reproducible_mode):
    """Four launches give the same bits, within tol + 2^-12 (32 splits x
    2^-17 grid rounding). The mode is order-independent while sums stay
    below 2^8, which these outputs do."""
    assert gr.splits_k(case), "shape no longer splits K"
    x, w, bias = gr.build_case(case)
    r64, mag = gr.case_reference(case, x, w, bias, device)
    assert float(r64.abs().max()) < 2.0 ** 8
    outs = [gr.gemm_call(w, x, bias, device) for _ in range(4)]
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    _report("reproducible " + gr.case_id(case),
            gr.ratio(outs[0], r64, gr.gemm_tol(r64, mag, case["K"],
                                               2.0 ** -12)))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n,k", [(5, 64), (33, 320), (256, 1088)])
@pytest.mark.parametrize("kind", ["int8", "int8-packed", "int4"])
def test_dequant_exact(kind, n, k, device):
    """dequant_* equals bf16(q*s) exactly on full-range codes. int4 needs
    K % 128 == 0 (a DNET_CHECK), so its K is rounded up to 128, 384, 1152."""
    gen = torch.Generator().manual_seed(n + k)
    if kind == "int4":
        k = -(-k // 128) * 128
        w = gr.make_weights("int4", n, k, 128, gen)
        wt = w["packed"] if device != "cpu" else w["plain"]
        got = ops.dequant_int4(wt.to(device), w["scales"].to(device), 128)
    else:
        packed = kind == "int8-packed"
        w = gr.make_weights("int8", n, k, 64, gen)
        got = ops.dequant_int8(w["packed" if packed else "plain"].to(device),
                               w["scales"].to(device), 64, packed=packed)
    assert int(w["codes"].min()) == (-8 if kind == "int4" else -128)
    want = gr.contract_weights(w).to(BF16)
    assert got.shape == want.shape
    assert torch.equal(got.cpu().float(), want.float())


# ------------------------------------- C. variants latched per process

@functools.lru_cache(maxsize=None)
def _parent_records():
    return {r["case"]: r for r in gr.run_variant_cases("cuda")}


_CHILD_DIED = []        # children that ended on a signal or a timeout


@pytest.fixture(autouse=True)
def _no_gpu_work_after_a_dead_child(request):
    """A child that died on a signal or ran into its time limit may have
    faulted the GPU: start nothing more on it from this module."""
    if _CHILD_DIED and "gpu" in request.keywords:
        pytest.fail(f"not started: child {_CHILD_DIED[0]} died earlier")


def _run_child(var):
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("DNET_GEMM_")}
    env[var.split("=")[0]] = var.split("=")[1]
    t0 = time.time()
    try:
        r = subprocess.run(
            [sys.executable, os.path.abspath(gr.__file__), "--variant-cases"],
            env=env, timeout=300, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(var)
        raise
    print(f"[{var} child] {time.time() - t0:.1f} s of 300 s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _CHILD_DIED.append(var)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-2000:])
    recs = [json.loads(ln) for ln in r.stdout.splitlines()
            if ln.startswith("{")]
    assert len(recs) == len(gr.variant_cases())
    for kind in ("onehot", "matrix"):
        worst = max((x for x in recs if x["case"].startswith(kind)),
                    key=lambda x: x["ratio"])
        print(f"[err/tol] {var} {kind} worst: {worst['ratio']:.3f} "
              f"({worst['case']})")
    bad = [x for x in recs if not x["ratio"] <= 1.0]
    assert not bad, bad
    return recs


def _no_gemm_env():
    assert not [k for k in os.environ if k.startswith("DNET_GEMM_")], \
        "the parent must run the default kernels"


@pytest.mark.parametrize("device", CUDA_ONLY)
def test_variant_nostream_in_child(device):
    """DNET_GEMM_NOSTREAM=1: the generic kernel at G = 64/128, production's
    fallback for misaligned splits. Where K is not split it must give the
    streamed kernel's bits (same products, same order); with split-k the
    atomics reorder, so only the bound is claimed."""
    _no_gemm_env()
    recs = _run_child("DNET_GEMM_NOSTREAM=1")
    parent = _parent_records()
    same = diff = 0
    for x in recs:
        p = parent[x["case"]]
        assert x["split"] == p["split"], x["case"]
        if not x["split"]:
            assert x["checksum"] == p["checksum"], x["case"]
            same += 1
        else:
            diff += x["checksum"] != p["checksum"]
    print(f"[nostream] {same} unsplit cases bit-identical to the streamed "
          f"kernel; {diff} split cases differ in bits")
    assert same > 50


@pytest.mark.parametrize("device", CUDA_ONLY)
def test_variant_noglds_in_child(device):
    """DNET_GEMM_NOGLDS=1: activations staged by plain loads + ds_write
    instead of the global->LDS DMA; same swizzled image."""
    _no_gemm_env()
    _run_child("DNET_GEMM_NOGLDS=1")


@pytest.mark.parametrize("device", CUDA_ONLY)
def test_variant_forced_splitk_in_child(device):
    """DNET_GEMM_SPLITK=8: K = 576 gives one pair per split and a 2-pair
    last split; int8 K = 640 at G = 128 (576 is no multiple of 128) gives
    misaligned split starts, so production's generic fallback runs; int4
    K = 640 has 5 quads for 8 splits, so the last split does everything;
    K < 512 stays at one split."""
    _no_gemm_env()
    recs = _run_child("DNET_GEMM_SPLITK=8")
    parent = _parent_records()
    forced = [x["case"] for x in recs
              if x["split"] and not parent[x["case"]]["split"]]
    print(f"[splitk=8] {len(forced)} cases split only when forced")
    # K = 576 splits in two on its own; here it must split (in eight)
    k576 = [x for x in recs if "-K576-G64" in x["case"]]
    assert k576 and all(x["split"] for x in k576)
    assert any("int8" in c and "-K640-G128" in c for c in forced)
    assert any("int4" in c and "-K640-" in c for c in forced)
    assert not [x for x in recs if x["split"] and "-K384-" in x["case"]]


# ------------------------------- D. elementwise and deferred consumers

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("t,h", [(1, 8), (33, 1024), (2049, 8), (9, 5120)])
def test_rmsnorm_vs_fp64(t, h, with_res, device):
    gen = torch.Generator().manual_seed(t + h + with_res)
    x = torch.randn(t, h, generator=gen).to(BF16)
    res = torch.randn(t, h, generator=gen).to(BF16) if with_res else None
    wn = torch.randn(h, generator=gen).to(BF16)
    eps = 1e-6
    h64 = x.to(F64) + (res.to(F64) if with_res else 0.0)
    y64, rms = gr.rmsnorm_ref(h64, wn, eps)
    rd = None if res is None else res.clone().to(device)
    y = ops.rmsnorm(x.to(device), rd, wn.to(device), eps)
    dh = None
    if with_res:        # the kernel normalizes the bf16-rounded sum
        dh = 2.0 ** -8 * h64.abs()
        _report(f"rmsnorm residual T{t} H{h}", gr.ratio(rd, h64, dh))
    _report(f"rmsnorm y T{t} H{h} res={with_res}",
            gr.ratio(y, y64, gr.rmsnorm_tol(y64, h64, rms, wn, dh)))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("t,i", [(1, 8), (17, 1024), (33, 131072)])
def test_swiglu_vs_fp64(t, i, device):
    gen = torch.Generator().manual_seed(t + i)
    gu = torch.randn(t, 2 * i, generator=gen).to(BF16)
    y64, _ = gr.swiglu_ref(gu[:, :i].to(F64), gu[:, i:].to(F64))
    y = ops.swiglu(gu.to(device))
    _report(f"swiglu T{t} I{i}", gr.ratio(y, y64, gr.swiglu_tol(y64)))


def _scratch():
    return ops._get_scratch(torch.device("cuda", 0))


FUSED_SHAPES = [(3, True), (16, True), (64, True), (3, False), (16, False),
                (64, False)]            # (M, K splits)


def _fused_setup(fmt, m, defer, n, device, seed):
    """x, weights and the fp64 GEMM (ref, acc) for a consumer test. K =
    1024 splits four ways at these N; K = 256 has too few pairs to split."""
    k = 1024 if defer else 256
    c = dict(gr._case(fmt, m, n, k, 128), seed=seed)
    if device != "cpu":
        assert gr.splits_k(c) == defer, gr.case_id(c)
    x, w, _ = gr.build_case(c)
    r64, mag = gr.gemm_ref(x, gr.contract_weights(w))
    return c, x, w, r64, gr.gemm_acc(mag, k)


def _mid_round(device, defer):
    """The CPU path and the unsplit branch round the GEMM output to bf16
    before the consumer; the fused branch reads the f32 scratch."""
    return device == "cpu" or not defer


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("m,defer", FUSED_SHAPES)
@pytest.mark.parametrize("fmt", ["int8", "int4"])
def test_gemv_swiglu_vs_fp64(fmt, m, defer, device):
    i = 512
    c, x, w, r64, acc = _fused_setup(fmt, m, defer, 2 * i, device,
                                     5000 + m + defer)
    g, u, dg, du = r64[:, :i], r64[:, i:], acc[:, :i], acc[:, i:]
    if _mid_round(device, defer):
        dg, du = dg + 2.0 ** -8 * g.abs(), du + 2.0 ** -8 * u.abs()
    y64, silu = gr.swiglu_ref(g, u)
    tol = gr.swiglu_tol(y64, u, silu, dg, du)
    if device == "cpu":
        y = ops.swiglu(gr.gemm_call(w, x, None, device))
    else:
        try:
            y = ops.gemv_swiglu(x.to(device), w["packed"].to(device),
                                w["scales"].to(device), 128, gr.BITS[fmt])
            assert int(_scratch().count_nonzero()) == 0, "scratch not zero"
        finally:
            _scratch().zero_()
    _report(f"gemv_swiglu {gr.case_id(c)} defer={defer}",
            gr.ratio(y, y64, tol))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("m,defer", FUSED_SHAPES)
@pytest.mark.parametrize("fmt", ["int8", "int4"])
def test_gemv_rmsnorm_vs_fp64(fmt, m, defer, device):
    n, eps = 1024, 1e-6
    c, x, w, proj, acc = _fused_setup(fmt, m, defer, n, device,
                                      5100 + m + defer)
    gen = torch.Generator().manual_seed(c["seed"] + 1)
    res = torch.randn(m, n, generator=gen).to(BF16)
    wn = torch.randn(n, generator=gen).to(BF16)
    h64 = res.to(F64) + proj
    # the projection is rounded to bf16 (by the norm kernel when it reads
    # the scratch, by the GEMM otherwise), then h = res + proj is
    dh = acc + 2.0 ** -8 * proj.abs() + 2.0 ** -8 * h64.abs()
    y64, rms = gr.rmsnorm_ref(h64, wn, eps)
    rd = res.clone().to(device)
    if device == "cpu":
        y = ops.rmsnorm(gr.gemm_call(w, x, None, device), rd, wn, eps)
    else:
        try:
            y = ops.gemv_rmsnorm(x.to(device), w["packed"].to(device),
                                 w["scales"].to(device), 128, gr.BITS[fmt],
                                 rd, wn.to(device), eps)
            assert int(_scratch().count_nonzero()) == 0, "scratch not zero"
        finally:
            _scratch().zero_()
    name = f"gemv_rmsnorm {gr.case_id(c)} defer={defer}"
    _report(name + " residual", gr.ratio(rd, h64, dh))
    _report(name + " y", gr.ratio(y, y64,
                                  gr.rmsnorm_tol(y64, h64, rms, wn, dh)))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("m", [3, 16, 64])
@pytest.mark.parametrize("fmt", ["int8", "int4"])
def test_resid_add_scratch_vs_fp64(fmt, m, device):
    """gemv_defer + resid_add_scratch: h += projection straight from the
    f32 scratch (GPU); the CPU path adds the bf16 GEMM output."""
    n = 1024
    c, x, w, proj, acc = _fused_setup(fmt, m, True, n, device, 5200 + m)
    gen = torch.Generator().manual_seed(c["seed"] + 1)
    h = torch.randn(m, n, generator=gen).to(BF16)
    h64 = h.to(F64) + proj
    tol = 2.0 ** -8 * h64.abs() + acc
    hd = h.clone().to(device)
    if device == "cpu":
        tol = tol + 2.0 ** -8 * proj.abs()
        hd.add_(gr.gemm_call(w, x, None, device))
    else:
        try:
            assert ops.gemv_defer(x.to(device), w["packed"].to(device),
                                  w["scales"].to(device), 128, gr.BITS[fmt])
            ops.resid_add_scratch(hd)
            assert int(_scratch().count_nonzero()) == 0, "scratch not zero"
        finally:
            _scratch().zero_()
    _report(f"resid_add {gr.case_id(c)}", gr.ratio(hd, h64, tol))


# ------------------------------------------- E. reference sensitivity

def test_bound_rejects_wrong_references():
    """The bound bites: against a reference that reads the next group's
    scale, drops the last 64-k pair, or omits the bias, the (correct) CPU
    path fails every matrix case the mutation applies to."""
    counts = {}
    for c in MATRIX_CASES:
        x, w, bias = gr.build_case(c)
        got = gr.gemm_call(w, x, bias, "cpu")
        muts = ["pair"]
        if c["fmt"] != "bf16" and c["K"] // c["G"] >= 2 \
                and not c.get("quantizer"):
            muts.append("scale")
        if c["bias"]:
            muts.append("bias")
        for mut in [""] + muts:
            r64, mag = gr.case_reference(c, x, w, bias, "cpu", mut)
            r = gr.ratio(got, r64, gr.gemm_tol(r64, mag, c["K"]))
            if mut == "":
                assert r <= 1.0, (gr.case_id(c), r)
                continue
            n, worst = counts.get(mut, (0, float("inf")))
            counts[mut] = (n + 1, min(worst, r))
            assert r > 1.0, (gr.case_id(c), mut, r)
    for mut, (n, worst) in counts.items():
        print(f"[sensitivity] wrong-{mut} reference: {n} cases red, "
              f"smallest err/tol {worst:.1f}")
    assert set(counts) == {"pair", "scale", "bias"}
