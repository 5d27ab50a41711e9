"""Split-k partial slices of the decode GEMM (gemm_m16): split s stores its
[M,N] f32 tile into slice s of the partials buffer and the consumer sums
slices 0..sk-1 in order. Nothing zeroes the buffer and nothing may depend
on what it held before, so every test here poisons it with NaN first: an
element that is read without having been written makes the output NaN.

References and bounds are those of tests/gemm_reference.py. The fused
consumers are driven so that their output IS the GEMM's (RoPE at position
0 rotates by cos 1 / sin 0, the residual is zero), which puts them under
the plain gemm_tol; SwiGLU and the RMSNorm output use that module's
swiglu_tol / rmsnorm_tol the way test_gemm_gpu.py does.

Run as a script it is the child of the empty-splits test: the
DNET_GEMM_SPLITK / DNET_GEMM_NOSTREAM switches are latched per process.
"""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))

import gemm_reference as gr
import dnet_amd.ops as ops

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
DEV = "cuda"

# (fmt, G, K): the smallest shapes that split on their own. N = 72 is one
# full 64-column block plus a block with a single partial wave; int8 G = 64
# at K = 1088 ends on a short last tile.
FORMATS = [("int8", 128, 1280), ("int4", 128, 1280), ("int8", 64, 1088)]
MS = [3, 17, 64]                    # MT tiers 1, 2, 4, each with a row tail
N = 72
HQ, HKV, D = 5, 2, 8                # (HQ + 2 HKV) * D == N


def _dev():
    return torch.device(DEV, 0)


def _poison():
    ops._get_partials(_dev()).fill_(float("nan"))


def _report(name, ratio):
    print(f"[err/tol] {name}: {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err/tol = {ratio:.3f} > 1"


def _case(fmt, g, k, m, bias=False):
    seed = 6000 + 7 * m + k + g + (1 if fmt == "int4" else 0) + 3 * bias
    return dict(gr._case(fmt, m, N, k, g, bias), seed=seed)


@functools.lru_cache(maxsize=None)
def _built(fmt, g, k, m, bias=False):
    """(case, x, w, bias, ref64, mag), computed once and never modified."""
    c = _case(fmt, g, k, m, bias)
    x, w, b = gr.build_case(c)
    r64, mag = gr.case_reference(c, x, w, b, DEV)
    return c, x, w, b, r64, mag


def _assert_splits(c):
    assert ops._will_defer(c["M"], c["N"], c["K"], c["G"], gr.BITS[c["fmt"]],
                           ops._get_partials(_dev()).numel()), \
        f"{gr.case_id(c)} no longer splits K"


def _wargs(c, w):
    return (w["packed"].to(DEV), w["scales"].to(DEV), c["G"],
            gr.BITS[c["fmt"]])


def _scratch_is_zero():
    assert int(ops._get_scratch(_dev()).count_nonzero()) == 0, \
        "the legacy scratch was written"


CASES = [(f, g, k, m) for f, g, k in FORMATS for m in MS]
IDS = [f"{f}-G{g}-K{k}-M{m}" for f, g, k, m in CASES]


# ------------------------------------------------------- 1. poisoned buffer

@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("fmt,g,k,m", CASES, ids=IDS)
def test_poisoned_plain_gemm(fmt, g, k, m, bias):
    c, x, w, b, r64, mag = _built(fmt, g, k, m, bias)
    _assert_splits(c)
    _poison()
    got = gr.gemm_call(w, x, b, DEV)
    _report("plain " + gr.case_id(c),
            gr.ratio(got, r64, gr.gemm_tol(r64, mag, k)))
    _scratch_is_zero()


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("fmt,g,k,m", CASES, ids=IDS)
def test_poisoned_qkv_rope(fmt, g, k, m, use_bias):
    """Position 0 rotates by (cos 1, sin 0): q and the appended k / v rows
    are bf16(GEMM + bias) themselves."""
    c, x, w, b, r64, mag = _built(fmt, g, k, m, use_bias)
    _assert_splits(c)
    smax = 4
    cos, sin = ops.rope_tables(smax, D, 1e6, _dev())
    pos = torch.zeros(m, dtype=torch.int32, device=DEV)
    kc = torch.full((m, HKV, smax, D), 9.0, dtype=BF16, device=DEV)
    vc = torch.full((m, HKV, smax, D), 9.0, dtype=BF16, device=DEV)
    _poison()
    wp, sc, grp, bits = _wargs(c, w)
    q = ops.gemv_qkv_rope(x.to(DEV), wp, sc, grp, bits,
                          None if b is None else b.to(DEV), HQ, HKV, D, kc,
                          vc, pos, cos, sin)
    got = torch.cat([q.reshape(m, HQ * D), kc[:, :, 0].reshape(m, HKV * D),
                     vc[:, :, 0].reshape(m, HKV * D)], dim=1)
    _report("qkv_rope " + gr.case_id(c),
            gr.ratio(got, r64, gr.gemm_tol(r64, mag, k)))
    assert bool((kc[:, :, 1:] == 9.0).all()) and bool((vc[:, :, 1:] == 9.0).all())
    _scratch_is_zero()


def _check_norm(name, c, k, rd, y, r64, mag, wn, eps):
    """Zero residual: the updated residual is bf16(GEMM); y as in
    test_gemm_gpu.py::test_gemv_rmsnorm_vs_fp64."""
    _report(name + " residual", gr.ratio(rd, r64, gr.gemm_tol(r64, mag, k)))
    dh = gr.gemm_acc(mag, k) + 2.0 ** -8 * r64.abs() + 2.0 ** -8 * r64.abs()
    y64, rms = gr.rmsnorm_ref(r64, wn, eps)
    _report(name + " y", gr.ratio(y, y64,
                                  gr.rmsnorm_tol(y64, r64, rms, wn, dh)))


@pytest.mark.parametrize("fmt,g,k,m", CASES, ids=IDS)
def test_poisoned_gemv_rmsnorm(fmt, g, k, m):
    c, x, w, _, r64, mag = _built(fmt, g, k, m)
    _assert_splits(c)
    wn = torch.randn(N, generator=torch.Generator().manual_seed(c["seed"] + 1)
                     ).to(BF16)
    rd = torch.zeros(m, N, dtype=BF16, device=DEV)
    _poison()
    y = ops.gemv_rmsnorm(x.to(DEV), *_wargs(c, w), rd, wn.to(DEV), 1e-6)
    _check_norm("gemv_rmsnorm " + gr.case_id(c), c, k, rd, y, r64, mag, wn,
                1e-6)
    _scratch_is_zero()


@pytest.mark.parametrize("fmt,g,k,m", CASES, ids=IDS)
def test_poisoned_gemv_swiglu(fmt, g, k, m):
    c, x, w, _, r64, mag = _built(fmt, g, k, m)
    _assert_splits(c)
    i = N // 2
    acc = gr.gemm_acc(mag, k)
    gg, uu = r64[:, :i], r64[:, i:]
    y64, silu = gr.swiglu_ref(gg, uu)
    tol = gr.swiglu_tol(y64, uu, silu, acc[:, :i], acc[:, i:])
    _poison()
    y = ops.gemv_swiglu(x.to(DEV), *_wargs(c, w))
    _report("gemv_swiglu " + gr.case_id(c), gr.ratio(y, y64, tol))
    _scratch_is_zero()


@pytest.mark.parametrize("fmt,g,k,m", CASES, ids=IDS)
def test_poisoned_gemv_defer_consumers(fmt, g, k, m):
    """gemv_defer, then each consumer of a deferred projection, with the
    slice count handed over explicitly and through the default."""
    c, x, w, _, r64, mag = _built(fmt, g, k, m)
    _assert_splits(c)
    wn = torch.randn(N, generator=torch.Generator().manual_seed(c["seed"] + 1)
                     ).to(BF16)
    xd, wa = x.to(DEV), _wargs(c, w)
    for explicit in (True, False):
        _poison()
        sk = ops.gemv_defer(xd, *wa)
        assert sk > 1
        rd = torch.zeros(m, N, dtype=BF16, device=DEV)
        y = ops.rmsnorm_f32_scratch(rd, wn.to(DEV), 1e-6,
                                    sk if explicit else None)
        _check_norm(f"defer+rmsnorm {gr.case_id(c)} explicit={explicit}", c,
                    k, rd, y, r64, mag, wn, 1e-6)
        # the slices are only read: a second consumer sees them unchanged
        h = torch.zeros(m, N, dtype=BF16, device=DEV)
        if explicit:
            ops.resid_add_scratch(h, sk)
        else:
            ops.resid_add_scratch(h)
        _report(f"defer+resid_add {gr.case_id(c)} explicit={explicit}",
                gr.ratio(h, r64, gr.gemm_tol(r64, mag, k)))
    _scratch_is_zero()


def test_rmsnorm_wide_row_same_bits_as_one_slice():
    """H = 5120 is 640 8-element vectors: the slice-summing RMSNorm runs
    three 256-thread groups (the last half empty) and promises the bits of
    the one-group kernel. Sum the slices on the host in the same order,
    hand that single buffer to the legacy one-slice mode, and compare."""
    m, n, k = 3, 5120, 1280
    c = dict(gr._case("int8", m, n, k, 128), seed=6400)
    _assert_splits(c)
    x, w, _ = gr.build_case(c)
    r64, mag = gr.case_reference(c, x, w, None, DEV)
    gen = torch.Generator().manual_seed(c["seed"] + 1)
    wn = torch.randn(n, generator=gen).to(BF16).to(DEV)
    res = torch.randn(m, n, generator=gen).to(BF16)
    _poison()
    sk = ops.gemv_defer(x.to(DEV), *_wargs(c, w))
    part = ops._get_partials(_dev())[:sk * m * n].view(sk, m, n)
    total = part[0].clone()
    for s in range(1, sk):
        total += part[s]
    rd = res.clone().to(DEV)
    y = ops.rmsnorm_f32_scratch(rd, wn, 1e-6, sk)
    scratch = ops._get_scratch(_dev())
    rd1, y1 = res.clone().to(DEV), torch.empty(m, n, dtype=BF16, device=DEV)
    try:
        scratch[:m * n] = total.reshape(-1)
        ops._native().rmsnorm_f32(scratch, rd1, wn, y1, 1e-6)
        _scratch_is_zero()
    finally:
        scratch.zero_()
    assert torch.equal(rd, rd1) and torch.equal(y, y1)
    h64 = res.to(F64) + r64
    dh = gr.gemm_acc(mag, k) + 2.0 ** -8 * r64.abs() + 2.0 ** -8 * h64.abs()
    _report("wide rmsnorm residual", gr.ratio(rd, h64, dh))
    y64, rms = gr.rmsnorm_ref(h64, wn, 1e-6)
    _report("wide rmsnorm y",
            gr.ratio(y, y64, gr.rmsnorm_tol(y64, h64, rms, wn, dh)))


# ---------------------------------------------------------- 2. empty splits

# DNET_GEMM_SPLITK=8. int4 K = 640 has 5 quads for 8 splits: splits 0-6
# have no work and must store zeros. int8 K = 576: one pair per split (two
# in the last).
EMPTY_CASES = [dict(gr._case("int4", 17, N, 640, 128), seed=6500),
               dict(gr._case("int8", 17, N, 576, 64), seed=6501)]


def main_child() -> int:
    for c in EMPTY_CASES:
        x, w, b = gr.build_case(c)
        r64, mag = gr.case_reference(c, x, w, b, DEV)
        tol = gr.gemm_tol(r64, mag, c["K"])
        split = bool(gr.splits_k(c))
        _poison()
        plain = gr.ratio(gr.gemm_call(w, x, b, DEV), r64, tol)
        _poison()
        sk = ops.gemv_defer(x.to(DEV), *_wargs(c, w)) if split else 0
        h = torch.zeros(c["M"], N, dtype=BF16, device=DEV)
        if split:
            ops.resid_add_scratch(h, sk)
        print(json.dumps({"case": gr.case_id(c), "split": split, "sk": sk,
                          "plain": plain, "deferred": gr.ratio(h, r64, tol)}),
              flush=True)
    torch.cuda.synchronize()
    return 0


_CHILD_DIED = []


@pytest.fixture(autouse=True)
def _no_gpu_work_after_a_dead_child():
    """A child that died on a signal or ran into its time limit may have
    faulted the GPU: start nothing more on it from this module."""
    if _CHILD_DIED:
        pytest.fail(f"not started: child {_CHILD_DIED[0]} died earlier")


def _run_child(extra):
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("DNET_GEMM_")}
    env["DNET_GEMM_SPLITK"] = "8"
    env.update(extra)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__),
                            "--child"], env=env, timeout=120,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(str(extra))
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _CHILD_DIED.append(str(extra))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:],
                               r.stderr[-2000:])
    recs = [json.loads(ln) for ln in r.stdout.splitlines()
            if ln.startswith("{")]
    assert len(recs) == len(EMPTY_CASES)
    for x in recs:
        print(f"[err/tol] splitk=8 {extra} {x['case']}: plain "
              f"{x['plain']:.3f} deferred {x['deferred']:.3f}")
        assert x["split"] and x["sk"] == 8, x
        assert x["plain"] <= 1.0 and x["deferred"] <= 1.0, x
    return recs


@pytest.mark.parametrize("extra", [{}, {"DNET_GEMM_NOSTREAM": "1"}],
                         ids=["streamed", "nostream"])
def test_empty_splits_in_child(extra):
    assert not [k for k in os.environ if k.startswith("DNET_GEMM_")], \
        "the parent must run the default kernels"
    _run_child(extra)


# ----------------------------------------------------------- 3. determinism

@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_four_launches_same_bits(exact):
    c, x, w, b, r64, mag = _built("int8", 128, 1280, 17)
    _assert_splits(c)
    ops.set_reproducible(exact)
    try:
        _poison()
        outs = [gr.gemm_call(w, x, b, DEV) for _ in range(4)]
    finally:
        ops.set_reproducible(False)
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    # exact mode: + 32 splits x 2^-17 grid rounding, as test_gemm_gpu.py
    _report(f"determinism exact={exact}",
            gr.ratio(outs[0], r64, gr.gemm_tol(r64, mag, c["K"],
                                               2.0 ** -12 if exact else 0.0)))


# ------------------------------------------------------ 4. large then small

def test_large_then_small_then_larger():
    """The three hygiene cases in order on a buffer that is poisoned once
    and never cleaned: each launch overwrites all it later reads."""
    _poison()
    for i, c in enumerate(gr.HYGIENE_CASES):
        assert gr.splits_k(c), gr.case_id(c)
        r, _ = gr.run_case(c, DEV)
        _report(f"slices hygiene {i} {gr.case_id(c)}", r)
    _scratch_is_zero()


if __name__ == "__main__":
    if "--child" in sys.argv[1:]:
        sys.exit(main_child())
    sys.exit("usage: test_gemm_slices_gpu.py --child")
