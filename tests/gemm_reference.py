"""fp64 references and derived error bounds for the decode GEMM family
(gemm_m16, the scalar gemv kernels, dequant) and for the elementwise and
deferred-combine consumers (helper for tests/test_gemm_gpu.py; not a test
module).

Inputs are generated on the CPU from a per-case seed, so every process
sees the same bits. Quantized weights are built directly: codes uniform
over the full range and group scales 2^u (u real, rounded to bf16, so they
carry 8 significant bits and q*s is not exact in bf16) spread over 16x, so
a wrong scale index or a wrong k is an O(1) error.

Run as a script it replays the quantized gemm_m16 cases in a fresh
process (``python tests/gemm_reference.py --variant-cases``): the
DNET_GEMM_NOSTREAM / NOGLDS / SPLITK switches are latched per process.
"""
from __future__ import annotations

import functools
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

F64 = torch.float64
BF16 = torch.bfloat16
BITS = {"bf16": 16, "int8": 8, "int4": 4}


# ------------------------------------------------------------------ weights

def hostile_scales(n: int, groups: int, gen) -> torch.Tensor:
    """Per-(row, group) scales 2^u, u uniform in [-9, -5], rounded to bf16:
    neighbouring groups differ by up to 16x."""
    u = torch.rand(n, groups, generator=gen) * 4.0 - 9.0
    return torch.pow(2.0, u).to(BF16)


def make_weights(fmt: str, n: int, k: int, g: int, gen,
                 quantizer: bool = False) -> dict:
    """One weight matrix in every layout the entry points take.

    codes   int8 [N, K] integer values (int4: nibble - 8, in [-8, 7])
    scales  bf16 [N, K/G]
    plain   row-major storage (int8 codes / int4 nibble bytes / bf16)
    packed  MFMA layout (pack_int8_mfma / pack_int4_mfma); bf16: plain
    ``quantizer`` runs the production quantize_int8/int4 on randn/30
    instead of drawing codes and scales directly."""
    from dnet_amd.ops import reference as ref
    w = dict(fmt=fmt, N=n, K=k, G=g, codes=None, scales=None)
    if fmt == "bf16":
        w["plain"] = w["packed"] = (
            torch.randn(n, k, generator=gen) / 8).to(BF16)
        return w
    if quantizer:
        wf = (torch.randn(n, k, generator=gen) / 30).to(BF16)
        if fmt == "int8":
            plain, scales = ref.quantize_int8(wf, g)
            codes = plain
        else:
            plain, scales = ref.quantize_int4(wf, g)
            codes = ref.unpack_int4(plain)
    else:
        scales = hostile_scales(n, k // g, gen)
        if fmt == "int8":
            codes = torch.randint(-128, 128, (n, k), generator=gen,
                                  dtype=torch.int16).to(torch.int8)
            plain = codes
        else:
            nib = torch.randint(0, 16, (n, k), generator=gen,
                                dtype=torch.int16).to(torch.uint8)
            codes = nib.to(torch.int8) - 8
            plain = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    w["codes"], w["scales"], w["plain"] = codes, scales, plain
    if fmt == "int4":
        w["packed"] = ref.pack_int4_mfma(plain)
    else:       # the packed layout needs whole 64-k pairs
        w["packed"] = ref.pack_int8_mfma(plain) if k % 64 == 0 else None
    return w


def contract_weights(w: dict, exact: bool = False,
                     scale_shift: int = 0) -> torch.Tensor:
    """The weights a path promises to multiply by, as fp64 [N, K].

    bf16(q*s) for gemm_m16, dequant_* and the CPU path; the exact product
    q*s (``exact``) for the scalar gemv_int8 kernel; the bf16 value itself
    for bf16 weights. ``scale_shift`` reads group g+shift's scale instead
    (a deliberately wrong reference for the sensitivity tests)."""
    if w["fmt"] == "bf16":
        return w["plain"].to(F64)
    sc = w["scales"]
    if scale_shift:
        sc = torch.roll(sc, -scale_shift, dims=1)
    s = sc.float().repeat_interleave(w["G"], dim=1)
    q = w["codes"].float()
    if exact:
        return q.to(F64) * s.to(F64)
    # q*s is exact in f32 (8 x 8 significant bits); one bf16 rounding
    return (q * s).to(BF16).to(F64)


# ------------------------------------------------------- reference and bound

def gemm_ref(x: torch.Tensor, w64: torch.Tensor, bias=None):
    """(ref, A): ref = x w^T + bias and A = |x| |w|^T + |bias| in fp64."""
    x64 = x.detach().cpu().to(F64)
    ref = x64 @ w64.t()
    mag = x64.abs() @ w64.abs().t()
    if bias is not None:
        b = bias.detach().cpu().to(F64)
        ref = ref + b
        mag = mag + b.abs()
    return ref, mag


def gemm_acc(mag: torch.Tensor, k: int) -> torch.Tensor:
    """f32 accumulation allowance: one f32 ulp (2^-23 relative) of the
    magnitude sum A per accumulation step, K steps charged. The kernels
    take at most K + 32 + 1 <= 2K steps whose running magnitude is <= A
    (products, split-k atomics, bias); the bound holds for any order and
    for truncating accumulators, since it charges a whole ulp, not half."""
    return k * 2.0 ** -23 * mag


def gemm_tol(ref, mag, k: int, extra: float = 0.0) -> torch.Tensor:
    """2^-8 |ref| (one bf16 rounding of the output) + (1 + 2^-8) acc (the
    accumulation error, itself carried through that rounding) + extra."""
    return 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * gemm_acc(mag, k) + extra


def ratio(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """max |got - ref| / tol (nan/inf -> inf; an element with zero
    tolerance must match exactly)."""
    got = got.detach().cpu().to(F64)
    if got.shape != ref.shape or not torch.isfinite(got).all():
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(tol > 0, err / tol,
                    torch.where(err > 0, torch.full_like(err, float("inf")),
                                torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def checksum(t: torch.Tensor) -> str:
    raw = t.detach().cpu().contiguous().view(torch.int16).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


# --------------------------------------------------------------- dispatch

def gemm_call(w: dict, x, bias, device: str, packed: bool = True):
    """The production entry point for this format on ``device``. The CPU
    path of gemv_int4 takes the row-major nibbles."""
    import dnet_amd.ops as ops
    fmt = w["fmt"]
    x = x.to(device)
    b = None if bias is None else bias.to(device)
    if fmt == "bf16":
        return ops.gemv_bf16(x, w["plain"].to(device), b)
    sc = w["scales"].to(device)
    if fmt == "int8":
        wt = w["packed"] if packed else w["plain"]
        return ops.gemv_int8(x, wt.to(device), sc, w["G"], b, packed=packed)
    wt = w["packed"] if device != "cpu" else w["plain"]
    return ops.gemv_int4(x, wt.to(device), sc, w["G"], b, True)


def exact_contract(c: dict, device: str) -> bool:
    """Only the scalar gemv_int8 kernel multiplies by the unrounded q*s:
    on the GPU, int8 at M <= 2 or in the unpacked layout."""
    return (device != "cpu" and c["fmt"] == "int8"
            and (c["M"] <= 2 or not c.get("packed", True)))


def via_gemm_m16(c: dict) -> bool:
    """Does the GPU path of this case run gemm_m16 (not a scalar kernel)?"""
    if c["fmt"] == "int4":
        return True
    if c["fmt"] == "int8":
        return c.get("packed", True) and c["M"] > 2
    return c["K"] % 64 == 0


def splits_k(c: dict) -> bool:
    """Does gemm_m16 split K for this shape in this process? (M enters the
    choice only through the scratch capacity, and the query refuses
    M <= 2 and M > 64, so every chunk is asked at a clamped M.)"""
    import dnet_amd.ops as ops
    if not via_gemm_m16(c):
        return False
    scratch = ops._get_scratch(torch.device("cuda", 0)).numel()
    m = max(3, min(c["M"], 64))
    return ops._will_defer(m, c["N"], c["K"], c["G"] if c["G"] else 0,
                           BITS[c["fmt"]], scratch)


# ------------------------------------------------------ B. random-data cases

MAT_M = [1, 2, 3, 15, 16, 17, 32, 33, 64, 65, 129]
MAT_N = [8, 17, 63, 64, 65, 1000]
MAT_K = [64, 128, 192, 256, 320, 576, 1088, 2048]
MAT_G = [64, 128, 256]
MAT_FMT = ["bf16", "int8", "int4"]
MAT_BIAS = [False, True]
MAT_AXES = [MAT_FMT, MAT_M, MAT_N, MAT_K, MAT_G, MAT_BIAS]
MAT_KEYS = ["fmt", "M", "N", "K", "G", "bias"]


def matrix_row_valid(fmt, m, n, k, g, bias) -> bool:
    """G divides K; int4 takes K % 128 == 0 and G in {128, 256}; bf16 has
    no groups, so its rows carry the first G value only."""
    if fmt == "bf16":
        return g == MAT_G[0]
    if k % g:
        return False
    if fmt == "int4":
        return k % 128 == 0 and g % 128 == 0
    return True


def pairwise(axes, valid, seed_rows=()):
    """Greedy all-pairs cover of the valid rows of the cartesian product:
    every pair of values of two different axes that occurs in some valid
    row occurs in a chosen row. Deterministic. ``seed_rows`` (index
    tuples) count as already chosen."""
    n = len(axes)
    cand = [r for r in itertools.product(*[range(len(a)) for a in axes])
            if valid(*[axes[i][r[i]] for i in range(n)])]
    off = np.cumsum([0] + [len(a) for a in axes])
    width = int(off[-1])
    combos = list(itertools.combinations(range(n), 2))
    ids = np.array([[(off[i] + r[i]) * width + off[j] + r[j]
                     for i, j in combos] for r in cand])
    need = np.zeros(width * width, dtype=bool)
    need[ids.ravel()] = True
    for r in seed_rows:
        need[[(off[i] + r[i]) * width + off[j] + r[j]
              for i, j in combos]] = False
    rows = []
    while need.any():
        best = int(np.argmax(need[ids].sum(axis=1)))
        rows.append(cand[best])
        need[ids[best]] = False
    return rows


def case_id(c: dict) -> str:
    s = f"{c['fmt']}-M{c['M']}-N{c['N']}-K{c['K']}"
    if c["fmt"] != "bf16":
        s += f"-G{c['G']}"
        if not c.get("packed", True):
            s += "-plain"
    if c.get("bias"):
        s += "-bias"
    if c.get("quantizer"):
        s += "-quantizer"
    return s


def _case(fmt, m, n, k, g=0, bias=False, **kw) -> dict:
    return dict(fmt=fmt, M=m, N=n, K=k, G=0 if fmt == "bf16" else g,
                bias=bias, **kw)


@functools.lru_cache(maxsize=None)
def _matrix_cases() -> tuple:
    cs = []
    # all pairs among the quantized rows first (the bf16 kernel has no
    # groups and would otherwise soak up most of the M x K pairs), then
    # whatever pairs the bf16 rows still owe
    rows = pairwise(MAT_AXES, lambda f, *r: f != "bf16"
                    and matrix_row_valid(f, *r))
    rows += pairwise(MAT_AXES, matrix_row_valid, rows)
    for r in rows:
        v = [MAT_AXES[i][r[i]] for i in range(len(MAT_AXES))]
        cs.append(_case(*v))
    # the production quantizers stay in the loop: one case per format
    cs.append(_case("int8", 17, 65, 576, 64, True, quantizer=True))
    cs.append(_case("int4", 17, 65, 2048, 128, True, quantizer=True))
    # forced 8-way splits with fewer 128-k quads than splits (the last
    # split does everything); naturally a single-split tail-only shape
    cs.append(_case("int4", 16, 72, 640, 128, True))
    # forced 8-way splits start at odd pairs: misaligned for G = 128
    cs.append(_case("int8", 33, 65, 640, 128, True))
    # the all-pairs cover counts a (K, G) pair as held by any format, and
    # int4 holds these: int8 G = 128 over several scales per row, one M
    # per MT tier (1, 2, 4 stacked tiles)
    for i, (k, m) in enumerate(itertools.product((256, 2048), (16, 33, 64))):
        cs.append(_case("int8", m, (65, 1000, 63)[i % 3], k, 128, i % 2 == 1))
    for i, c in enumerate(cs):
        c["seed"] = 2000 + i
    return tuple(cs)


def matrix_cases() -> list:
    return [dict(c) for c in _matrix_cases()]


def scalar_bf16_cases() -> list:
    """K % 64 != 0: the only shapes that reach the scalar gemv_bf16 kernel
    (M tiling 7 -> 6+1, 11 -> 8+3, 15 -> 12+3, 17 -> 16+1, 33 -> 16+16+1)."""
    cs = [_case("bf16", m, n, k, bias=True)
          for k in (72, 200) for m in (1, 2, 7, 11, 15, 16, 17, 33)
          for n in (5, 1000)]
    for i, c in enumerate(cs):
        c["seed"] = 3000 + i
    return cs


def scalar_int8_cases() -> list:
    """Unpacked int8 stays on the scalar gemv_int8 kernel at any M."""
    cs = []
    for i, ((k, g), m) in enumerate(itertools.product(
            ((80, 16), (1024, 16), (1024, 64)), (1, 7, 13, 17, 33))):
        cs.append(_case("int8", m, (5, 1000)[i % 2], k, g, bias=i % 3 != 0,
                        packed=False))
    for i, c in enumerate(cs):
        c["seed"] = 3100 + i
    return cs


GRID_STRIDE_CASE = dict(_case("int8", 64, 8200, 1024, 128, True), seed=3200)
HYGIENE_CASES = [dict(_case("int8", 64, 4096, 1024, 128), seed=3210),
                 dict(_case("int8", 3, 72, 1088, 64), seed=3211),
                 dict(_case("int4", 16, 1000, 2048, 128, True), seed=3212)]


def build_case(c: dict):
    """(x, weights, bias) of one case, from its own seed."""
    gen = torch.Generator().manual_seed(c["seed"])
    x = torch.randn(c["M"], c["K"], generator=gen).to(BF16)
    w = make_weights(c["fmt"], c["N"], c["K"], c["G"], gen,
                     c.get("quantizer", False))
    bias = torch.randn(c["N"], generator=gen).to(BF16) if c["bias"] else None
    return x, w, bias


def case_reference(c: dict, x, w, bias, device: str, mutate: str = ""):
    """(ref, A) over the contract weights of the path ``device`` takes.
    ``mutate`` builds a deliberately wrong reference: "scale" reads the
    next group's scale, "pair" drops the last 64 k, "bias" omits the bias."""
    w64 = contract_weights(w, exact_contract(c, device),
                           scale_shift=1 if mutate == "scale" else 0)
    if mutate == "pair":
        w64 = w64.clone()
        w64[:, -64:] = 0
    if mutate == "bias":
        bias = None
    return gemm_ref(x, w64, bias)


def run_case(c: dict, device: str, mutate: str = "", extra: float = 0.0):
    """One GEMM case -> (worst err/tol, output)."""
    x, w, bias = build_case(c)
    got = gemm_call(w, x, bias, device, c.get("packed", True))
    ref, mag = case_reference(c, x, w, bias, device, mutate)
    return ratio(got, ref, gemm_tol(ref, mag, c["K"], extra)), got


# --------------------------------------------------------- A. one-hot sweep

def onehot_cases() -> list:
    cs = []
    for m, k in itertools.product((1, 16, 33, 64), (64, 320, 1088)):
        cs.append(_case("bf16", m, 72, k))
    for m, k in itertools.product((3, 16, 17, 64), (64, 192, 320, 1088)):
        cs.append(_case("int8", m, 72, k, 64))
    # G = 128 divides none of the issue's int8 K (64, 192, 320, 1088), so
    # its G = 128 column gets K of its own: one group, one full 256-k tile,
    # tiles + tail (640, 1152), and 1280, which splits K in two
    for m, k in itertools.product((3, 16, 17, 64),
                                  (128, 256, 640, 1152, 1280)):
        cs.append(_case("int8", m, 72, k, 128))
    for m, k in itertools.product((3, 16, 17, 64), (256, 1280)):
        cs.append(_case("int8", m, 72, k, 256))
    # K = 1280 is not in the issue's table: it is the smallest int4 shape
    # here that splits K on its own (see docs/KERNELS.md)
    for m, k, g in itertools.product((3, 16, 17, 64), (128, 384, 1152, 1280),
                                     (128, 256)):
        if k % g == 0:
            cs.append(_case("int4", m, 72, k, g))
    for m, k, packed in itertools.product((1, 2), (64, 320, 1088),
                                          (True, False)):
        cs.append(_case("int8", m, 72, k, 64, packed=packed))
    for m, k, packed in itertools.product((1, 2), (128, 640, 1152),
                                          (True, False)):     # as above
        cs.append(_case("int8", m, 72, k, 128, packed=packed))
    for i, c in enumerate(cs):
        c["seed"] = 4000 + i
    return cs


def run_onehot(c: dict, device: str):
    """Feed the rows of I_K, M at a time (zero-padded), through the entry
    point: launch j must return bf16(w_contract[:, jM:(j+1)M])^T exactly.
    One exact product plus exact zeros: no rounding anywhere but the
    output's, under either int8 contract (a single q*s rounded once is
    bf16(q*s)). Returns (#mismatching elements, all outputs [J*M, N])."""
    m, k = c["M"], c["K"]
    gen = torch.Generator().manual_seed(c["seed"])
    w = make_weights(c["fmt"], c["N"], k, c["G"], gen)
    launches = -(-k // m)
    eye = torch.zeros(launches * m, k, dtype=BF16)
    eye[:k] = torch.eye(k, dtype=BF16)
    eye = eye.to(device)
    wd = {**w, **{key: w[key].to(device) for key in ("plain", "packed")
                  if w[key] is not None}}
    if w["scales"] is not None:
        wd["scales"] = w["scales"].to(device)
    outs = [gemm_call(wd, eye[j * m:(j + 1) * m], None, device,
                      c.get("packed", True)) for j in range(launches)]
    got = torch.cat(outs).cpu()
    want = torch.zeros(launches * m, c["N"], dtype=BF16)
    want[:k] = contract_weights(w).to(BF16).t()
    # values, not bit patterns: a zero's sign is not part of the contract
    bad = int((got.float() != want.float()).sum()) if torch.isfinite(
        got.float()).all() else got.numel()
    return bad, got


# -------------------------------------------- D. elementwise / fused chains

def swiglu_ref(g: torch.Tensor, u: torch.Tensor):
    """fp64 silu(g) * u -> (y, silu(g))."""
    s = g * torch.sigmoid(g)
    return s * u, s


def swiglu_tol(y, u=None, silu=None, dg=None, du=None) -> torch.Tensor:
    """2^-8 |y| (output rounding) + 2^-16 |y| (cap for __expf and the f32
    arithmetic, 256x below the bf16 term) + the propagated input errors
    1.1 |u| dg + |silu(g)| du (|silu'| <= 1.1)."""
    tol = (2.0 ** -8 + 2.0 ** -16) * y.abs()
    if dg is not None:
        tol = tol + 1.1 * u.abs() * dg + silu.abs() * du
    return tol


def rmsnorm_ref(h: torch.Tensor, wn: torch.Tensor, eps: float):
    """fp64 RMSNorm -> (y, rms)."""
    wn = wn.detach().cpu().to(F64)
    rms = torch.sqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return h / rms * wn, rms


def rmsnorm_tol(y, h, rms, wn, dh=None) -> torch.Tensor:
    """2^-8 |y| (output rounding) + 2^-16 |y| (f32 reduction, rsqrtf, two
    f32 multiplies) + the propagation of an input error dh:
    |w_i| dh_i / rms + |y_i| * ||dh|| / ||h|| (the second term is the
    change of the row's rms)."""
    tol = (2.0 ** -8 + 2.0 ** -16) * y.abs()
    if dh is not None:
        wn = wn.detach().cpu().to(F64).abs()
        hn = h.norm(dim=-1, keepdim=True)
        tol = tol + wn * dh / rms + y.abs() * dh.norm(dim=-1,
                                                     keepdim=True) / hn
    return tol


# ------------------------------------------------ C. per-process variants

def variant_cases():
    """The quantized gemm_m16 part of the one-hot sweep and of the matrix:
    ("onehot" | "matrix", case)."""
    q = lambda c: c["fmt"] != "bf16" and via_gemm_m16(c)
    return ([("onehot", c) for c in onehot_cases() if q(c)]
            + [("matrix", c) for c in matrix_cases() if q(c)])


def run_variant_cases(device: str = "cuda") -> list:
    """One record per case: its err/tol (one-hot: 0 if exact, else inf),
    whether K is split in this process, and the output bits' checksum."""
    out = []
    for kind, c in variant_cases():
        if kind == "onehot":
            bad, got = run_onehot(c, device)
            r = 0.0 if bad == 0 else float("inf")
        else:
            r, got = run_case(c, device)
        out.append({"case": f"{kind}:{case_id(c)}", "ratio": r,
                    "split": bool(splits_k(c)), "checksum": checksum(got)})
    return out


def main_variant_cases() -> int:
    for rec in run_variant_cases("cuda"):
        print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    if "--variant-cases" in sys.argv[1:]:
        sys.exit(main_variant_cases())
    sys.exit("usage: gemm_reference.py --variant-cases")
