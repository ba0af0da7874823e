"""Hand-built weights on which every weight kernel has ONE right answer, bit for bit (tests/test_gpu_exact_linear.py).

Codes and scales are written directly, never through a quantizer, packed with the specifications the formats already
have (oracle.quant, mxfp4_spec, kv8_spec), and the expected weight W' comes from those same specifications: the bf16
value a kernel multiplies, bf16(value(code) * scale).

Two families per format (bf16, int4-g, nf4, fp4, fp8-g128, mxfp4):

* ``full_range``: every code in every column residue of a 16-B chunk and in a row's last chunk, the scales cycling over
  the contract range, both ends included. For products with ONE non-zero term (one-hot activations, X = v I): the
  result is that term, whatever the order of summation.
* ``integer``: codes whose values are small integer multiples of ``UNIT[fmt]``, scales in {1, 2, 4}; with activations
  in {-2 .. 2} and an integer bias every partial sum, in any order, is an integer below 2^24 units and so exact in fp32
  (``assert_order_free`` is that condition, checked, not assumed). nf4 keeps the three codes whose table value is a
  dyadic (-1, 0, 1), fp4 the eight that are (0, 1/4, 1/2, 1 and their negatives).

The expected outputs go through the rounding points the kernels document: h = bf16(sum + bias), y = bf16(h + residual);
SwiGLU y = bf16(bf16(silu(bf16 a)) * bf16 b), where a >= 32 makes bf16(silu(bf16 a)) == bf16 a for any exp.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from kv8_spec import kv8_dequantize
from mxfp4_spec import mx_dequantize, mx_pack
from oracle import quant

FORMATS = ("bf16", "int4", "nf4", "fp4", "fp8", "mxfp4")
Q4_FMT = {"int4": 0, "nf4": 1, "bf16": 2, "fp4": 3}  # include/litgpt_amd.h LGA_FMT_*
CHUNK = {"bf16": 8, "int4": 32, "nf4": 32, "fp4": 32, "fp8": 16, "mxfp4": 32}  # columns of one 16-B load
MIN_K = {"bf16": 8, "int4": 32, "nf4": 32, "fp4": 32, "fp8": 128, "mxfp4": 32}
UNIT = {"bf16": 1.0, "int4": 1.0, "nf4": 1.0, "fp4": 0.25, "fp8": 0.5, "mxfp4": 0.5}
EXP_RANGE = {"int4": (-100, 100), "nf4": (-100, 100), "fp4": (-100, 100), "fp8": (-100, 100), "mxfp4": (-125, 125)}

# bf16 as a code book: normal values and the two zeros over the exponent range, never a subnormal
_BF16_MANT = (1.0, 1.0078125, 1.5, 1.9921875)  # 1, 1 + 2^-7, 1.5, 2 - 2^-7: both ends of the 7-bit mantissa
_BF16_EXP = (-100, -61, -20, -1, 0, 1, 20, 61, 100)
BF16_TABLE = np.array([0.0, -0.0] + [s * m * 2.0 ** e for e in _BF16_EXP for m in _BF16_MANT for s in (1.0, -1.0)],
                      dtype=np.float32)
FP8_CODES = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)  # the 254 finite e4m3fn codes


def group_of(fmt: str, K: int) -> int:
    """The scale group the tests use at this K: the format's own, or the widest of 128 / 64 / 32 dividing K."""
    if fmt == "bf16":
        return K
    if fmt == "fp8":
        return 128
    if fmt == "mxfp4":
        return 32
    for g in ((128, 64, 32) if fmt == "int4" else (64, 32)):
        if K % g == 0:
            return g
    raise ValueError(f"{fmt}: K={K} is no multiple of 32")


@dataclass
class Weight:
    fmt: str
    N: int
    K: int
    group: int
    index: np.ndarray  # (N, K) position of each weight's code in the format's code list (the coverage tests)
    operands: Tuple[torch.Tensor, ...]  # what the entry point takes: (weight,) or (codes, scales), CPU tensors
    deq: torch.Tensor  # (N, K) fp32: W', the bf16 value the kernels multiply
    exps: Optional[np.ndarray] = None  # (N, K / group) scale exponents (full-range family)


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """fp32 / fp64 values that are exact in fp32 -> the nearest bf16 (ties to even), as fp32."""
    f = t.float()
    assert torch.equal(f.double(), t.double()), "bf16_round: the value is not exact in fp32"
    return f.bfloat16().float()


# ------------------------------------------------------------------------------------------------ packing
def _pack(fmt: str, codes: np.ndarray, scales: np.ndarray, group: int):
    """Code values (N, K) (bf16: fp32 values) and per-group scales (N, K / group) (int4: bf16 bits; nf4 / fp4: fp32
    absmax; fp8: fp32 powers of two; mxfp4: e8m0 bytes) -> (operands, W')."""
    N, K = codes.shape
    if fmt == "bf16":
        w = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.float32))
        assert torch.equal(w.bfloat16().float(), w)
        return (w.bfloat16(),), w
    if fmt in ("int4", "nf4", "fp4"):
        packed = quant._pack_nibbles(codes)
        deq = torch.from_numpy(quant.dequantize_fmt(packed, scales, Q4_FMT[fmt], group))
        sc = (torch.from_numpy(scales.view(np.int16)).view(torch.bfloat16) if fmt == "int4"
              else torch.from_numpy(scales.astype(np.float32)))
        return (torch.from_numpy(packed), sc.contiguous()), deq.bfloat16().float()  # bf16(value * scale)
    if fmt == "fp8":
        c = torch.from_numpy(codes)
        s = torch.from_numpy(scales.astype(np.float32))
        deq = kv8_dequantize(c.view(N, K // 128, 128), s).view(N, K)
        assert torch.equal(s.bfloat16().float(), s) and torch.equal(deq.bfloat16().float(), deq)
        return (c, s.bfloat16()), deq
    c, e = torch.from_numpy(codes), torch.from_numpy(scales.astype(np.uint8))
    deq = mx_dequantize(c.view(N, K // 32, 32), e).view(N, K)
    assert torch.equal(deq.bfloat16().float(), deq)
    return (mx_pack(c), e), deq


def _coprime_at_most(n: int, ncodes: int) -> int:
    return next(m for m in range(max(n, 1), 0, -1) if math.gcd(m, ncodes) == 1)


def _code_list(fmt: str) -> np.ndarray:
    if fmt == "bf16":
        return BF16_TABLE
    return FP8_CODES if fmt == "fp8" else np.arange(16, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ full range
def _exponent_cycle(lo: int, hi: int) -> np.ndarray:
    """lo, hi, lo + 1, hi - 1, ...: both ends come first, so the shortest weight has them."""
    out = []
    a, b = lo, hi
    while a <= b:
        out.append(a)
        if b != a:
            out.append(b)
        a, b = a + 1, b - 1
    return np.array(out, dtype=np.int64)


def full_range(fmt: str, N: int, K: int, exp_range: Optional[Tuple[int, int]] = None,
               group: Optional[int] = None) -> Weight:
    """index(n, k) = (n + m (k // C + k % C)) mod ncodes, C the chunk's columns and m <= N coprime to ncodes: along one
    residue, and along one chunk, n + m j runs over a gap-free range, so each holds every code once N * (K / C) (N * C)
    reaches ncodes. Scale exponents follow _exponent_cycle over (row, group); int4 / nf4 / fp4 scales carry non-trivial
    mantissas."""
    group = group or group_of(fmt, K)
    code_list = _code_list(fmt)
    nc, C = len(code_list), CHUNK[fmt]
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    index = ((n + _coprime_at_most(N, nc) * (k // C + k % C)) % nc).astype(np.int16)
    codes = code_list[index]
    if fmt == "bf16":
        return Weight(fmt, N, K, group, index, *_pack(fmt, codes, None, group))
    G = K // group
    cyc = _exponent_cycle(*(exp_range or EXP_RANGE[fmt]))
    t = np.arange(N)[:, None] * G + np.arange(G)[None, :]
    exps = cyc[t % len(cyc)]
    if fmt == "mxfp4":
        scales = (exps + 127).astype(np.uint8)
    elif fmt == "fp8":
        scales = np.ldexp(np.float32(1.0), exps).astype(np.float32)
    elif fmt == "int4":  # 1.m with a 7-bit mantissa that changes from group to group
        scales = quant.f32_to_bf16_bits(np.ldexp((1.0 + (t * 37 % 128) / 128.0), exps).astype(np.float32))
    else:  # fp32 absmax, all 23 mantissa bits in use
        scales = np.ldexp(1.0 + (t * 7919 % 8388608 + 4321) % 8388608 / 8388608.0, exps).astype(np.float32)
    ops_, deq = _pack(fmt, codes, scales, group)
    assert bool(torch.isfinite(deq).all()) and bool(((deq == 0) | (deq.abs() >= 2.0 ** -126)).all())
    return Weight(fmt, N, K, group, index, ops_, deq, exps)


# ------------------------------------------------------------------------------------------------ integer family
def _integer_codes(fmt: str, positive: bool) -> np.ndarray:
    """The codes of the dense family: every value a multiple of UNIT[fmt]; positive: values >= 0.5 only."""
    if fmt == "bf16":
        v = np.arange(1, 9) if positive else np.arange(-8, 9)
        return v.astype(np.float32)
    if fmt == "int4":
        return np.arange(9 if positive else 0, 16, dtype=np.uint8)
    if fmt == "nf4":
        return np.array([15] if positive else [0, 7, 15], dtype=np.uint8)
    if fmt == "fp4":  # FP4: 3 -> 1, 5 -> 1/2, 7 -> 1/4, 0 -> 0, + 8: the negatives
        return np.array([3, 5] if positive else [0, 3, 5, 7, 8, 11, 13, 15], dtype=np.uint8)
    if fmt == "fp8":
        mags = torch.arange(1, 17).float() * 0.5  # 0.5 .. 8: three mantissa bits hold every one
        pos = mags.to(torch.float8_e4m3fn)
        assert torch.equal(pos.float(), mags)
        pos = pos.view(torch.uint8).numpy()
        return pos if positive else np.concatenate([[0, 0x80], pos, pos | 0x80]).astype(np.uint8)
    return np.arange(1, 8, dtype=np.uint8) if positive else np.arange(16, dtype=np.uint8)


def integer(fmt: str, N: int, K: int, seed: int = 0, positive: bool = False, group: Optional[int] = None) -> Weight:
    group = group or group_of(fmt, K)
    rng = np.random.default_rng([seed, N, K, FORMATS.index(fmt)])
    allowed = _integer_codes(fmt, positive)
    pick = rng.integers(0, len(allowed), size=(N, K))
    pick[:, -CHUNK[fmt]:] = (np.arange(N)[:, None] + np.arange(CHUNK[fmt])[None, :]) % len(allowed)  # the last chunk: all
    codes = allowed[pick]
    if fmt == "bf16":
        return Weight(fmt, N, K, group, pick.astype(np.int16), *_pack(fmt, codes, None, group))
    e = rng.integers(0, 3, size=(N, K // group))
    if fmt == "mxfp4":
        scales = (e + 127).astype(np.uint8)
    elif fmt == "int4":
        scales = quant.f32_to_bf16_bits(np.ldexp(np.float32(1.0), e).astype(np.float32))
    else:
        scales = np.ldexp(np.float32(1.0), e).astype(np.float32)
    ops_, deq = _pack(fmt, codes, scales, group)
    assert torch.equal(deq / UNIT[fmt], (deq / UNIT[fmt]).round())
    return Weight(fmt, N, K, group, pick.astype(np.int16), ops_, deq, e)


def activations(shape, seed: int, positive: bool = False) -> torch.Tensor:
    """{-2 .. 2}, fp32. positive (the SwiGLU forms): {1, 2} * max(1, 64 // K), so that against weights >= 0.5 the sum
    over K columns is at least 32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(1 if positive else -2, 3, tuple(shape), generator=g).float()
    return x * max(1, 64 // shape[-1]) if positive else x


def small_ints(shape, seed: int, bound: int = 4) -> torch.Tensor:
    """Bias / residual: integers in [-bound, bound], fp32."""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


# ------------------------------------------------------------------------------------------------ the condition
def assert_order_free(x: torch.Tensor, w_deq: torch.Tensor, bias: Optional[torch.Tensor] = None,
                      unit: float = 1.0) -> None:
    """x (K,) or (M, K), w_deq (N, K): raises unless x, W' and the bias are whole units and sum_k |x_k| |w_nk| + |bias_n|
    stays below 2^24 units for every output — then every partial sum, in any order and grouping, is an integer below
    2^24 units and exact in fp32."""
    xd, wd = x.double().reshape(-1, x.shape[-1]), w_deq.double() / unit
    for name, t in (("x", xd), ("w", wd), ("bias", None if bias is None else bias.double() / unit)):
        if t is not None and not bool((t == t.round()).all()):
            raise ValueError(f"assert_order_free: {name} is not a whole number of units")
    tot = xd.abs() @ wd.abs().T
    if bias is not None:
        tot = tot + bias.double().abs() / unit
    worst = float(tot.max())
    if not worst < 2.0 ** 24:
        raise ValueError(f"assert_order_free: sum |x| |w| reaches {worst:.0f} units, not below 2^24")


# ------------------------------------------------------------------------------------------------ expected outputs
def expect_linear(x: torch.Tensor, w_deq: torch.Tensor, bias=None, residual=None) -> torch.Tensor:
    """bf16(bf16(x W'^T + bias) + residual) from the exact (float64) product; x (K,) -> (N,), (M, K) -> (M, N)."""
    s = x.double() @ w_deq.double().T
    if bias is not None:
        s = s + bias.double()
    h = bf16_round(s)
    return h if residual is None else bf16_round(h.double() + residual.double())


def expect_swiglu(x: torch.Tensor, w1_deq: torch.Tensor, w2_deq: torch.Tensor) -> torch.Tensor:
    """bf16(bf16(silu(bf16 a)) * bf16 b) with a = x W1'^T >= 32 everywhere, where silu(a) rounds to a."""
    a = bf16_round(x.double() @ w1_deq.double().T)
    b = bf16_round(x.double() @ w2_deq.double().T)
    if not bool((a >= 32).all()):
        raise ValueError("expect_swiglu: a < 32, silu(a) is not a in bf16")
    return bf16_round(a.double() * b.double())  # two 8-bit mantissas: the product is exact in fp32


def one_hot_columns(K: int, seed: int = 0) -> list:
    """Every column up to K = 512; above, the boundaries of chunks, passes and scale groups, the row's tail, and 64
    seeded random columns."""
    if K <= 512:
        return list(range(K))
    cols = {0, 1, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128}
    for c in range(512, K + 1, 512):
        cols |= {c - 1, c, c + 1}
    for p in range(4096, K + 1, 4096):
        cols |= {p - 1, p}
    cols |= set(range(K - 33, K))
    cols |= set(np.random.default_rng([seed, K]).integers(0, K, size=64).tolist())
    return sorted(c for c in cols if 0 <= c < K)


# ------------------------------------------------------------------------------------------------ the case table
def gemv_shapes(fmt: str) -> list:
    """(N, K) of the decode GEMV cases: one K per dispatch class (the smallest, one pass, several passes off a pass
    boundary, the long rows), N = 77 leaving a wave's rows past N, and N = 5 at the largest K."""
    return [(77, K) for K in (MIN_K[fmt], 4096, 11008, 16384, 32768)] + [(5, 32768)]


Q4_GEMV_VARIANT_SHAPES = [(77, 1376), (640, 4096)]  # q4_gemv under variant -1, 0, 3, 4, 38
Q4_GEMV_VARIANTS = (-1, 0, 3, 4, 38)
# (N, K) of the prefill GEMMs, by entry point; K = 96 and 160: K % 64 == 32, the half K-step
GEMM_SHAPES = {
    "fp8_gemm": [(N, K) for N in (64, 200) for K in (128, 384)],
    "mxfp4_gemm": [(N, K) for N in (64, 200) for K in (96, 160)],
    "q4_gemm": [(64, 96), (200, 128)],
    "bf16_gemm": [(64, 96), (200, 128)],
    "q4_gemm_fused": [(136, 64), (136, 256), (136, 512)],  # K = 512: eight K-steps, LGA_Q4F_SPLITS up to 8
}
# q4_gemm_fused / q4_gemm_swiglu at N = 136 under the planner's knobs: (environment, K) of the identity runs and
# (environment, M, K) of the dense ones; every K is one of GEMM_SHAPES["q4_gemm_fused"]
Q4F_IDENTITY_ENV = [({"LGA_Q4F_BN": "256"}, 256), ({"LGA_Q4F_SPLITS": "2"}, 512), ({"LGA_Q4F_SPLITS": "8"}, 512)]
Q4F_DENSE_ENV = [({}, 17, 256), ({}, 129, 256), ({"LGA_Q4F_BN": "256"}, 129, 256), ({"LGA_Q4F_SPLITS": "2"}, 17, 512),
                 ({"LGA_Q4F_SPLITS": "8"}, 129, 512)]
GEMM_FORMATS = {"fp8_gemm": ("fp8",), "mxfp4_gemm": ("mxfp4",), "q4_gemm": ("int4", "nf4", "fp4"),
                "bf16_gemm": ("bf16",), "q4_gemm_fused": ("int4", "nf4", "bf16", "fp4")}
GEMM_M = (2, 17, 129)
ROWS_M = (2, 5, 8)
