"""The bnb.int8 (LLM.int8) arithmetic restated in numpy: the specification the int8 kernels are tested against.

Modelled on bitsandbytes ``Linear8bitLt(has_fp16_weights=False, threshold=6.0)`` with bf16 where bitsandbytes uses
fp16. Imports nothing from the product.

Weights (once): ``s_w[n] = max_k |W[n,k]|`` (fp32), ``q = clamp(rint(W * (127 / s_w)), -127, 127)`` with the division
and the multiply in fp32 and ties to even; a zero row gives ``s_w = 0``, ``q = 0``.

Activations (per call, X (M, K) bf16 values, threshold tau): column j is an outlier column iff ``|X[m,j]| >= tau`` for
any row m (``tau <= 0``: none); ``s_x[m]`` = max |X[m,j]| over the other columns (0 when there is none);
``a = clamp(rint(X * (127 / s_x[m])), -127, 127)``, 0 in outlier columns and where ``s_x[m] = 0``.

Product: ``acc = sum_j a q`` exact; ``main = float(acc) * ((s_x * s_w) * C)``, ``C = float32(1 / 16129)``, every
operation fp32 in this association; ``out = sum_{j outlier} X[m,j] * (float(q[n,j]) * (s_w[n] * (1f / 127f)))`` with fp32
accumulation (ascending j here; the kernels' order may differ); ``y = bf16(main + out + bias)``; with a residual
``bf16(float(y) + float(res))``.
"""

from __future__ import annotations

import numpy as np

F = np.float32
TAU = 6.0
C = F(1.0 / 16129.0)


def bf16_round(x) -> np.ndarray:
    """fp32 -> nearest bf16 (ties to even), returned as fp32."""
    x = np.ascontiguousarray(x, dtype=F)
    b = x.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(F).reshape(x.shape)


def bf16_bits(x) -> np.ndarray:
    return (np.ascontiguousarray(x, dtype=F).view(np.uint32) >> 16).astype(np.uint16)


def _inv(s: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return np.where(s > 0, F(127.0) / s, F(0.0)).astype(F)


def quantize_weight(W):
    """W (N, K) fp32 (or bf16 values held in fp32) -> (q int8 (N, K), s_w fp32 (N,))."""
    W = np.asarray(W, dtype=F)
    s = np.abs(W).max(axis=1).astype(F)
    q = np.clip(np.rint(W * _inv(s)[:, None]), -127, 127).astype(np.int8)
    return q, s


def dequantize_weight(q, s) -> np.ndarray:
    """float64 q * s_w / 127."""
    return q.astype(np.float64) * (s.astype(np.float64) / 127.0)[:, None]


def quantize_act(X, tau: float = TAU):
    """X (M, K) bf16 values in fp32 -> (a int8 (M, K), s_x fp32 (M,), outlier column mask bool (K,))."""
    X = np.atleast_2d(np.asarray(X, dtype=F))
    O = (np.abs(X) >= F(tau)).any(axis=0) if tau > 0 else np.zeros(X.shape[1], bool)
    s = np.abs(np.where(O[None, :], F(0), X)).max(axis=1).astype(F)
    a = np.clip(np.rint(X * _inv(s)[:, None]), -127, 127).astype(np.int8)
    a[:, O] = 0
    return a, s, O


def int_product(a, q) -> np.ndarray:
    """sum_j a q as float64 (exact: |acc| < 2^53)."""
    return a.astype(np.float64) @ q.astype(np.float64).T


def linear(X, q, s_w, bias=None, residual=None, tau: float = TAU) -> np.ndarray:
    """The spec's rounding points in fp32; returns y (M, N) as bf16 values in fp32."""
    X = np.atleast_2d(np.asarray(X, dtype=F))
    a, s_x, O = quantize_act(X, tau)
    acc = int_product(a, q).astype(F)
    main = acc * ((s_x[:, None] * s_w[None, :].astype(F)) * C)
    out = np.zeros_like(main)
    s127 = s_w.astype(F) * (F(1.0) / F(127.0))
    for j in np.nonzero(O)[0]:
        out = out + X[:, j, None] * (q[:, j].astype(F) * s127)[None, :]
    t = main + out
    if bias is not None:
        t = t + np.asarray(bias, dtype=F)[None, :]
    y = bf16_round(t)
    if residual is not None:
        y = bf16_round(y + np.asarray(residual, dtype=F).reshape(y.shape))
    return y


def linear_exact(X, q, s_w, bias=None, residual=None, tau: float = TAU) -> np.ndarray:
    """The same decomposition evaluated in float64 with no rounding after the two quantizations."""
    X = np.atleast_2d(np.asarray(X, dtype=F))
    a, s_x, O = quantize_act(X, tau)
    s_w = s_w.astype(np.float64)
    y = int_product(a, q) * (s_x.astype(np.float64)[:, None] * s_w[None, :] / 16129.0)
    if O.any():
        y = y + X[:, O].astype(np.float64) @ (q[:, O].astype(np.float64) * (s_w / 127.0)[:, None]).T
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)[None, :]
    if residual is not None:
        y = y + np.asarray(residual, dtype=np.float64).reshape(y.shape)
    return y
