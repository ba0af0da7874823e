"""Python view of the C-ABI library ``liblitgpt_amd.so`` (declared in ``include/litgpt_amd.h``).

Every hot op of the decode path is a HIP kernel in ``lit-gpt_amd/csrc`` reached through these thin wrappers:
they validate dtype / shape / contiguity / device, pass raw device pointers and sizes, launch on torch's
current HIP stream (so the calls can be captured into a HIP graph), and turn a non-zero return code into a
``RuntimeError`` carrying ``lga_last_error_string()``. There is no CPU fallback: without the library, or on a
non-GPU tensor, every op raises.

Reference boundary replaced: bitsandbytes' ctypes C functions behind ``Linear4bit`` and the ATen
kernels that ``lit_gpt/model.py`` issues (RMSNorm, RoPE, index_copy_, SDPA, embedding, argmax).
"""

from __future__ import annotations

import ctypes
import math
import os
from pathlib import Path
from typing import Optional

import torch

LIB_PATH = Path(os.environ.get("LGA_LIB", Path(__file__).resolve().parent / "_lib" / "liblitgpt_amd.so"))

FMT_Q4G = 0  # int4, symmetric, per-group bf16 scale
FMT_NF4 = 1  # bitsandbytes NF4 codebook, per-block fp32 absmax
FMT_BF16 = 2  # (prefill GEMM only) unquantized bf16 weight
FMT_FP4 = 3  # bitsandbytes FP4 code, per-block fp32 absmax
FMT_INT8 = 4  # LLM.int8: int8 (N, K) + fp32 row absmax (the int8_* ops only)

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_long
_F = ctypes.c_float
_SZ = ctypes.c_size_t

# symbol -> argtypes; the exported surface of include/litgpt_amd.h (tests check the .so exports each one)
SIGNATURES = {
    "lga_version": [],
    "lga_last_error_string": [],
    "lga_device_info": [_I, _P, _P, _I],
    "lga_preload_kernels": [],
    "lga_quantize": [_P, _I, _P, _P, _I, _I, _I, _I, _P],
    "lga_nf4_double_quant": [_P, _L, _P, _P, _P],
    "lga_q4_gemv": [_P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P],
    "lga_q4_gemv_swiglu": [_P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P],
    "lga_q4_gemv_rows": [_P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P],
    "lga_q4_gemv_swiglu_rows": [_P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P],
    "lga_q4_gemm": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "lga_q4f_fits": [_I, _I, _I, _I, _I],
    "lga_q4f_workspace_bytes": [_I, _I, _I, _I],
    "lga_q4_gemm_fused": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P],
    "lga_q4_gemm_swiglu": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P],
    "lga_q4_dequantize": [_P, _P, _P, _I, _I, _I, _I, _P],
    "lga_bf16_gemv": [_P, _P, _P, _P, _P, _F, _P, _I, _I, _P],
    "lga_bf16_gemv_swiglu": [_P, _P, _P, _P, _F, _P, _I, _I, _P],
    "lga_bf16_gemm": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "lga_int8_quantize": [_P, _I, _P, _P, _I, _I, _P],
    "lga_int8_gemv": [_P, _P, _P, _P, _P, _P, _F, _F, _P, _I, _I, _P],
    "lga_int8_gemv_swiglu": [_P, _P, _P, _P, _P, _P, _F, _F, _P, _I, _I, _P],
    "lga_int8_quantize_act": [_P, _P, _P, _P, _P, _P, _I, _I, _F, _P],
    "lga_int8_gemm": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "lga_lora_gemv": [_P, _P, _F, _P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _I, _P],
    "lga_lora_gemv_rows": [_P, _P, _F, _P, _P, _P, _P, _I, ctypes.c_longlong, ctypes.c_longlong, _F, _P, _P, _P, _I,
                           _I, _I, _I, _I, _P],
    "lga_lora_down": [_P, _P, _P, _I, _I, _I, _P],
    "lga_lora_up": [_P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _I, _P],
    "lga_lora_merge": [_P, _P, _P, _P, _F, _I, _I, _I, _I, _P],
    "lga_rmsnorm": [_P, _P, _P, _I, _I, _F, _P],
    "lga_rope_kv_append": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "lga_embedding": [_P, _I, _P, _P, _I, _I, _I, _P],
    "lga_add": [_P, _P, _P, _L, _P],
    "lga_swiglu": [_P, _P, _P, _L, _P],
    "lga_layernorm": [_P, _P, _P, _P, _I, _I, _F, _P],
    "lga_gelu": [_P, _P, _L, _I, _P],
    "lga_attention": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P],
    "lga_attention_workspace_bytes": [_I, _I, _I, _I],
    "lga_attention_decode_fused": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P],
    "lga_attention_decode_window": [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P],
    "lga_attention_decode_fused_kv8": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F,
                                       _P],
    "lga_attention_decode_window_kv8": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F,
                                        _P],
    "lga_attention_decode_batch": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, ctypes.c_longlong, _P, _I, _I, _I, _I,
                                   _I, _I, _F, _P],
    "lga_attention_decode_shared": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, ctypes.c_longlong, _P, _I, _I, _I, _I,
                                    _I, _I, _F, _P],
    "lga_attention_decode_batch_kv8": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, ctypes.c_longlong,
                                       ctypes.c_longlong, _P, _I, _I, _I, _I, _I, _I, _F, _P],
    "lga_kv8_rope_append": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "lga_kv8_dequantize": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "lga_spec_accept": [_P, _I, _I, _P, _P, _P, _P, _P],
    "lga_adapter_attention": [_P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P],
    "lga_argmax": [_P, _I, _P, _P, _P, _P],
    "lga_q4_gemv_argmax_work_bytes": [_I, _I],
    "lga_q4_gemv_argmax_embed": [_P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P],
    "lga_argmax_embed": [_P, _I, _P, _P, _P, _P, _I, _I, _P, _P],
    "lga_moe_route": [_P, _I, _I, _I, _P, _P, _P],
    "lga_moe_gate_route": [_P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _P, _P, _P],
    "lga_q4_gemv_experts_pair_supported": [_I, _I, _I, _I],
    "lga_q4_gemv_experts_pair_counters": [_I],
    "lga_q4_gemv_experts_pair_combine": [_P, _P, _P, _P, _P, _P, _I, ctypes.c_longlong, ctypes.c_longlong, _P, _P,
                                         _P, _I, _I, _I, _I, _P],
    "lga_q4_gemv_experts": [_P, _P, _P, _P, _I, _I, ctypes.c_longlong, ctypes.c_longlong, _I, _P, _I, _I, _I, _I,
                            _I, _P],
    "lga_q4_gemv_swiglu_experts": [_P, _P, _P, _P, _P, _P, _I, _I, ctypes.c_longlong, ctypes.c_longlong, _P, _F,
                                   _P, _I, _I, _I, _I, _I, _P],
    "lga_moe_combine": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "lga_moe_group_tiles": [_I, _I, _I],
    "lga_moe_group": [_P, _I, _I, _I, _I, _P, _P, _P, _P],
    "lga_q4_gemm_swiglu_grouped": [_P, _P, _P, _P, _P, ctypes.c_longlong, ctypes.c_longlong, _P, _P, _P, _I, _I, _I,
                                   _I, _I, _I, _I, _P],
    "lga_q4_gemm_grouped": [_P, _P, _P, ctypes.c_longlong, ctypes.c_longlong, _P, _P, _P, _P, _I, _I, _I, _I, _I,
                            _I, _I, _P],
    "lga_comm_mailbox_bytes": [_I],
    "lga_comm_alloc": [ctypes.c_size_t, ctypes.POINTER(_P), _P],
    "lga_comm_open": [_P, ctypes.POINTER(_P)],
    "lga_comm_close": [_P],
    "lga_comm_free": [_P],
    "lga_comm_trace": [_P, _I],
    "lga_allreduce_bf16": [_P, _P, _P, _I, ctypes.POINTER(_P), _I, _I, _I, _P, _P, _P],
    "lga_f32_linear": [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    "lga_f32_layernorm": [_P, _P, _P, _P, _I, _I, _F, _P],
    "lga_f32_gelu": [_P, _P, _L, _I, _P],
    "lga_f32_add": [_P, _P, _P, _L, _P],
    "lga_f32_rope_kv_append": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "lga_f32_attention": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P],
    "lga_argmax_f32": [_P, _I, _P, _P, _P, _P],
    "lga_sample_topk": [_P, _I, _I, _F, _P, ctypes.c_ulonglong, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "lga_spec_accept_sample": [_P, _I, _I, _I, _F, _P, ctypes.c_ulonglong, _P, _P, _P, _P, _P, _P, _P],
    "lga_sample_nucleus": [_P, _I, _I, _F, _F, _P, ctypes.c_ulonglong, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P],
    "lga_spec_accept_sample_nucleus": [_P, _I, _I, _I, _F, _F, _P, ctypes.c_ulonglong, _P, _P, _P, _P, _P, _P, _P],
    "lga_q4_gemv_allreduce": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, ctypes.POINTER(_P), _I, _I, _I, _P, _P, _P,
                              _P],
    "lga_q4_gemv_allreduce_tagged": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, ctypes.POINTER(_P), _I, _I, _I, _P, _P,
                                     _P, _P],
    "lga_token_logprobs": [_P, _I, _I, _P, _P, _P, _P],
    "lga_token_logprobs_f32": [_P, _I, _I, _P, _P, _P, _P],
    "lga_logits_kl": [_P, _P, _I, _I, _P, _P, _P],
}
_RESTYPES = {"lga_q4_gemv_experts_pair_counters": ctypes.c_size_t, "lga_q4f_workspace_bytes": ctypes.c_size_t, "lga_last_error_string": ctypes.c_char_p, "lga_attention_workspace_bytes": ctypes.c_size_t,
             "lga_comm_mailbox_bytes": ctypes.c_size_t, "lga_q4_gemv_argmax_work_bytes": ctypes.c_size_t}

_lib: Optional[ctypes.CDLL] = None


class NativeLibraryError(RuntimeError):
    pass


def load_library(path: Optional[Path] = None, strict: bool = True) -> ctypes.CDLL:
    """Load (once) and return the HIP library. Raises loudly when it is missing: there is no fallback.
    ``strict=False`` (lab A/B of older builds only) skips the symbols a library does not export."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path or LIB_PATH)
    if not p.is_file():
        raise NativeLibraryError(
            f"HIP library not found at {p}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C lit-gpt_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(str(p))
    for name, argtypes in SIGNATURES.items():
        if not strict and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    if path is None:
        _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load_library().lga_last_error_string()
        raise RuntimeError(f"liblitgpt_amd error {rc}: {msg.decode() if msg else ''}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str, dtype: Optional[torch.dtype] = None) -> int:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (this build has no CPU path), got {t.device}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return t.data_ptr()


def _opt(t: Optional[torch.Tensor], name: str, dtype=None) -> Optional[int]:
    return None if t is None else _dev(t, name, dtype)


# ------------------------------------------------------------------------------------------------ quantizer
def quantize(weight: torch.Tensor, fmt: int, group: int):
    """(N, K) fp32/bf16 device weight -> (packed uint8 (N, K/2), scales) on the same device."""
    N, K = weight.shape
    w = weight.contiguous()
    if w.dtype not in (torch.float32, torch.bfloat16):
        w = w.float()
    qw = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    sdt = torch.bfloat16 if fmt == FMT_Q4G else torch.float32
    sc = torch.empty(N, K // group, dtype=sdt, device=w.device)
    _check(load_library().lga_quantize(_dev(w, "weight"), int(w.dtype == torch.bfloat16), qw.data_ptr(),
                                       sc.data_ptr(), N, K, group, fmt, _stream()))
    return qw, sc


# ------------------------------------------------------------------------------------------------ linear
def nf4_double_quant(absmax: torch.Tensor, code: torch.Tensor) -> torch.Tensor:
    """In place: nf4 absmax (fp32, contiguous) -> bitsandbytes' double-quantized statistic; returns the offset."""
    off = torch.empty(1, dtype=torch.float32, device=absmax.device)
    _check(load_library().lga_nf4_double_quant(_dev(absmax, "absmax", torch.float32), absmax.numel(),
                                               _dev(code, "code", torch.float32), _dev(off, "offset", torch.float32),
                                               _stream()))
    return off


def q4_gemv(x, qweight, scales, N, K, group, fmt, *, bias=None, residual=None, norm_weight=None, eps=1e-5,
            out=None, variant=-1):
    """y (N,) = x (K,) . dequant(W)^T  [+bias] [+residual]; optional fused RMSNorm of x (norm_weight)."""
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_q4_gemv(_dev(x, "x", torch.bfloat16), _dev(qweight, "qweight", torch.uint8),
                                      _dev(scales, "scales"), _opt(bias, "bias", torch.bfloat16),
                                      _opt(residual, "residual", torch.bfloat16),
                                      _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
                                      _dev(y, "y", torch.bfloat16), N, K, group, fmt, variant, _stream()))
    return y


def q4_gemv_swiglu(x, qw1, sc1, qw2, sc2, N, K, group, fmt, *, norm_weight=None, eps=1e-5, out=None, variant=-1):
    """y (N,) = bf16(silu(bf16(x W1^T))) * bf16(x W2^T), optional fused RMSNorm of x."""
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_q4_gemv_swiglu(_dev(x, "x", torch.bfloat16), _dev(qw1, "qw1", torch.uint8),
                                             _dev(sc1, "sc1"), _dev(qw2, "qw2", torch.uint8), _dev(sc2, "sc2"),
                                             _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
                                             _dev(y, "y", torch.bfloat16), N, K, group, fmt, variant, _stream()))
    return y


MAX_GEMV_ROWS = 8  # rows of one lga_q4_gemv*_rows launch == sequences of one batched decode step


def _gemv_rows(x, K, name):
    """The row count M of a (M, K) activation block for the rows GEMVs (1..MAX_GEMV_ROWS)."""
    if x.dim() != 2 or x.shape[1] != K:
        raise ValueError(f"{name}: x must be (M, K={K}), got {tuple(x.shape)}")
    M = x.shape[0]
    if not 1 <= M <= MAX_GEMV_ROWS:
        raise ValueError(f"{name}: M must be 1..{MAX_GEMV_ROWS} rows, got {M}")
    return M


def _rows_out(out, M, N, x, name):
    if out is None:
        return torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    if tuple(out.shape) != (M, N):
        raise ValueError(f"{name}: out must be ({M}, {N}), got {tuple(out.shape)}")
    return out


def q4_gemv_rows(x, qweight, scales, N, K, group, fmt, *, bias=None, residual=None, norm_weight=None, eps=1e-5,
                 out=None):
    """Y (M, N) = X (M, K) . dequant(W)^T [+bias] [+residual (M, N)] for 1 <= M <= 8 rows in one pass over the
    weights; row r has the bits of ``q4_gemv(x[r], ..., residual=residual[r], variant=-1)``."""
    M = _gemv_rows(x, K, "q4_gemv_rows")
    if fmt not in (FMT_Q4G, FMT_NF4, FMT_FP4):
        raise ValueError(f"q4_gemv_rows: fmt must be 0 (int4-g), 1 (nf4) or 3 (fp4), got {fmt}")
    if residual is not None and tuple(residual.shape) != (M, N):
        raise ValueError(f"q4_gemv_rows: residual must be ({M}, {N}), got {tuple(residual.shape)}")
    y = _rows_out(out, M, N, x, "q4_gemv_rows")
    _check(load_library().lga_q4_gemv_rows(_dev(x, "x", torch.bfloat16), _dev(qweight, "qweight", torch.uint8),
                                           _dev(scales, "scales"), _opt(bias, "bias", torch.bfloat16),
                                           _opt(residual, "residual", torch.bfloat16),
                                           _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
                                           _dev(y, "y", torch.bfloat16), M, N, K, group, fmt, _stream()))
    return y


def q4_gemv_swiglu_rows(x, qw1, sc1, qw2, sc2, N, K, group, fmt, *, norm_weight=None, eps=1e-5, out=None):
    """Y (M, N) = bf16(silu(bf16(X W1^T))) * bf16(X W2^T) for 1 <= M <= 8 rows in one pass over both weights; row r
    has the bits of ``q4_gemv_swiglu(x[r], ..., variant=-1)``."""
    M = _gemv_rows(x, K, "q4_gemv_swiglu_rows")
    if fmt not in (FMT_Q4G, FMT_NF4, FMT_FP4):
        raise ValueError(f"q4_gemv_swiglu_rows: fmt must be 0 (int4-g), 1 (nf4) or 3 (fp4), got {fmt}")
    y = _rows_out(out, M, N, x, "q4_gemv_swiglu_rows")
    _check(load_library().lga_q4_gemv_swiglu_rows(_dev(x, "x", torch.bfloat16), _dev(qw1, "qw1", torch.uint8),
                                                  _dev(sc1, "sc1"), _dev(qw2, "qw2", torch.uint8), _dev(sc2, "sc2"),
                                                  _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
                                                  _dev(y, "y", torch.bfloat16), M, N, K, group, fmt, _stream()))
    return y


def q4_gemm(x, qweight, scales, N, K, group, fmt, *, bias=None, residual=None, out=None):
    """Y (M, N) = X (M, K) . dequant(W)^T [+bias] [+residual] with MFMA tiles."""
    M = x.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_q4_gemm(_dev(x, "x", torch.bfloat16), _dev(qweight, "qweight", torch.uint8),
                                      _dev(scales, "scales"), _opt(bias, "bias", torch.bfloat16),
                                      _opt(residual, "residual", torch.bfloat16), _dev(y, "y", torch.bfloat16),
                                      M, N, K, group, fmt, _stream()))
    return y


def q4f_fits(M, N, K, group, fmt) -> bool:
    """Whether lga_q4_gemm_fused / lga_q4_gemm_swiglu take this shape (fmt 2 = bf16 weights)."""
    return bool(load_library().lga_q4f_fits(int(M), int(N), int(K), int(group), int(fmt)))


_Q4F_WS: dict = {}


def _q4f_workspace(M, N, K, swiglu, device):
    """The split-K workspace of a short-prompt fused GEMM: one zeroed buffer per device, grown as needed (its
    per-tile counters are left zeroed by every launch). Returns (ptr, bytes) or (None, 0)."""
    need = int(load_library().lga_q4f_workspace_bytes(int(M), int(N), int(K), int(bool(swiglu))))
    if need == 0:
        return None, 0
    ws = _Q4F_WS.get(device)
    if ws is None or ws.numel() < need:
        ws = _Q4F_WS[device] = torch.zeros(need, dtype=torch.uint8, device=device)
    return ws.data_ptr(), ws.numel()


def q4_gemm_fused(x, weight, scales, N, K, group, fmt, *, bias=None, residual=None, out=None):
    """Y (M, N) = X (M, K) . dequant(W)^T [+bias] [+residual], dequantization fused into the MFMA tiles
    (fmt 2: ``weight`` is the bf16 (N, K) matrix, ``scales`` None)."""
    M = x.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    wdt = torch.bfloat16 if fmt == 2 else torch.uint8
    ws, nws = _q4f_workspace(M, N, K, False, x.device)
    _check(load_library().lga_q4_gemm_fused(_dev(x, "x", torch.bfloat16), _dev(weight, "weight", wdt),
                                            _opt(scales, "scales"), _opt(bias, "bias", torch.bfloat16),
                                            _opt(residual, "residual", torch.bfloat16), _dev(y, "y", torch.bfloat16),
                                            M, N, K, group, fmt, ws, nws, _stream()))
    return y


def q4_gemm_swiglu(x, w1, s1, w2, s2, N, K, group, fmt, *, out=None):
    """G (M, N) = bf16(silu(bf16(X W1^T))) * bf16(X W2^T) in one launch (LLaMAMLP fc_1 / fc_2 / silu*mul)."""
    M = x.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    wdt = torch.bfloat16 if fmt == 2 else torch.uint8
    ws, nws = _q4f_workspace(M, N, K, True, x.device)
    _check(load_library().lga_q4_gemm_swiglu(_dev(x, "x", torch.bfloat16), _dev(w1, "w1", wdt), _opt(s1, "s1"),
                                             _dev(w2, "w2", wdt), _opt(s2, "s2"), _dev(y, "y", torch.bfloat16),
                                             M, N, K, group, fmt, ws, nws, _stream()))
    return y


def q4_dequantize(qweight, scales, N, K, group, fmt, *, out=None):
    """W (N, K) bf16 = bf16(value(nibble) * scale): the bits lga_q4_gemm stages (bnb dequantize_4bit)."""
    w = out if out is not None else torch.empty(N, K, dtype=torch.bfloat16, device=qweight.device)
    if w.numel() < N * K:
        raise ValueError(f"q4_dequantize: out holds {w.numel()} elements, needs {N * K}")
    _check(load_library().lga_q4_dequantize(_dev(qweight, "qweight", torch.uint8), _dev(scales, "scales"),
                                            _dev(w, "w", torch.bfloat16), N, K, group, fmt, _stream()))
    return w[: N * K].view(N, K) if w.dim() == 1 else w


def bf16_gemv(x, weight, *, bias=None, residual=None, norm_weight=None, eps=1e-5, out=None):
    """y (N,) = x (K,) . W (N, K)^T [+bias] [+residual] with bf16 weights; optional fused RMSNorm of x."""
    N, K = weight.shape
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_bf16_gemv(_dev(x, "x", torch.bfloat16), _dev(weight, "weight", torch.bfloat16),
                                        _opt(bias, "bias", torch.bfloat16), _opt(residual, "residual", torch.bfloat16),
                                        _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
                                        _dev(y, "y", torch.bfloat16), N, K, _stream()))
    return y


def bf16_gemv_swiglu(x, w1, w2, *, norm_weight=None, eps=1e-5, out=None):
    """y (N,) = bf16(silu(bf16(x W1^T))) * bf16(x W2^T) with bf16 weights, optional fused RMSNorm of x."""
    N, K = w1.shape
    if tuple(w2.shape) != (N, K):
        raise ValueError(f"bf16_gemv_swiglu: weight shapes differ {tuple(w1.shape)} vs {tuple(w2.shape)}")
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_bf16_gemv_swiglu(_dev(x, "x", torch.bfloat16), _dev(w1, "w1", torch.bfloat16),
                                               _dev(w2, "w2", torch.bfloat16),
                                               _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
                                               _dev(y, "y", torch.bfloat16), N, K, _stream()))
    return y


def bf16_gemm(x, weight, *, bias=None, residual=None, out=None):
    """Y (M, N) = X (M, K) . W (N, K)^T [+bias] [+residual] with bf16 weights on gemm.hip's MFMA tiles (bias and
    residual fused in its epilogue; the residual added after the product's bf16 rounding, as Block adds it)."""
    M = x.shape[0]
    N, K = weight.shape
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_bf16_gemm(_dev(x, "x", torch.bfloat16), _dev(weight, "weight", torch.bfloat16),
                                        _opt(bias, "bias", torch.bfloat16), _opt(residual, "residual", torch.bfloat16),
                                        _dev(y, "y", torch.bfloat16), M, N, K, _stream()))
    return y


# ------------------------------------------------------------------------------------------------ bnb.int8
INT8_THRESHOLD = 6.0  # bitsandbytes Linear8bitLt(threshold=6.0): |x| >= threshold marks an outlier column


def int8_quantize(weight: torch.Tensor):
    """(N, K) fp32/bf16 device weight -> (int8 (N, K), fp32 row absmax (N,)): q = rint(W * (127 / absmax))."""
    N, K = weight.shape
    w = weight.contiguous()
    if w.dtype not in (torch.float32, torch.bfloat16):
        w = w.float()
    qw = torch.empty(N, K, dtype=torch.int8, device=w.device)
    sc = torch.empty(N, dtype=torch.float32, device=w.device)
    _check(load_library().lga_int8_quantize(_dev(w, "weight"), int(w.dtype == torch.bfloat16), qw.data_ptr(),
                                            sc.data_ptr(), N, K, _stream()))
    return qw, sc


def int8_gemv(x, qweight, scales, *, bias=None, residual=None, norm_weight=None, eps=1e-5,
              threshold=INT8_THRESHOLD, out=None):
    """y (N,) = x (K,) against the LLM.int8 weight: x quantized per call, outlier elements (|x| >= threshold) kept in
    bf16 [+bias] [+residual]; optional fused RMSNorm of x."""
    N, K = qweight.shape
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_int8_gemv(_dev(x, "x", torch.bfloat16), _dev(qweight, "qweight", torch.int8),
                                        _dev(scales, "scales", torch.float32), _opt(bias, "bias", torch.bfloat16),
                                        _opt(residual, "residual", torch.bfloat16),
                                        _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps), float(threshold),
                                        _dev(y, "y", torch.bfloat16), N, K, _stream()))
    return y


def int8_gemv_swiglu(x, qw1, sc1, qw2, sc2, *, norm_weight=None, eps=1e-5, threshold=INT8_THRESHOLD, out=None):
    """y (N,) = bf16(silu(bf16(x W1^T))) * bf16(x W2^T) with LLM.int8 weights (one activation quantization for
    both), optional fused RMSNorm of x."""
    N, K = qw1.shape
    if tuple(qw2.shape) != (N, K):
        raise ValueError(f"int8_gemv_swiglu: weight shapes differ {tuple(qw1.shape)} vs {tuple(qw2.shape)}")
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_int8_gemv_swiglu(_dev(x, "x", torch.bfloat16), _dev(qw1, "qw1", torch.int8),
                                               _dev(sc1, "sc1", torch.float32), _dev(qw2, "qw2", torch.int8),
                                               _dev(sc2, "sc2", torch.float32),
                                               _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
                                               float(threshold), _dev(y, "y", torch.bfloat16), N, K, _stream()))
    return y


def int8_quantize_act(x, *, threshold=INT8_THRESHOLD):
    """X (M, K) bf16 -> (xq int8 (M, K), sx fp32 (M,), cols int32 (K,), count int32 (1,), col_flags int32 (K,)):
    a column with any |x| >= threshold is an outlier column (flag 1, listed ascending in cols[:count], 0 in xq);
    sx is each row's absmax over the other columns. Everything stays on the device."""
    M, K = x.shape
    dev = x.device
    xq = torch.empty(M, K, dtype=torch.int8, device=dev)
    sx = torch.empty(M, dtype=torch.float32, device=dev)
    flags = torch.empty(K, dtype=torch.int32, device=dev)
    cols = torch.empty(K, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _check(load_library().lga_int8_quantize_act(_dev(x, "x", torch.bfloat16), xq.data_ptr(), sx.data_ptr(),
                                                flags.data_ptr(), cols.data_ptr(), count.data_ptr(), M, K,
                                                float(threshold), _stream()))
    return xq, sx, cols, count, flags


def int8_gemm(x, xq, sx, cols, count, qweight, scales, *, bias=None, residual=None, out=None):
    """Y (M, N) from int8_quantize_act's image of X against the LLM.int8 weight on the i8 MFMA: dequantized integer
    product + the outlier columns' bf16 term [+bias] [+residual]; M >= 2."""
    M, K = xq.shape
    N = qweight.shape[0]
    if tuple(qweight.shape) != (N, K) or tuple(x.shape) != (M, K):
        raise ValueError(f"int8_gemm: shapes x {tuple(x.shape)} xq {tuple(xq.shape)} qweight {tuple(qweight.shape)}")
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_int8_gemm(_dev(x, "x", torch.bfloat16), _dev(xq, "xq", torch.int8),
                                        _dev(sx, "sx", torch.float32), _dev(cols, "cols", torch.int32),
                                        _dev(count, "count", torch.int32), _dev(qweight, "qweight", torch.int8),
                                        _dev(scales, "scales", torch.float32), _opt(bias, "bias", torch.bfloat16),
                                        _opt(residual, "residual", torch.bfloat16), _dev(y, "y", torch.bfloat16),
                                        M, N, K, _stream()))
    return y


# ------------------------------------------------------------------------------------------------ LoRA
LORA_MAX_RANK = 64  # r after padding to a multiple of 8
LORA_MAX_ROWS = 192  # R: rows of A over all segments
LORA_MAX_K = 32768


def _lora_dims(A, B, row_off, name):
    """(N, K, R, r) of an adapter in the device layout (include/litgpt_amd.h), refusing what the kernels do not
    take."""
    (R, K), (N, r) = A.shape, B.shape
    if r % 8 or R % 8 or not 0 < r <= LORA_MAX_RANK or not r <= R <= LORA_MAX_ROWS or K % 8 or K > LORA_MAX_K:
        raise ValueError(f"{name}: adapter with r={r}, R={R}, K={K} is outside the kernels' limits (r % 8 == 0, "
                         f"r <= {LORA_MAX_RANK}, R % 8 == 0, R <= {LORA_MAX_ROWS}, K % 8 == 0, K <= {LORA_MAX_K})")
    if row_off is not None and row_off.numel() != N:
        raise ValueError(f"{name}: row_off holds {row_off.numel()} entries, B has {N} rows")
    if row_off is None and R != r:
        raise ValueError(f"{name}: A has {R} rows for r={r}: a segmented adapter needs row_off")
    return N, K, R, r


def lora_gemv(x, A, B, row_off, scaling, *, base=None, residual=None, norm_weight=None, eps=1e-5, out=None):
    """One row: y (N,) = [base +] bf16(bf16(B t) * scaling) [+ residual], t = bf16(A x'), x' = x or its RMSNorm — the
    whole chain in one launch (``out`` may be ``base``)."""
    N, K, R, r = _lora_dims(A, B, row_off, "lora_gemv")
    if x.numel() != K:
        raise ValueError(f"lora_gemv: x holds {x.numel()} elements, A has {K} columns")
    for name, v in (("base", base), ("residual", residual), ("out", out)):
        if v is not None and v.numel() != N:
            raise ValueError(f"lora_gemv: {name} holds {v.numel()} elements, B has {N} rows")
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_lora_gemv(_dev(x, "x", torch.bfloat16), _opt(norm_weight, "norm_weight", torch.bfloat16),
                                        float(eps), _dev(A, "A", torch.bfloat16), _dev(B, "B", torch.bfloat16),
                                        _opt(row_off, "row_off", torch.int32), float(scaling),
                                        _opt(base, "base", torch.bfloat16), _opt(residual, "residual", torch.bfloat16),
                                        _dev(y, "y", torch.bfloat16), N, K, R, r, _stream()))
    return y


def lora_gemv_rows(x, A, B, row_off, adapter, scaling, *, base, residual=None, norm_weight=None, eps=1e-5, out=None):
    """Up to ``MAX_GEMV_ROWS`` rows, each with its own adapter, in one launch (batched decode): x (M, K); A (n, R, K) and
    B (n, N, r) the stacked adapters; ``adapter`` (M,) int32 on the device, read by the kernel. Row m has the bits of
    ``lora_gemv(x[m], A[a], B[a], ...)`` for a = adapter[m]; an id outside [0, n) passes ``base`` (+ ``residual``)
    through. ``base`` (M, N) is required (``out`` may be ``base``)."""
    if A.dim() != 3 or B.dim() != 3 or A.shape[0] != B.shape[0]:
        raise ValueError(f"lora_gemv_rows: A {tuple(A.shape)} / B {tuple(B.shape)} must be stacked (n, R, K) / (n, N, r) "
                         "adapters of one set")
    n = A.shape[0]
    N, K, R, r = _lora_dims(A[0], B[0], row_off, "lora_gemv_rows")
    if x.dim() != 2 or x.shape[1] != K or not 1 <= x.shape[0] <= MAX_GEMV_ROWS:
        raise ValueError(f"lora_gemv_rows: x {tuple(x.shape)} must be (M, {K}) with 1 <= M <= {MAX_GEMV_ROWS}")
    M = x.shape[0]
    if adapter.numel() != M:
        raise ValueError(f"lora_gemv_rows: adapter holds {adapter.numel()} ids for {M} rows")
    if base is None:
        raise ValueError("lora_gemv_rows: base is required")
    for name, v in (("base", base), ("residual", residual), ("out", out)):
        if v is not None and v.numel() != M * N:
            raise ValueError(f"lora_gemv_rows: {name} holds {v.numel()} elements, expected {M} x {N}")
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_lora_gemv_rows(
        _dev(x, "x", torch.bfloat16), _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps),
        _dev(A, "A", torch.bfloat16), _dev(B, "B", torch.bfloat16), _opt(row_off, "row_off", torch.int32),
        _dev(adapter, "adapter", torch.int32), n, R * K, N * r, float(scaling), _dev(base, "base", torch.bfloat16),
        _opt(residual, "residual", torch.bfloat16), _dev(y, "y", torch.bfloat16), M, N, K, R, r, _stream()))
    return y


def lora_down(x, A, out=None):
    """t (M, R) = bf16(x (M, K) . A (R, K)^T) on the MFMA (prefill)."""
    M, K = x.shape
    R = A.shape[0]
    if A.shape[1] != K or K % 8 or K > LORA_MAX_K or R % 8 or not 0 < R <= LORA_MAX_ROWS:
        raise ValueError(f"lora_down: x {tuple(x.shape)} against A {tuple(A.shape)} is outside the kernel's limits "
                         f"(K % 8 == 0, K <= {LORA_MAX_K}, R % 8 == 0, R <= {LORA_MAX_ROWS})")
    t = out if out is not None else torch.empty(M, R, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_lora_down(_dev(x, "x", torch.bfloat16), _dev(A, "A", torch.bfloat16),
                                        _dev(t, "t", torch.bfloat16), M, K, R, _stream()))
    return t


def lora_up(t, B, row_off, scaling, *, base=None, residual=None, out=None):
    """y (M, N) = [base +] bf16(bf16(t B^T per segment) * scaling) [+ residual] (``out`` may be ``base``)."""
    M, R = t.shape
    N, r = B.shape
    if r % 8 or R % 8 or not 0 < r <= LORA_MAX_RANK or not r <= R <= LORA_MAX_ROWS:
        raise ValueError(f"lora_up: r={r}, R={R} is outside the kernel's limits")
    if (row_off is None and R != r) or (row_off is not None and row_off.numel() != N):
        raise ValueError("lora_up: row_off must hold one entry per row of B (and is needed when R != r)")
    for name, v in (("base", base), ("residual", residual), ("out", out)):
        if v is not None and v.numel() != M * N:
            raise ValueError(f"lora_up: {name} holds {v.numel()} elements, expected {M} x {N}")
    y = out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=t.device)
    _check(load_library().lga_lora_up(_dev(t, "t", torch.bfloat16), _dev(B, "B", torch.bfloat16),
                                      _opt(row_off, "row_off", torch.int32), float(scaling),
                                      _opt(base, "base", torch.bfloat16), _opt(residual, "residual", torch.bfloat16),
                                      _dev(y, "y", torch.bfloat16), M, N, R, r, _stream()))
    return y


def lora_merge(weight, A, B, row_off, scaling):
    """In place on the bf16 weight (N, K): W = bf16(W + bf16(bf16(B A per segment) * scaling)); returns it."""
    N, K, R, r = _lora_dims(A, B, row_off, "lora_merge")
    if tuple(weight.shape) != (N, K):
        raise ValueError(f"lora_merge: weight {tuple(weight.shape)} against an adapter for ({N}, {K})")
    _check(load_library().lga_lora_merge(_dev(weight, "weight", torch.bfloat16), _dev(A, "A", torch.bfloat16),
                                         _dev(B, "B", torch.bfloat16), _opt(row_off, "row_off", torch.int32),
                                         float(scaling), N, K, R, r, _stream()))
    return weight


# ------------------------------------------------------------------------------------------------ row ops
def rmsnorm(x, weight, eps, out=None):
    n = x.shape[-1]
    rows = x.numel() // n
    y = out if out is not None else torch.empty_like(x)
    _check(load_library().lga_rmsnorm(_dev(x, "x", torch.bfloat16), _dev(weight, "weight", torch.bfloat16),
                                      _dev(y, "y", torch.bfloat16), rows, n, float(eps), _stream()))
    return y


def rope_kv_append(qkv, k_cache, v_cache, cache_pos, rope_pos, cos, sin, n_head, n_query_groups, head_size,
                   rope_n_elem, q_out=None):
    """qkv (T, (H+2G)*hs) -> q (T, H, hs) roped with cos/sin rows rope_pos; k (roped) and v written into the
    (G, max_seq, hs) caches at rows cache_pos."""
    T = qkv.shape[0]
    max_seq = k_cache.shape[-2]
    q = q_out if q_out is not None else torch.empty(T, n_head, head_size, dtype=qkv.dtype, device=qkv.device)
    if qkv.dtype == torch.float32:  # --precision 32-true (csrc/fp32.hip)
        _check(load_library().lga_f32_rope_kv_append(
            _dev(qkv, "qkv", torch.float32), _dev(q, "q", torch.float32), _dev(k_cache, "k_cache", torch.float32),
            _dev(v_cache, "v_cache", torch.float32), _dev(cache_pos, "cache_pos", torch.int64),
            _dev(rope_pos, "rope_pos", torch.int64), _dev(cos, "cos", torch.float32), _dev(sin, "sin", torch.float32),
            cos.shape[0], T, n_head, n_query_groups, head_size, rope_n_elem, max_seq, _stream()))
        return q
    _check(load_library().lga_rope_kv_append(
        _dev(qkv, "qkv", torch.bfloat16), _dev(q, "q", torch.bfloat16), _dev(k_cache, "k_cache", torch.bfloat16),
        _dev(v_cache, "v_cache", torch.bfloat16), _dev(cache_pos, "cache_pos", torch.int64),
        _dev(rope_pos, "rope_pos", torch.int64), _dev(cos, "cos", torch.float32), _dev(sin, "sin", torch.float32),
        cos.shape[0], T, n_head, n_query_groups, head_size, rope_n_elem, max_seq, _stream()))
    return q


ATTN_COUNTER_STRIDE = 64  # uint32 per (row, group) arrival counter (kCounterStride in attention.hip)


class AttentionWorkspace:
    """Persistent split-attention scratch: fp32 partials + per-(row, group) arrival counters. The counters are
    zeroed once here; the kernel's last-arriving workgroup re-arms them, so the buffers are reusable across
    launches and HIP-graph replays (allocate before capture)."""

    def __init__(self, T: int, n_head: int, n_query_groups: int, head_size: int, n_splits: int, device) -> None:
        nbytes = load_library().lga_attention_workspace_bytes(T, n_head, head_size, n_splits)
        self.key = (T, n_head, n_query_groups, head_size, n_splits)
        self.partials = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device)
        # one counter per (row, query group, head slice): at most n_head of them per row (csrc/attention.hip
        # attn_hsplit deals a group's heads to up to q_per_kv workgroups when the groups are few)
        self.counters = torch.zeros(T * n_head * ATTN_COUNTER_STRIDE, dtype=torch.int32, device=device)


def attention(q, k_cache, v_cache, input_pos, n_head, n_query_groups, head_size, scale, n_splits=1,
              workspace: Optional[AttentionWorkspace] = None, out=None):
    """y (T, H*hs): causal attention of q (T, H, hs) over the (G, max_seq, hs) caches, keys <= input_pos[t]."""
    T = q.shape[0]
    max_seq = k_cache.shape[-2]
    y = out if out is not None else torch.empty(T, n_head * head_size, dtype=q.dtype, device=q.device)
    if q.dtype == torch.float32:  # --precision 32-true: one workgroup per (row, head), no splits (csrc/fp32.hip)
        _check(load_library().lga_f32_attention(
            _dev(q, "q", torch.float32), _dev(k_cache, "k_cache", torch.float32),
            _dev(v_cache, "v_cache", torch.float32), _dev(input_pos, "input_pos", torch.int64),
            _dev(y, "y", torch.float32), T, n_head, n_query_groups, head_size, max_seq, float(scale), _stream()))
        return y
    if n_splits > 1:
        if workspace is None or workspace.key != (T, n_head, n_query_groups, head_size, n_splits):
            workspace = AttentionWorkspace(T, n_head, n_query_groups, head_size, n_splits, q.device)
        ws, cnt = _dev(workspace.partials, "workspace", torch.float32), _dev(workspace.counters, "counters", torch.int32)
    else:
        ws = cnt = None
    _check(load_library().lga_attention(
        _dev(q, "q", torch.bfloat16), _dev(k_cache, "k_cache", torch.bfloat16),
        _dev(v_cache, "v_cache", torch.bfloat16), _dev(input_pos, "input_pos", torch.int64),
        _dev(y, "y", torch.bfloat16), ws, cnt, T, n_head, n_query_groups, head_size, max_seq, n_splits, float(scale),
        _stream()))
    return y


MAX_WINDOW_ROWS = 8  # rows per lga_attention_decode_window / lga_spec_accept launch
MAX_BATCH_ROWS = 8  # sequences per lga_attention_decode_batch launch (the rows GEMVs' MAX_GEMV_ROWS)


# ------------------------------------------------------------------------------------------ fp8 (e4m3) KV cache
# One sequence's cache is (k_codes, v_codes, k_scale, v_scale): codes (G, max_seq, 128) uint8, scales (G, max_seq)
# fp32 powers of two (include/litgpt_amd.h states the format); the batch forms take all slots at once, one more
# leading dimension on each.
def _kv8(cache, name, dims=3):
    kc, vc, ks, vs = cache
    if (kc.shape != vc.shape or kc.dim() != dims or kc.shape[-1] != 128 or ks.shape != kc.shape[:-1]
            or vs.shape != ks.shape):
        lead = "(G" if dims == 3 else "(slots, G"
        raise ValueError(f"{name}: an fp8 cache is codes {lead}, max_seq, 128) uint8 x 2 and scales {lead}, max_seq) "
                         f"fp32 x 2, got {tuple(kc.shape)}, {tuple(vc.shape)}, {tuple(ks.shape)}, {tuple(vs.shape)}")
    return (_dev(kc, "k_codes", torch.uint8), _dev(vc, "v_codes", torch.uint8), _dev(ks, "k_scale", torch.float32),
            _dev(vs, "v_scale", torch.float32))


def _attention_decode(form, qkv, cache, pos, rope_pos, cos, sin, n_head, n_query_groups, head_size, rope_n_elem, scale,
                      n_splits, workspace, out, active=None, prefix_len=None):
    """The seven ``attention_decode_*`` functions: ``form`` is "fused" (one row), "window" (M rows of one sequence from
    ``pos`` (1,)), "batch" (B sequences, ``pos`` (B,), the caches of all slots) or "shared" (B samples of one prompt at
    ``pos`` (1,) — their rope position too, ``rope_pos`` is not read — behind ``prefix_len`` (1,); bf16 only); ``cache`` is (k, v) bf16 or (k
    codes, v codes, k scales, v scales) fp8. Checks, workspace, one ``lga_attention_decode_*`` call; returns y."""
    H, G, hs = n_head, n_query_groups, head_size
    fp8 = len(cache) == 4
    name = f"attention_decode_{form}" + ("_kv8" if fp8 else "")
    rows, kc = qkv.shape[0], cache[0]
    R = {"fused": "T", "window": "M", "batch": "B", "shared": "B"}[form]
    slots = form in ("batch", "shared")  # the caches of all slots
    if form == "shared" and fp8:
        raise NotImplementedError("attention_decode_shared reads bf16 caches only")
    if form == "fused":
        if rows != 1:
            raise ValueError(f"{name} handles exactly one token (T = 1)")
    else:
        cap = MAX_WINDOW_ROWS if form == "window" else MAX_BATCH_ROWS
        if qkv.dim() != 2 or not 1 <= rows <= cap:
            raise ValueError(f"{name}: qkv must be ({R}, (H + 2G) * hs) with 1 <= {R} <= {cap}, got "
                             f"{tuple(qkv.shape)}")
        if qkv.shape[1] != (H + 2 * G) * hs:
            raise ValueError(f"{name}: qkv rows must hold (H + 2G) * hs values")
    if form == "window" and pos.numel() != 1:
        raise ValueError(f"{name}: pos0 holds one position (row r sits at pos0 + r)")
    if form == "shared":
        if pos.numel() != 1:
            raise ValueError(f"{name}: pos holds the one position all rows sit at, got {tuple(pos.shape)}")
        if prefix_len is None or prefix_len.numel() != 1:
            raise ValueError(f"{name}: prefix_len must be one int64 value on the device")
    if slots:
        if kc.dim() != 4 or kc.shape[0] < rows or kc.shape[1] != G:
            raise ValueError(f"{name}: the caches are the whole (slots >= B, G, max_seq, hs) tensors, got "
                             f"{tuple(kc.shape)} for B = {rows}")
        if form == "batch" and pos.numel() != rows:
            raise ValueError(f"{name}: pos holds one position per sequence ({rows}), got {tuple(pos.shape)}")
        if active is not None and (active.numel() != rows or active.dtype != torch.int32):
            raise ValueError(f"{name}: active must hold {rows} int32 flags")
        if cache[1].shape != kc.shape:
            raise ValueError(f"{name}: k_cache and v_cache must have one shape")
    if fp8:
        ptrs = _kv8(cache, name, 4 if slots else 3)
    else:
        ptrs = _dev(kc, "k_cache", torch.bfloat16), _dev(cache[1], "v_cache", torch.bfloat16)
    y = out if out is not None else torch.empty(rows, H * hs, dtype=torch.bfloat16, device=qkv.device)
    if y.numel() != rows * H * hs:
        raise ValueError(f"{name}: out must hold ({R}, H * hs) values")
    ws = cnt = None
    if n_splits > 1:
        key = (rows, H, G, hs, n_splits)
        if form == "fused":  # the one-row forms build what they need
            if workspace is None or workspace.key != key:
                workspace = AttentionWorkspace(*key, qkv.device)
        elif workspace is None:
            raise ValueError(f"{name}: split attention needs an AttentionWorkspace({R}, ...)")
        elif workspace.key != key:
            raise ValueError(f"{name}: workspace built for {workspace.key}, the call needs {key}")
        ws, cnt = _dev(workspace.partials, "workspace", torch.float32), _dev(workspace.counters, "counters", torch.int32)
    args = [_dev(qkv, "qkv", torch.bfloat16), *ptrs, _dev(pos, "pos", torch.int64)]
    if form != "window":  # (a window's rope positions are its cache positions, pos0 + r)
        args.append(_dev(prefix_len, "prefix_len", torch.int64) if form == "shared"
                    else _dev(rope_pos, "rope_pos", torch.int64))
    args += [_dev(cos, "cos", torch.float32), _dev(sin, "sin", torch.float32), cos.shape[0],
             _dev(y, "y", torch.bfloat16), ws, cnt]
    if form != "fused":
        args.append(rows)
    if slots:  # the slot strides (of the scale rows too), the idle flags
        args += [kc.stride(0)] + ([cache[2].stride(0)] if fp8 else []) + [_opt(active, "active", torch.int32)]
    _check(getattr(load_library(), "lga_" + name)(*args, H, G, hs, rope_n_elem, kc.shape[-2], n_splits, float(scale),
                                                  _stream()))
    return y


def attention_decode_fused(qkv, k_cache, v_cache, cache_pos, rope_pos, cos, sin, n_head, n_query_groups,
                           head_size, rope_n_elem, scale, n_splits=1, workspace: Optional[AttentionWorkspace] = None,
                           out=None):
    """One decode token: RoPE + KV-append + attention in one launch. qkv (1, (H+2G)*hs) is the fused projection
    row; returns y (1, H*hs) and leaves roped k / v stored in the caches at cache_pos[0]."""
    return _attention_decode("fused", qkv, (k_cache, v_cache), cache_pos, rope_pos, cos, sin, n_head, n_query_groups,
                             head_size, rope_n_elem, scale, n_splits, workspace, out)


def attention_decode_window(qkv, k_cache, v_cache, pos0, cos, sin, n_head, n_query_groups, head_size, rope_n_elem,
                            scale, n_splits=1, workspace: Optional[AttentionWorkspace] = None, out=None):
    """A speculative verify window: M = qkv.shape[0] (1..8) rows of ONE sequence at positions pos0[0] + r. RoPE +
    KV-append + decode attention; y (M, H*hs) and the caches end bit-identical to M successive
    ``attention_decode_fused`` calls with the same ``n_splits``. ``pos0`` (1,) int64 is read on the device."""
    return _attention_decode("window", qkv, (k_cache, v_cache), pos0, None, cos, sin, n_head, n_query_groups,
                             head_size, rope_n_elem, scale, n_splits, workspace, out)


def kv8_rope_append(qkv, cache, cache_pos, rope_pos, cos, sin, n_head, n_query_groups, head_size, rope_n_elem,
                    q_out=None):
    """``rope_kv_append`` into an fp8 cache: q (T, H, hs) roped; k (roped) and v quantized row by row into the codes
    and scales at rows cache_pos."""
    T = qkv.shape[0]
    ptrs = _kv8(cache, "kv8_rope_append")
    q = q_out if q_out is not None else torch.empty(T, n_head, head_size, dtype=torch.bfloat16, device=qkv.device)
    _check(load_library().lga_kv8_rope_append(
        _dev(qkv, "qkv", torch.bfloat16), _dev(q, "q", torch.bfloat16), *ptrs,
        _dev(cache_pos, "cache_pos", torch.int64), _dev(rope_pos, "rope_pos", torch.int64),
        _dev(cos, "cos", torch.float32), _dev(sin, "sin", torch.float32), cos.shape[0], T, n_head, n_query_groups,
        head_size, rope_n_elem, cache[0].shape[-2], _stream()))
    return q


def kv8_dequantize(cache, n=None, out=None):
    """Rows [0, n) (default: all) of an fp8 cache as bf16 (k, v), each (G, n, 128): float(code) * scale, exact."""
    ptrs = _kv8(cache, "kv8_dequantize")
    G, S, hs = cache[0].shape
    n = S if n is None else n
    if out is None:
        out = (torch.empty(G, n, hs, dtype=torch.bfloat16, device=cache[0].device),
               torch.empty(G, n, hs, dtype=torch.bfloat16, device=cache[0].device))
    if out[0].numel() != G * n * hs or out[1].numel() != G * n * hs:
        raise ValueError("kv8_dequantize: out must hold two (G, n, 128) bf16 buffers")
    _check(load_library().lga_kv8_dequantize(*ptrs, _dev(out[0], "k_out", torch.bfloat16),
                                             _dev(out[1], "v_out", torch.bfloat16), G, n, hs, S, _stream()))
    return out


def attention_decode_fused_kv8(qkv, cache, cache_pos, rope_pos, cos, sin, n_head, n_query_groups, head_size,
                               rope_n_elem, scale, n_splits=1, workspace: Optional[AttentionWorkspace] = None,
                               out=None):
    """``attention_decode_fused`` over an fp8 cache: the new row is quantized into the cache at cache_pos[0] and every
    key and value, the new one included, is read as the cache holds it."""
    return _attention_decode("fused", qkv, tuple(cache), cache_pos, rope_pos, cos, sin, n_head, n_query_groups,
                             head_size, rope_n_elem, scale, n_splits, workspace, out)


def attention_decode_window_kv8(qkv, cache, pos0, cos, sin, n_head, n_query_groups, head_size, rope_n_elem, scale,
                                n_splits=1, workspace: Optional[AttentionWorkspace] = None, out=None):
    """``attention_decode_window`` over an fp8 cache: y (M, H*hs), codes and scales bit-identical to M successive
    ``attention_decode_fused_kv8`` calls with the same ``n_splits``."""
    return _attention_decode("window", qkv, tuple(cache), pos0, None, cos, sin, n_head, n_query_groups, head_size,
                             rope_n_elem, scale, n_splits, workspace, out)


def attention_decode_batch(qkv, k_cache, v_cache, pos, cos, sin, n_head, n_query_groups, head_size, rope_n_elem,
                           scale, n_splits=1, workspace: Optional[AttentionWorkspace] = None, active=None, out=None):
    """One decode token of each of B = qkv.shape[0] (1..8) sequences in ONE launch. ``k_cache`` / ``v_cache`` are the
    whole (slots, G, max_seq, hs) tensors, row b owns slot b and sits at ``pos[b]`` (cache and rope position, (B,)
    int64 read on the device). y (B, H*hs) and slot b end bit-identical to ``attention_decode_fused`` on that row and
    slot with the same ``n_splits``. ``active`` (B,) int32: a row with active[b] == 0 is idle (y[b] = 0, slot b
    untouched); None runs every row."""
    return _attention_decode("batch", qkv, (k_cache, v_cache), pos, pos, cos, sin, n_head, n_query_groups, head_size,
                             rope_n_elem, scale, n_splits, workspace, out, active)


def attention_decode_shared(qkv, k_cache, v_cache, pos, prefix_len, cos, sin, n_head, n_query_groups, head_size,
                            rope_n_elem, scale, n_splits=1, workspace: Optional[AttentionWorkspace] = None, active=None,
                            out=None):
    """One decode token of each of B = qkv.shape[0] (1..8) samples of ONE prompt in one launch: every row sits at
    ``pos[0]`` and the keys below ``prefix_len[0]`` (both (1,) int64, read on the device) are held by slot 0 alone. Row b
    reads them there, its own later keys in slot b, and appends to slot b. y (B, H*hs) and row pos[0] of every slot are
    bit-identical to ``attention_decode_batch`` on caches whose slot b holds slot 0's prefix rows; those rows of slots
    1.. are never touched. ``active`` as in the batch form. bf16 caches only."""
    return _attention_decode("shared", qkv, (k_cache, v_cache), pos, pos, cos, sin, n_head, n_query_groups,
                             head_size, rope_n_elem, scale, n_splits, workspace, out, active, prefix_len)


def attention_decode_batch_kv8(qkv, cache, pos, cos, sin, n_head, n_query_groups, head_size, rope_n_elem, scale,
                               n_splits=1, workspace: Optional[AttentionWorkspace] = None, active=None, out=None):
    """``attention_decode_batch`` over an fp8 cache: ``cache`` is the whole (k codes, v codes, k scales, v scales),
    codes (slots, G, max_seq, 128) uint8 and scales (slots, G, max_seq) fp32. Row b's y, codes and scales are
    bit-identical to ``attention_decode_fused_kv8`` on that row and slot with the same ``n_splits``."""
    return _attention_decode("batch", qkv, tuple(cache), pos, pos, cos, sin, n_head, n_query_groups, head_size,
                             rope_n_elem, scale, n_splits, workspace, out, active)


ADAPTER_MAX_KEYS = 64  # adapter_prompt_length of one lga_adapter_attention launch (a lane per key)
ADAPTER_MAX_HEAD_SIZE = 256
ADAPTER_POS_MODES = {"rows": 0, "window": 1, "one": 2}


def adapter_attention(y, qkv, ak, av, gating, pos, cos, sin, n_head, n_query_groups, head_size, rope_n_elem, scale, *,
                      pos_mode="rows", active=None):
    """LLaMA-Adapter v1's gated prefix-attention term, in place on ``y`` (T, H * hs) bf16: y[t, h] = bf16(y[t, h] +
    bf16(g_h * bf16(softmax(scale * rope(q[t, h]) ak^T) av))) over the aT keys of ``ak`` / ``av`` (G, aT, hs) —
    one ``lga_adapter_attention`` launch (include/litgpt_amd.h states the rounding points). ``qkv`` (T, (H + 2G) * hs)
    is the fused projection, q un-roped; ``cos`` / ``sin`` the fp32 tables; ``pos`` int64 on the device: ``pos_mode``
    "rows" one position per row (T,), "window" row t at pos[0] + t, "one" every row at pos[0]. ``active`` (T,) int32:
    rows flagged 0 keep their bits. Returns ``y``."""
    H, G, hs = n_head, n_query_groups, head_size
    if qkv.dim() != 2 or qkv.shape[1] != (H + 2 * G) * hs:
        raise ValueError(f"adapter_attention: qkv must be (T, (H + 2G) * hs), got {tuple(qkv.shape)}")
    T = qkv.shape[0]
    if y.numel() != T * H * hs:
        raise ValueError(f"adapter_attention: y must hold (T, H * hs) = ({T}, {H * hs}) values")
    if ak.dim() != 3 or ak.shape[0] != G or ak.shape[2] != hs or av.shape != ak.shape:
        raise ValueError(f"adapter_attention: ak and av must be (G, aT, hs) = ({G}, aT, {hs}), got {tuple(ak.shape)} "
                         f"and {tuple(av.shape)}")
    if gating.numel() != H:
        raise ValueError(f"adapter_attention: gating must hold one factor per head ({H})")
    if pos_mode not in ADAPTER_POS_MODES:
        raise ValueError(f"adapter_attention: pos_mode must be one of {sorted(ADAPTER_POS_MODES)}")
    if pos.numel() != (T if pos_mode == "rows" else 1):
        raise ValueError(f"adapter_attention: pos_mode {pos_mode!r} takes {T if pos_mode == 'rows' else 1} "
                         f"position(s), got {tuple(pos.shape)}")
    if active is not None and active.numel() != T:
        raise ValueError(f"adapter_attention: active must hold {T} int32 flags")
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != rope_n_elem:
        raise ValueError(f"adapter_attention: cos / sin must be (rows, rope_n_elem = {rope_n_elem}) tables")
    _check(load_library().lga_adapter_attention(
        _dev(qkv, "qkv", torch.bfloat16), _dev(ak, "ak", torch.bfloat16), _dev(av, "av", torch.bfloat16),
        _dev(gating, "gating", torch.bfloat16), _dev(cos, "cos", torch.float32), _dev(sin, "sin", torch.float32),
        cos.shape[0], _dev(pos, "pos", torch.int64), ADAPTER_POS_MODES[pos_mode], _opt(active, "active", torch.int32),
        _dev(y, "y", torch.bfloat16), T, H, G, hs, rope_n_elem, ak.shape[1], float(scale), _stream()))
    return y


def spec_accept(logits, window, out=None, token_inout=None, pos_inout=None):
    """Greedy speculative acceptance in one launch. logits (M, n) bf16, window (M,) int32 (window[0] the last emitted
    token, window[1:] the drafts): t_r = argmax(logits[r]) in ``argmax``'s order, a = the number of leading drafts
    with window[r + 1] == t_r. Returns out (M + 1,) int32 = [a, t_0 .. t_a, -1 ...]; ``token_inout`` (1,) int32
    receives t_a and ``pos_inout`` (1,) int64 advances by a + 1."""
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= MAX_WINDOW_ROWS:
        raise ValueError(f"spec_accept: logits must be (M, n) with 1 <= M <= {MAX_WINDOW_ROWS}, "
                         f"got {tuple(logits.shape)}")
    M, n = logits.shape
    if window.numel() != M:
        raise ValueError(f"spec_accept: window holds {window.numel()} tokens for {M} rows of logits")
    lp = _dev(logits, "logits", torch.bfloat16)
    res = out if out is not None else torch.empty(M + 1, dtype=torch.int32, device=logits.device)
    if res.numel() < M + 1:
        raise ValueError("spec_accept: out needs M + 1 int32 values")
    _check(load_library().lga_spec_accept(lp, M, n, _dev(window, "window", torch.int32), _dev(res, "out", torch.int32),
                                          _opt(token_inout, "token_inout", torch.int32),
                                          _opt(pos_inout, "pos_inout", torch.int64), _stream()))
    return res


class HeadWorkspace:
    """Scratch of the fused greedy head (lga_q4_gemv_argmax_embed): per-workgroup winners + arrival counters,
    zeroed once; the kernel re-arms its counters, so it is reusable across launches and graph replays."""

    def __init__(self, N: int, K: int, device) -> None:
        nbytes = load_library().lga_q4_gemv_argmax_work_bytes(N, K)
        self.key = (N, K)
        self.buf = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=device)


def q4_gemv_argmax_embed(x, lin, work: HeadWorkspace, *, norm_weight=None, eps=1e-5, table=None, emb_out=None,
                         logits=None, out_idx=None, token_out=None, pos_inout=None):
    """Greedy decode head in one launch: logits = lm_head(RMSNorm(x)), token = argmax(logits) (torch.argmax order),
    the lga_argmax_embed bookkeeping (token_out, out_idx, pos_inout += 1, table row -> emb_out). Returns logits."""
    N, K = lin.out_features, lin.in_features
    logits = logits if logits is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    V, C = (table.shape if table is not None else (0, 0))
    _check(load_library().lga_q4_gemv_argmax_embed(
        _dev(x.reshape(-1), "x", torch.bfloat16), _dev(lin.qweight, "qweight", torch.uint8), _dev(lin.scales, "scales"),
        _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps), _dev(logits, "logits", torch.bfloat16), N, K,
        lin.group, lin.fmt, _dev(work.buf, "work"), _opt(out_idx, "out_idx", torch.int64),
        _opt(token_out, "token_out", torch.int32), _opt(pos_inout, "pos_inout", torch.int64),
        _opt(table, "table", torch.bfloat16), C, V, _opt(emb_out, "emb_out", torch.bfloat16), _stream()))
    return logits


def preload_kernels() -> None:
    """Build the prefill path's kernel objects now (model load) rather than at their first launch
    (lga_preload_kernels; nothing runs on the GPU)."""
    _check(load_library().lga_preload_kernels())


_N_CU = None


def num_cus() -> int:
    """Compute units of the current device (lga_device_info)."""
    global _N_CU
    if _N_CU is None:
        n = ctypes.c_int(0)
        arch = ctypes.create_string_buffer(64)
        _check(load_library().lga_device_info(torch.cuda.current_device(), ctypes.byref(n), arch, 64))
        _N_CU = int(n.value)
    return _N_CU


def decode_fusable(head_size: int, rope_n_elem: int) -> bool:
    """Whether lga_attention_decode_fused covers this geometry (full rotary over 128-dim heads)."""
    return head_size == 128 and rope_n_elem == 128


def decode_splits(n_query_groups: int, q_per_kv: int, head_size: int, max_seq: int, n_cu: int = 256) -> int:
    """Sequence splits for T = 1 attention: one workgroup per CU across all query groups, at most 16 splits
    (tools/attn_sweep.py on MI355X, p = 2048..4000: 8 splits beat 16 for Llama-2-7B's 32 groups; with the few
    groups per rank of tensor parallelism 16 splits beat 32/64/128 — G = 4: 7.8 vs 10.9 us at 64 splits; G = 1,
    8 heads per group: 21 vs 34 us at 64 — because the last-arriving split's combine grows with the split count).
    Caches of >= 12k rows (a long prompt: generate/base.py sizes the cache to prompt + new tokens) take up to 32:
    with the log2-domain softmax, Mixtral 18.6 vs 19.3 us at p = 16000 and 28.4 vs 31.3 at 32066, its TP = 2 rank
    13.8 vs 14.9 and 20.3 vs 24.4; at 8000 16 still wins for Mixtral (13.0 vs 14.4) and ties at TP = 2
    (tools/attn_ab.py interleaved, round 5, profiles/r05z_attn_long_context.txt)."""
    s = max(1, min(n_cu // max(1, n_query_groups), 32 if max_seq >= 12288 else 16))
    return min(s, max(1, max_seq // 16), 256)


def embedding(idx, table, out=None):
    """out[t] = table[idx[t]]; bf16 or fp32 rows (fp32 rows move as pairs of 16-bit words: a byte copy)."""
    T = idx.numel()
    V, C = table.shape
    y = out if out is not None else torch.empty(T, C, dtype=table.dtype, device=table.device)
    if idx.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"embedding: idx must be int32/int64, got {idx.dtype}")
    if table.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"embedding: table must be bf16 or fp32, got {table.dtype}")
    words = C * (2 if table.dtype == torch.float32 else 1)
    _check(load_library().lga_embedding(_dev(idx, "idx"), int(idx.dtype == torch.int64),
                                        _dev(table, "table", table.dtype), _dev(y, "y", table.dtype), T, words, V,
                                        _stream()))
    return y


def add(a, b, out=None):
    y = out if out is not None else torch.empty_like(a)
    if a.dtype == torch.float32:
        _check(load_library().lga_f32_add(_dev(a, "a", torch.float32), _dev(b, "b", torch.float32),
                                          _dev(y, "y", torch.float32), a.numel(), _stream()))
        return y
    _check(load_library().lga_add(_dev(a, "a", torch.bfloat16), _dev(b, "b", torch.bfloat16),
                                  _dev(y, "y", torch.bfloat16), a.numel(), _stream()))
    return y


def layernorm(x, weight, bias, eps, out=None):
    """torch.nn.LayerNorm over the last dim of a contiguous bf16 GPU tensor (GPT-NeoX)."""
    n = x.shape[-1]
    y = out if out is not None else torch.empty_like(x)
    if x.dtype == torch.float32:
        _check(load_library().lga_f32_layernorm(_dev(x, "x", torch.float32), _dev(weight, "weight", torch.float32),
                                                _opt(bias, "bias", torch.float32), _dev(y, "y", torch.float32),
                                                x.numel() // n, n, float(eps), _stream()))
        return y
    _check(load_library().lga_layernorm(_dev(x, "x", torch.bfloat16), _dev(weight, "weight", torch.bfloat16),
                                        _opt(bias, "bias", torch.bfloat16), _dev(y, "y", torch.bfloat16),
                                        x.numel() // n, n, float(eps), _stream()))
    return y


def gelu(a, approximate: str = "none", out=None):
    """bf16(F.gelu(a, approximate)) (GptNeoxMLP)."""
    if approximate not in ("none", "tanh"):
        raise ValueError(f"gelu approximate must be 'none' or 'tanh', got {approximate!r}")
    y = out if out is not None else torch.empty_like(a)
    if a.dtype == torch.float32:
        _check(load_library().lga_f32_gelu(_dev(a, "a", torch.float32), _dev(y, "y", torch.float32), a.numel(),
                                           int(approximate == "tanh"), _stream()))
        return y
    _check(load_library().lga_gelu(_dev(a, "a", torch.bfloat16), _dev(y, "y", torch.bfloat16), a.numel(),
                                   int(approximate == "tanh"), _stream()))
    return y


def swiglu(a, b, out=None):
    y = out if out is not None else torch.empty_like(a)
    _check(load_library().lga_swiglu(_dev(a, "a", torch.bfloat16), _dev(b, "b", torch.bfloat16),
                                     _dev(y, "y", torch.bfloat16), a.numel(), _stream()))
    return y


def argmax(logits, out_idx=None, token_out=None, pos_inout=None):
    """Greedy token (lowest index on ties); optionally writes the token buffer and advances input_pos."""
    n = logits.numel()
    idx = out_idx if out_idx is not None else torch.empty(1, dtype=torch.int64, device=logits.device)
    if logits.dtype == torch.float32:
        _check(load_library().lga_argmax_f32(_dev(logits, "logits", torch.float32), n,
                                             _dev(idx, "out_idx", torch.int64), _opt(token_out, "token_out", torch.int32),
                                             _opt(pos_inout, "pos_inout", torch.int64), _stream()))
        return idx
    _check(load_library().lga_argmax(_dev(logits, "logits", torch.bfloat16), n, _dev(idx, "out_idx", torch.int64),
                                     _opt(token_out, "token_out", torch.int32),
                                     _opt(pos_inout, "pos_inout", torch.int64), _stream()))
    return idx


def f32_linear(x, weight, bias=None, residual=None, out=None):
    """y (M, N) = x (M, K) . W (N, K)^T (+ bias) (+ residual), all fp32 (--precision 32-true, csrc/fp32.hip)."""
    N, K = weight.shape
    M = x.numel() // K
    y = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=x.device)
    _check(load_library().lga_f32_linear(_dev(x, "x", torch.float32), _dev(weight, "weight", torch.float32),
                                         _opt(bias, "bias", torch.float32), _opt(residual, "residual", torch.float32),
                                         _dev(y, "y", torch.float32), M, N, K, _stream()))
    return y


def argmax_embed(logits, table, emb_out, out_idx=None, token_out=None, pos_inout=None):
    """argmax (as ``argmax``) + the embedding row of the chosen token written to ``emb_out`` (n_embd,) bf16 in
    the same launch (the next decode step's input)."""
    n = logits.numel()
    V, C = table.shape
    if emb_out.numel() != C:
        raise ValueError(f"argmax_embed: emb_out holds {emb_out.numel()} elements, the table rows {C}")
    idx = out_idx if out_idx is not None else torch.empty(1, dtype=torch.int64, device=logits.device)
    _check(load_library().lga_argmax_embed(_dev(logits, "logits", torch.bfloat16), n, _dev(idx, "out_idx", torch.int64),
                                           _opt(token_out, "token_out", torch.int32),
                                           _opt(pos_inout, "pos_inout", torch.int64), _dev(table, "table", torch.bfloat16),
                                           C, V, _dev(emb_out, "emb_out", torch.bfloat16), _stream()))
    return idx


MAX_TOP_K = 1024  # lga_sample_topk keeps at most this many logits
MAX_SAMPLE_VOCAB = 65536  # ... out of at most this many (one workgroup holds them in LDS)


def sample_topk(logits, top_k, temperature, *, uniform=None, seed=0, counter=None, out_idx=None, token_out=None,
                pos_inout=None, table=None, emb_out=None, kept_out=None, probs_out=None):
    """generate/base.py:30-41 at temperature > 0 with top_k (1..1024) in ONE launch (csrc/sample.hip
    topk_sample_kernel): top-k (ties lowest index first), softmax(logits / temperature) in bf16, inverse-CDF draw.
    ``uniform`` (1,) fp32 on the device fixes the draw (tests); otherwise ``counter`` (1,) int64 on the device is the
    RNG state (hash of ``seed`` and the counter; advanced per call, so the launch replays in a HIP graph). With
    ``table``/``emb_out`` the chosen token's embedding row is gathered as ``argmax_embed`` does. Returns out_idx."""
    n = logits.numel()
    if not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(f"sample_topk: top_k must be in [1, {MAX_TOP_K}], got {top_k}")
    if uniform is None and counter is None:
        raise ValueError("sample_topk: needs uniform or an RNG counter")
    idx = out_idx if out_idx is not None else torch.empty(1, dtype=torch.int64, device=logits.device)
    V, C = (table.shape if table is not None else (0, 0))
    if emb_out is not None and (table is None or emb_out.numel() != C):
        raise ValueError("sample_topk: emb_out needs the embedding table and one row of it")
    _check(load_library().lga_sample_topk(
        _dev(logits, "logits", torch.bfloat16), n, int(top_k), float(temperature), _opt(uniform, "uniform", torch.float32),
        int(seed) & (2**64 - 1), _opt(counter, "counter", torch.int64), _dev(idx, "out_idx", torch.int64),
        _opt(token_out, "token_out", torch.int32), _opt(pos_inout, "pos_inout", torch.int64),
        _opt(table, "table", torch.bfloat16), C, V, _opt(emb_out, "emb_out", torch.bfloat16),
        _opt(kept_out, "kept_out", torch.int32), _opt(probs_out, "probs_out", torch.bfloat16), _stream()))
    return idx


_U64 = 2**64 - 1


def sampler_uniform(seed: int, n: int) -> float:
    """The uniform the device sampler uses for draw number ``n`` under ``seed`` (csrc/sample.hip draw_uniform), on
    the host: ``((mix64(seed ^ n * 0xD1B54A32D192ED03) >> 41) + 0.5) * 2**-23`` in 64-bit wrap-around arithmetic,
    mix64 the splitmix64 finaliser. 24 significant bits, so the value is exact in fp32 and lies in (0, 1)."""
    x = ((int(seed) & _U64) ^ (((int(n) & _U64) * 0xD1B54A32D192ED03) & _U64))
    x = (x + 0x9E3779B97F4A7C15) & _U64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _U64
    x ^= x >> 31
    return ((x >> 41) + 0.5) * 2.0**-23


def spec_accept_sample(logits, window, top_k, temperature, *, uniform=None, seed=0, counter=None, out=None,
                       token_inout=None, pos_inout=None, sampled=None):
    """``spec_accept`` under top-k sampling (csrc/sample.hip lga_spec_accept_sample). logits (M, n) bf16, window (M,)
    int32: t_r = the token ``sample_topk`` draws from logits[r] at ``top_k`` / ``temperature`` under ``uniform[r]``
    (``uniform`` (M,) fp32 on the device), or otherwise under draw number ``counter + r`` of ``seed`` (``counter``
    (1,) int64 on the device, the tokens sampled so far); a = the number of leading drafts with window[r + 1] == t_r.
    Returns out (M + 1,) int32 = [a, t_0 .. t_a, -1 ...]; ``token_inout`` receives t_a, ``pos_inout`` advances by
    a + 1 and so does ``counter``. The M rows are sampled by M concurrent workgroups, then one small launch accepts;
    ``sampled`` (8,) int32 is the scratch between the two (allocated when omitted)."""
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= MAX_WINDOW_ROWS:
        raise ValueError(f"spec_accept_sample: logits must be (M, n) with 1 <= M <= {MAX_WINDOW_ROWS}, "
                         f"got {tuple(logits.shape)}")
    M, n = logits.shape
    if not 0 < n <= MAX_SAMPLE_VOCAB:
        raise ValueError(f"spec_accept_sample: rows hold {n} logits, the sampler takes 1..{MAX_SAMPLE_VOCAB}")
    if window.numel() != M:
        raise ValueError(f"spec_accept_sample: window holds {window.numel()} tokens for {M} rows of logits")
    if not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(f"spec_accept_sample: top_k must be in [1, {MAX_TOP_K}], got {top_k}")
    if not temperature > 0.0:
        raise ValueError("spec_accept_sample: temperature must be > 0 (0 is spec_accept)")
    if uniform is None and counter is None:
        raise ValueError("spec_accept_sample: needs uniforms or an RNG counter")
    if uniform is not None and uniform.numel() != M:
        raise ValueError(f"spec_accept_sample: {uniform.numel()} uniforms for {M} rows of logits")
    lp = _dev(logits, "logits", torch.bfloat16)
    res = out if out is not None else torch.empty(M + 1, dtype=torch.int32, device=logits.device)
    if res.numel() < M + 1:
        raise ValueError("spec_accept_sample: out needs M + 1 int32 values")
    tmp = sampled if sampled is not None else torch.empty(MAX_WINDOW_ROWS, dtype=torch.int32, device=logits.device)
    if tmp.numel() < M:
        raise ValueError("spec_accept_sample: sampled needs one int32 per row")
    _check(load_library().lga_spec_accept_sample(
        lp, M, n, int(top_k), float(temperature), _opt(uniform, "uniform", torch.float32), int(seed) & _U64,
        _opt(counter, "counter", torch.int64), _dev(window, "window", torch.int32), _dev(tmp, "sampled", torch.int32),
        _dev(res, "out", torch.int32), _opt(token_inout, "token_inout", torch.int32),
        _opt(pos_inout, "pos_inout", torch.int64), _stream()))
    return res


def _nucleus_args(name: str, n: int, top_k, top_p, temperature, uniform, counter) -> int:
    """Shared argument checks of the nucleus ops; returns top_k as the C ABI takes it (None -> 0)."""
    if not 0 < n <= MAX_SAMPLE_VOCAB:
        raise ValueError(f"{name}: {n} logits, the sampler takes 1..{MAX_SAMPLE_VOCAB}")
    if top_k is not None and not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(f"{name}: top_k must be None or in [1, {MAX_TOP_K}], got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"{name}: top_p must be in (0, 1], got {top_p}")
    if not temperature > 0.0:
        raise ValueError(f"{name}: temperature must be > 0 (0 is greedy)")
    if uniform is None and counter is None:
        raise ValueError(f"{name}: needs uniform or an RNG counter")
    return 0 if top_k is None else int(top_k)


def sample_nucleus(logits, top_k, top_p, temperature, *, uniform=None, seed=0, counter=None, out_idx=None,
                   token_out=None, pos_inout=None, table=None, emb_out=None, kept_out=None, probs_out=None,
                   nucleus_out=None):
    """Nucleus (top-p) sampling in ONE launch (csrc/sample.hip kernel_sample_nucleus): over the top-k
    set (``top_k`` 1..1024) or the whole vocabulary (``top_k=None``), the value classes enter in descending order
    until their integer weight reaches ``top_p`` of the total, and the token is drawn from them in proportion to the
    bf16 softmax of ``logits / temperature``. ``uniform`` / ``seed`` / ``counter``, the bookkeeping outputs and the
    embedding gather as ``sample_topk``. ``kept_out`` (int32, top-k form), ``probs_out`` (bf16), ``nucleus_out``
    (uint8): the candidates in index order, their probabilities and nucleus flags (tests). Returns out_idx."""
    n = logits.numel()
    k = _nucleus_args("sample_nucleus", n, top_k, top_p, temperature, uniform, counter)
    idx = out_idx if out_idx is not None else torch.empty(1, dtype=torch.int64, device=logits.device)
    V, C = (table.shape if table is not None else (0, 0))
    if emb_out is not None and (table is None or emb_out.numel() != C):
        raise ValueError("sample_nucleus: emb_out needs the embedding table and one row of it")
    cand = min(k, n) if k else n
    for t, nm in ((kept_out, "kept_out"), (probs_out, "probs_out"), (nucleus_out, "nucleus_out")):
        if t is not None and t.numel() < cand:
            raise ValueError(f"sample_nucleus: {nm} needs {cand} entries")
    if kept_out is not None and not k:
        raise ValueError("sample_nucleus: kept_out belongs to the top-k form")
    _check(load_library().lga_sample_nucleus(
        _dev(logits, "logits", torch.bfloat16), n, k, float(top_p), float(temperature),
        _opt(uniform, "uniform", torch.float32), int(seed) & _U64, _opt(counter, "counter", torch.int64),
        _dev(idx, "out_idx", torch.int64), _opt(token_out, "token_out", torch.int32),
        _opt(pos_inout, "pos_inout", torch.int64), _opt(table, "table", torch.bfloat16), C, V,
        _opt(emb_out, "emb_out", torch.bfloat16), _opt(kept_out, "kept_out", torch.int32),
        _opt(probs_out, "probs_out", torch.bfloat16), _opt(nucleus_out, "nucleus_out", torch.uint8), _stream()))
    return idx


def spec_accept_sample_nucleus(logits, window, top_k, top_p, temperature, *, uniform=None, seed=0, counter=None,
                               out=None, token_inout=None, pos_inout=None, sampled=None):
    """``spec_accept_sample`` with each row drawn as ``sample_nucleus`` draws it at ``top_k`` (None: the whole
    vocabulary) / ``top_p`` / ``temperature`` (csrc/sample.hip lga_spec_accept_sample_nucleus)."""
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= MAX_WINDOW_ROWS:
        raise ValueError(f"spec_accept_sample_nucleus: logits must be (M, n) with 1 <= M <= {MAX_WINDOW_ROWS}, "
                         f"got {tuple(logits.shape)}")
    M, n = logits.shape
    k = _nucleus_args("spec_accept_sample_nucleus", n, top_k, top_p, temperature, uniform, counter)
    if window.numel() != M:
        raise ValueError(f"spec_accept_sample_nucleus: window holds {window.numel()} tokens for {M} rows of logits")
    if uniform is not None and uniform.numel() != M:
        raise ValueError(f"spec_accept_sample_nucleus: {uniform.numel()} uniforms for {M} rows of logits")
    lp = _dev(logits, "logits", torch.bfloat16)
    res = out if out is not None else torch.empty(M + 1, dtype=torch.int32, device=logits.device)
    if res.numel() < M + 1:
        raise ValueError("spec_accept_sample_nucleus: out needs M + 1 int32 values")
    tmp = sampled if sampled is not None else torch.empty(MAX_WINDOW_ROWS, dtype=torch.int32, device=logits.device)
    if tmp.numel() < M:
        raise ValueError("spec_accept_sample_nucleus: sampled needs one int32 per row")
    _check(load_library().lga_spec_accept_sample_nucleus(
        lp, M, n, k, float(top_p), float(temperature), _opt(uniform, "uniform", torch.float32), int(seed) & _U64,
        _opt(counter, "counter", torch.int64), _dev(window, "window", torch.int32), _dev(tmp, "sampled", torch.int32),
        _dev(res, "out", torch.int32), _opt(token_inout, "token_inout", torch.int32),
        _opt(pos_inout, "pos_inout", torch.int64), _stream()))
    return res


# ------------------------------------------------------------------------------------------------ scoring
def _rows(logits: torch.Tensor, name: str):
    if logits.dim() != 2 or logits.numel() == 0:
        raise ValueError(f"{name}: expected non-empty (rows, n) logits, got {tuple(logits.shape)}")
    return logits.shape


def token_logprobs(logits, targets, *, logprob_out=None, argmax_out=None):
    """(rows, n) bf16 or fp32 logits, (rows,) int32 targets -> (logprob fp32 (rows,), argmax int32 (rows,)):
    log_softmax(logits)[r, targets[r]] and torch.argmax of each row, one pass over the logits on the device
    (csrc/score.hip). A target outside [0, n) scores NaN."""
    rows, n = _rows(logits, "token_logprobs")
    if targets.numel() != rows:
        raise ValueError(f"token_logprobs: {targets.numel()} targets for {rows} rows")
    lp = logprob_out if logprob_out is not None else torch.empty(rows, dtype=torch.float32, device=logits.device)
    am = argmax_out if argmax_out is not None else torch.empty(rows, dtype=torch.int32, device=logits.device)
    if lp.numel() != rows or am.numel() != rows:
        raise ValueError(f"token_logprobs: outputs must hold {rows} elements")
    if logits.dtype == torch.float32:
        fn, dt = load_library().lga_token_logprobs_f32, torch.float32
    elif logits.dtype == torch.bfloat16:
        fn, dt = load_library().lga_token_logprobs, torch.bfloat16
    else:
        raise TypeError(f"token_logprobs: logits must be bf16 or fp32, got {logits.dtype}")
    _check(fn(_dev(logits, "logits", dt), rows, n, _dev(targets, "targets", torch.int32),
              _dev(lp, "logprob_out", torch.float32), _dev(am, "argmax_out", torch.int32), _stream()))
    return lp, am


def logits_kl(p, q, *, kl_out=None, agree_out=None):
    """Two (rows, n) bf16 logit matrices -> (kl fp32 (rows,), agree int32 (rows,)): KL(softmax(p) || softmax(q)) per
    row (not clamped) and whether the rows' argmax agree, one pass over both (csrc/score.hip)."""
    rows, n = _rows(p, "logits_kl")
    if tuple(q.shape) != (rows, n):
        raise ValueError(f"logits_kl: shapes differ {tuple(p.shape)} vs {tuple(q.shape)}")
    kl = kl_out if kl_out is not None else torch.empty(rows, dtype=torch.float32, device=p.device)
    ag = agree_out if agree_out is not None else torch.empty(rows, dtype=torch.int32, device=p.device)
    if kl.numel() != rows or ag.numel() != rows:
        raise ValueError(f"logits_kl: outputs must hold {rows} elements")
    _check(load_library().lga_logits_kl(_dev(p, "p", torch.bfloat16), _dev(q, "q", torch.bfloat16), rows, n,
                                        _dev(kl, "kl_out", torch.float32), _dev(ag, "agree_out", torch.int32),
                                        _stream()))
    return kl, ag


# ------------------------------------------------------------------------------------------------ sparse MoE
def moe_route(logits, k, ids=None, probs=None):
    """(T, E) bf16 router logits -> (ids (T, k) int32, probs (T, k) bf16): torch.topk (CPU tie order) + fp32
    softmax over the k values, cast to bf16 (lit_gpt/model.py:737-738)."""
    T, E = logits.shape
    ids = ids if ids is not None else torch.empty(T, k, dtype=torch.int32, device=logits.device)
    probs = probs if probs is not None else torch.empty(T, k, dtype=torch.bfloat16, device=logits.device)
    _check(load_library().lga_moe_route(_dev(logits, "logits", torch.bfloat16), T, E, k, _dev(ids, "ids", torch.int32),
                                        _dev(probs, "probs", torch.bfloat16), _stream()))
    return ids, probs


def moe_gate_route_fits(n_expert: int, K: int) -> bool:
    """Whether lga_moe_gate_route takes this router gate (E <= 8 rows, K <= 6144, K % 32 == 0)."""
    return 0 < n_expert <= 8 and K % 32 == 0 and 0 < K <= 6144


def moe_gate_route(x, qweight, scales, n_expert, K, group, fmt, k, *, norm_weight=None, eps=1e-5, ids=None,
                   probs=None):
    """One token: router logits = gate(x) (4-bit GEMV, optional fused RMSNorm) and their routing in ONE launch ->
    (ids (1, k) int32, probs (1, k) bf16), bit-identical to q4_gemv + moe_route (lit_gpt/model.py:736-738)."""
    ids = ids if ids is not None else torch.empty(1, k, dtype=torch.int32, device=x.device)
    probs = probs if probs is not None else torch.empty(1, k, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_moe_gate_route(_dev(x, "x", torch.bfloat16), _dev(qweight, "qweight", torch.uint8),
                                             _dev(scales, "scales"), _opt(norm_weight, "norm_weight", torch.bfloat16),
                                             float(eps), n_expert, K, group, fmt, k, _dev(ids, "ids", torch.int32),
                                             _dev(probs, "probs", torch.bfloat16), _stream()))
    return ids, probs


def experts_pair_supported(N: int, K: int, group: int, fmt: int) -> bool:
    """Whether lga_q4_gemv_experts_pair_combine covers this routed proj shape."""
    return bool(load_library().lga_q4_gemv_experts_pair_supported(N, K, group, fmt))


class ExpertsPairWorkspace:
    """Persistent scratch of lga_q4_gemv_experts_pair_combine for one MoE block (allocate before graph capture): the
    first-arriving slot's rows [2][N] bf16 and the per-row-block arrival counters (zeroed once, re-armed by the kernel)."""

    def __init__(self, N: int, device) -> None:
        self.scratch = torch.empty(2 * N, dtype=torch.bfloat16, device=device)
        self.counters = torch.zeros(int(load_library().lga_q4_gemv_experts_pair_counters(N)), dtype=torch.int32,
                                    device=device)


def q4_gemv_experts_pair_combine(x, qweight, scales, ids, probs, residual, N, K, group, fmt, ws, out=None):
    """One token, k = 2: y (N,) = residual + combine of the two routed proj GEMVs (slot s: x[s] against expert ids[s]
    of the (E, N, K/2) stack), bit-identical to q4_gemv_experts + moe_combine, in one launch."""
    if ids.numel() != 2 or probs.numel() != 2 or x.numel() != 2 * K or residual.numel() != N:
        raise ValueError("q4_gemv_experts_pair_combine: needs 2 slots (ids, probs, x of 2 x K) and a residual of N")
    y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
    ws_, ss_ = _expert_strides(qweight, scales)
    _check(load_library().lga_q4_gemv_experts_pair_combine(
        _dev(x, "x", torch.bfloat16), _dev(qweight, "qweight", torch.uint8), _dev(scales, "scales"),
        _dev(ids, "ids", torch.int32), _dev(probs, "probs", torch.bfloat16), _dev(residual, "residual", torch.bfloat16),
        qweight.size(0), ws_, ss_, _dev(y, "y", torch.bfloat16), _dev(ws.scratch, "scratch", torch.bfloat16),
        _dev(ws.counters, "counters", torch.int32), N, K, group, fmt, _stream()))
    return y


def _expert_strides(qweight, scales):
    if qweight.dim() != 3 or scales.dim() != 3:
        raise ValueError("expert weights must be stacked as (E, N, K/2) / (E, N, K/group)")
    return qweight.stride(0) * qweight.element_size(), scales.stride(0) * scales.element_size()


def q4_gemv_experts(x, qweight, scales, ids, N, K, group, fmt, *, out=None, variant=-1):
    """y (k, N): slot s = x[s] (k, K) . dequant(W[ids[s]])^T with W stacked (E, N, K/2)."""
    k = ids.numel()
    ws, ss = _expert_strides(qweight, scales)
    y = out if out is not None else torch.empty(k, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_q4_gemv_experts(_dev(x, "x", torch.bfloat16), _dev(qweight, "qweight", torch.uint8),
                                              _dev(scales, "scales"), _dev(ids, "ids", torch.int32), k,
                                              qweight.size(0), ws, ss, K, _dev(y, "y", torch.bfloat16), N, K, group,
                                              fmt, variant, _stream()))
    return y


def q4_gemv_swiglu_experts(x, qw1, sc1, qw2, sc2, ids, N, K, group, fmt, *, norm_weight=None, eps=1e-5, out=None,
                           variant=-1):
    """y (k, N): slot s = bf16(silu(bf16(x W1[ids[s]]^T))) * bf16(x W2[ids[s]]^T), optional fused RMSNorm of x."""
    k = ids.numel()
    ws, ss = _expert_strides(qw1, sc1)
    if _expert_strides(qw2, sc2) != (ws, ss):
        raise ValueError("fc_1 and fc_2 expert stacks must share one stride")
    y = out if out is not None else torch.empty(k, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_q4_gemv_swiglu_experts(
        _dev(x, "x", torch.bfloat16), _dev(qw1, "qw1", torch.uint8), _dev(sc1, "sc1"), _dev(qw2, "qw2", torch.uint8),
        _dev(sc2, "sc2"), _dev(ids, "ids", torch.int32), k, qw1.size(0), ws, ss,
        _opt(norm_weight, "norm_weight", torch.bfloat16), float(eps), _dev(y, "y", torch.bfloat16), N, K, group, fmt,
        variant, _stream()))
    return y


def moe_group(ids, n_expert, bm):
    """(T, k) int32 expert ids -> (tiles, x_rows, y_rows) of the grouped prefill GEMMs (lga_moe_group): the
    (token, slot) pairs sorted by expert on the device, m-tiles of ``bm`` rows; no host synchronisation."""
    T, k = ids.shape
    lib = load_library()
    cap = int(lib.lga_moe_group_tiles(T * k, int(n_expert), int(bm)))
    tiles = torch.empty(1 + 3 * cap, dtype=torch.int32, device=ids.device)
    x_rows = torch.empty(T * k, dtype=torch.int32, device=ids.device)
    y_rows = torch.empty(T * k, dtype=torch.int32, device=ids.device)
    _check(lib.lga_moe_group(_dev(ids, "ids", torch.int32), T, k, int(n_expert), int(bm), _dev(tiles, "tiles"),
                             _dev(x_rows, "x_rows"), _dev(y_rows, "y_rows"), _stream()))
    return tiles, x_rows, y_rows


def moe_grouped_bm(rows: int) -> int:
    """Tile height of the grouped prefill GEMMs for ``rows`` permuted rows (T * k)."""
    return 64 if rows <= 512 else 256


def q4_gemm_swiglu_grouped(x, w1, s1, w2, s2, tiles, x_rows, rows, N, K, group, fmt, bm, n_expert, *, out=None):
    """g (rows, N): permuted row r = bf16(silu(bf16(x[x_rows[r]] W1_e^T))) * bf16(x[x_rows[r]] W2_e^T), e the row's
    expert, W stacked (E, N, K/2) — every expert's rows in one launch."""
    ws, ss = _expert_strides(w1, s1)
    y = out if out is not None else torch.empty(rows, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_q4_gemm_swiglu_grouped(
        _dev(x, "x", torch.bfloat16), _dev(w1, "w1", torch.uint8), _dev(s1, "s1"), _dev(w2, "w2", torch.uint8),
        _dev(s2, "s2"), ws, ss, _dev(tiles, "tiles", torch.int32), _dev(x_rows, "x_rows", torch.int32),
        _dev(y, "y", torch.bfloat16), int(rows), int(N), int(K), int(group), int(fmt), int(bm), int(n_expert),
        _stream()))
    return y


def q4_gemm_grouped(x, w, s, tiles, y_rows, rows, N, K, group, fmt, bm, n_expert, *, x_rows=None, out=None):
    """y[y_rows[r]] = x[r] W_e^T for every permuted row r (x rows in permuted order unless ``x_rows``)."""
    ws, ss = _expert_strides(w, s)
    y = out if out is not None else torch.empty(rows, N, dtype=torch.bfloat16, device=x.device)
    _check(load_library().lga_q4_gemm_grouped(
        _dev(x, "x", torch.bfloat16), _dev(w, "w", torch.uint8), _dev(s, "s"), ws, ss,
        _dev(tiles, "tiles", torch.int32), _opt(x_rows, "x_rows", torch.int32), _opt(y_rows, "y_rows", torch.int32),
        _dev(y, "y", torch.bfloat16), int(rows), int(N), int(K), int(group), int(fmt), int(bm), int(n_expert),
        _stream()))
    return y


def moe_combine(expert_out, probs, ids, residual=None, out=None):
    """(T, k, C) expert outputs -> (T, C): [residual +] sum over slots in ascending expert id of bf16(p * E)."""
    T, k, C = expert_out.shape
    y = out if out is not None else torch.empty(T, C, dtype=torch.bfloat16, device=expert_out.device)
    _check(load_library().lga_moe_combine(_dev(expert_out, "expert_out", torch.bfloat16),
                                          _dev(probs, "probs", torch.bfloat16), _dev(ids, "ids", torch.int32),
                                          _opt(residual, "residual", torch.bfloat16), _dev(y, "y", torch.bfloat16),
                                          T, k, C, _stream()))
    return y
