"""Quantized Linears — the drop-ins for bitsandbytes' ``Linear4bit`` (4-bit weight-only) and ``Linear8bitLt``
(``bnb.int8``, LLM.int8) — and how a Linear of each weight format (4-bit, int8, bf16, fp32) runs on the kernels
(``_Kernels``, ``kernels``, ``swiglu``).

Reference boundary ("Operator boundary being replaced"): any object used where ``nn.Linear`` is
expected — ``forward(x[..., in_features]) -> y[..., out_features]`` with attributes ``weight``, ``bias``,
``in_features``, ``out_features``. The reference gets it from Lightning's ``BitsandbytesPrecision(mode, dtype)``
whose ``convert_module`` swaps every ``nn.Linear`` (lm_head included: ``ignore_modules`` is not passed,
generate/base.py:133) and quantizes on the move to the GPU (generate/base.py:128-136, 168; generate/tp.py:171,
190). ``QuantizedPrecision`` mirrors that: ``convert_module`` swaps the Linears of a (possibly TP-sharded,
still float) model for ``QuantLinear`` modules that quantize their weight on the device with the HIP quantizer.

Modes:
  "int4-g128" (also "int4-g64", "int4-g32")  symmetric int4, per-group bf16 scale (BASELINE config 3)
  "nf4"  / "bnb.nf4"                          NF4 codebook, fp32 absmax per 64 (bitsandbytes nf4 layout)
  "bnb.nf4-dq"                                nf4 + bitsandbytes double quantization of the absmax (offset =
                                              mean, 8-bit dynamic-map codes per 256 blocks, fp32 absmax2): the
                                              kernels scale by the dequantized statistic code[q]*absmax2+offset,
                                              held expanded as fp32 per 64-block (lga_nf4_double_quant)
  "bnb.fp4" / "bnb.fp4-dq"                    bitsandbytes FP4 code ({0, .0625, 8, 12, 4, 6, 2, 3} / 12, sign
                                              bit), fp32 absmax per 64 (+ the same double quantization)
  "bnb.int8"                                  LLM.int8 (``Int8Linear``): int8 weights with an fp32 absmax per row;
                                              activations quantized per call to int8 with an absmax per row,
                                              columns holding any |x| >= 6.0 kept in bf16 (the outlier
                                              decomposition of Linear8bitLt(has_fp16_weights=False,
                                              threshold=6.0), bf16 where bitsandbytes computes in fp16)
Group sizes must divide in_features; for a TP row-shard whose width is not a multiple of the requested group
(e.g. Llama-2-7B mlp.proj at TP=8: 1376) the largest of {128, 64, 32} that divides it is used.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from lit_gpt import ops

_DOUBLE_QUANT = {"bnb.nf4-dq", "bnb.fp4-dq"}
_CODE_CACHE = {}


def bnb_dynamic_map(device) -> torch.Tensor:
    """bitsandbytes create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8): the 256 sorted fp32 codes
    of the absmax double quantization (7 decades of 2^i linearly spaced means, +-, plus 0 and 1)."""
    key = str(device)
    if key not in _CODE_CACHE:
        data = []
        for i in range(7):
            b = torch.linspace(0.1, 1, 2 ** i + 1)
            means = ((b[:-1] + b[1:]) / 2.0) * (10 ** (-6 + i))
            data += means.tolist() + (-means).tolist()
        data += [0.0, 1.0]
        _CODE_CACHE[key] = torch.tensor(sorted(data), dtype=torch.float32, device=device)
    return _CODE_CACHE[key]


_MODES = {
    "int4-g128": (ops.FMT_Q4G, 128),
    "int4-g64": (ops.FMT_Q4G, 64),
    "int4-g32": (ops.FMT_Q4G, 32),
    "nf4": (ops.FMT_NF4, 64),
    "bnb.nf4": (ops.FMT_NF4, 64),
    "bnb.nf4-dq": (ops.FMT_NF4, 64),
    "bnb.fp4": (ops.FMT_FP4, 64),
    "bnb.fp4-dq": (ops.FMT_FP4, 64),
    "bnb.int8": (ops.FMT_INT8, 0),  # Int8Linear: one fp32 scale per row, no group
}


# the --quantize modes whose Linears the batched decode route (B > 1) runs
ROWS_MODES = "int4-g128/64/32, nf4, bnb.nf4, bnb.nf4-dq, bnb.fp4, bnb.fp4-dq"


def parse_mode(mode: str):
    if mode not in _MODES:
        raise NotImplementedError(
            f"quantize mode {mode!r} is not supported on this build (supported: {sorted(_MODES)})")
    return _MODES[mode]


def _fit_group(K: int, group: int) -> int:
    for g in (group, 128, 64, 32):
        if g <= group and K % g == 0:
            return g
    raise ValueError(f"in_features={K} is not a multiple of 32; no 4-bit group layout fits")


class _Kernels:
    """How a Linear of one weight format runs on the HIP kernels: ``forward`` and ``swiglu`` below
    alone decide between launches. A format supplies ``in_features`` / ``out_features`` / ``bias``, ``gemv`` (one
    row), ``gemm`` (several), ``gemv_swiglu`` (the dual one-row launch) and what differs from the defaults here.
    4-bit and int8 are the modules themselves; a plain ``nn.Linear`` stays one (``generate/tp.py`` and the
    reference API isinstance-check it) and is wrapped per call by ``kernels``."""

    act_dtype, expects = torch.bfloat16, "bf16 activations (bf16-true)"
    kind = property(lambda self: type(self).__name__)  # the Linear's name in error messages

    def forward(self, x: torch.Tensor, *, residual: Optional[torch.Tensor] = None,
                norm_weight: Optional[torch.Tensor] = None, norm_eps: float = 1e-5, rows: bool = False) -> torch.Tensor:
        """y = linear(x) [+ residual], x RMSNorm-ed first when ``norm_weight`` is given: in the one-row launch's
        prologue where it takes the norm, else as a separate ``lga_rmsnorm``. ``rows``: the batched decode route
        (GPT.forward with B > 1, T = 1) — the x rows are one token each of the batch's sequences (at most 8 rows) and
        go through ``gemv_rows``, whose row r has the bits ``gemv`` gives for x[r]; nothing else sets it."""
        if rows:
            return self._forward_rows(x, residual, norm_weight, norm_eps)
        lead = x.shape[:-1]
        x2 = x.reshape(-1, self.in_features)
        if x2.dtype != self.act_dtype:
            raise TypeError(f"{self.kind} expects {self.expects}, got {x2.dtype}")
        x2 = x2.contiguous()
        M = x2.shape[0]
        res = None if residual is None else residual.reshape(M, self.out_features).contiguous()
        if norm_weight is not None and (not self.gemv_fuses_norm() or M > 1):
            x2, norm_weight = ops.rmsnorm(x2, norm_weight, norm_eps), None
        y = self.gemv(x2, res, norm_weight, norm_eps) if M == 1 else self.gemm(x2, res)
        return y.view(*lead, self.out_features)

    def gemv_fuses_norm(self, dual: bool = False) -> bool:
        """Whether the one-row launch (``dual``: the SwiGLU pair's) takes the RMSNorm of a row of this K."""
        return True

    def _forward_rows(self, x, residual, norm_weight, norm_eps) -> torch.Tensor:
        lead = x.shape[:-1]
        x2 = x.reshape(-1, self.in_features)
        if x2.dtype != self.act_dtype:
            raise TypeError(f"{self.kind} expects {self.expects}, got {x2.dtype}")
        x2 = x2.contiguous()
        res = None if residual is None else residual.reshape(x2.shape[0], self.out_features).contiguous()
        if norm_weight is not None and not self.gemv_fuses_norm():
            x2, norm_weight = ops.rmsnorm(x2, norm_weight, norm_eps), None
        return self.gemv_rows(x2, res, norm_weight, norm_eps).view(*lead, self.out_features)

    def gemv_rows(self, x, res, norm_weight, eps):
        """Up to 8 rows in one pass over the weights (batched decode): the 4-bit formats have the kernel."""
        raise NotImplementedError(f"batched decode (batch size > 1) with a {self.kind}: the multi-row decode GEMV "
                                  f"streams 4-bit weights only ({ROWS_MODES})")

    def gemv_swiglu_rows(self, o, x, norm_weight, eps):
        return self.gemv_rows(x, None, norm_weight, eps)  # (raises: only QuantLinear overrides the pair)

    def pairs_with(self, o: "_Kernels") -> bool:
        """Whether ``self`` and ``o`` (fc_1, fc_2) can share one dual launch: here what every format asks."""
        return (type(o) is type(self) and self.bias is None and o.bias is None
                and (self.out_features, self.in_features) == (o.out_features, o.in_features))

    def gemm_swiglu(self, o: "_Kernels", x: torch.Tensor) -> Optional[torch.Tensor]:
        """The fused fc_1 || fc_2 + SwiGLU prefill GEMM, or None where the format or the shape has none."""
        return None


class QuantLinear(_Kernels, nn.Module):
    """Packed 4-bit weight ``qweight`` (N, K/2) uint8 + ``scales`` (N, K/group) on the GPU.

    ``forward`` dispatches like bitsandbytes' ``matmul_4bit``: one token -> fused dequant-GEMV
    (``lga_q4_gemv``), several -> MFMA GEMM with the dequantization fused (``lga_q4_gemm_fused``). ``weight`` is kept as an alias of the packed
    buffer so code that inspects ``linear.weight`` (e.g. ``.device``/``.dtype``) keeps working.
    """

    # lga_q4_gemv launch variant for one-token inputs (-1: the library's heuristic). The opt-in fused kernels
    # (attention + out-projection, out-projection + MoE gate) reproduce the 4-rows-per-wave form (variant 0); their
    # bit-identity A/B tests pin the unfused side to it
    gemv_variant = -1

    def __init__(self, in_features: int, out_features: int, fmt: int, group: int,
                 bias: Optional[torch.Tensor] = None, device=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.fmt, self.group = fmt, group
        self.register_buffer("qweight", torch.empty(out_features, in_features // 2, dtype=torch.uint8, device=device))
        sdt = torch.bfloat16 if fmt == ops.FMT_Q4G else torch.float32
        self.register_buffer("scales", torch.empty(out_features, in_features // group, dtype=sdt, device=device))
        self.bias = None if bias is None else nn.Parameter(bias.to(torch.bfloat16), requires_grad=False)

    @property
    def weight(self) -> torch.Tensor:
        return self.qweight

    @classmethod
    def from_float(cls, weight: torch.Tensor, bias: Optional[torch.Tensor], mode: str,
                   device: Optional[torch.device] = None) -> "QuantLinear":
        fmt, group = parse_mode(mode)
        N, K = weight.shape
        group = _fit_group(K, group)
        device = device or (weight.device if weight.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        w = weight.detach().to(device)
        m = cls(K, N, fmt, group, None if bias is None else bias.detach().to(device), device=device)
        qw, sc = ops.quantize(w, fmt, group)
        m.qweight.copy_(qw)
        m.scales.copy_(sc)
        if mode in _DOUBLE_QUANT:
            m.dq_offset = ops.nf4_double_quant(m.scales, bnb_dynamic_map(device))
        return m

    def pairs_with(self, o) -> bool:
        return super().pairs_with(o) and (self.fmt, self.group) == (o.fmt, o.group)

    def gemv_fuses_norm(self, dual: bool = False) -> bool:
        """lga_q4_gemv(_swiglu) fuses the RMSNorm prologue only when the row fits one K tile (64 lanes x 2 chunks
        x 32 for the dual SwiGLU GEMV, x 4 chunks otherwise)."""
        return self.in_features // 32 <= (128 if dual else 256)

    def gemv(self, x, res, norm_weight, eps):
        return ops.q4_gemv(x, self.qweight, self.scales, self.out_features, self.in_features, self.group, self.fmt,
                           bias=self.bias, residual=res, norm_weight=norm_weight, eps=eps, variant=self.gemv_variant)

    def gemv_rows(self, x, res, norm_weight, eps):
        return ops.q4_gemv_rows(x, self.qweight, self.scales, self.out_features, self.in_features, self.group,
                                self.fmt, bias=self.bias, residual=res, norm_weight=norm_weight, eps=eps)

    def gemv_swiglu_rows(self, o, x, norm_weight, eps):
        return ops.q4_gemv_swiglu_rows(x, self.qweight, self.scales, o.qweight, o.scales, self.out_features,
                                       self.in_features, self.group, self.fmt, norm_weight=norm_weight, eps=eps)

    def gemm(self, x, res):
        N, K = self.out_features, self.in_features
        # several rows (prefill): the dequantization runs inside the MFMA tiles (csrc/gemm_q4f.hip) to the bits
        # bnb's dequantize_4bit writes — the reference's M > 1 path without a bf16 weight in HBM; group 32 /
        # K % 64: gemm.hip's 128 x 128 tiles (same staged weight bits)
        gemm = ops.q4_gemm_fused if ops.q4f_fits(x.shape[0], N, K, self.group, self.fmt) else ops.q4_gemm
        return gemm(x, self.qweight, self.scales, N, K, self.group, self.fmt, bias=self.bias, residual=res)

    def gemv_swiglu(self, o, x, norm_weight, eps):
        return ops.q4_gemv_swiglu(x, self.qweight, self.scales, o.qweight, o.scales, self.out_features,
                                  self.in_features, self.group, self.fmt, norm_weight=norm_weight, eps=eps)

    def gemm_swiglu(self, o, x):
        N, K = self.out_features, self.in_features
        if ops.q4f_fits(x.shape[0], N, K, self.group, self.fmt):
            return ops.q4_gemm_swiglu(x, self.qweight, self.scales, o.qweight, o.scales, N, K, self.group, self.fmt)
        return None

    def extra_repr(self) -> str:
        kind = {ops.FMT_Q4G: "int4", ops.FMT_NF4: "nf4", ops.FMT_FP4: "fp4"}[self.fmt]
        return f"in_features={self.in_features}, out_features={self.out_features}, {kind}, group={self.group}"


class Int8Linear(_Kernels, nn.Module):
    """LLM.int8 Linear: ``qweight`` (N, K) int8 + ``scales`` (N,) fp32 row absmax on the GPU (bitsandbytes
    ``Linear8bitLt(has_fp16_weights=False, threshold=6.0)`` with bf16 in place of fp16).

    ``forward`` follows ``QuantLinear.forward``: one token -> ``lga_int8_gemv`` (RMSNorm / bias / residual fused,
    activation quantization and outlier columns inside the launch), several -> RMSNorm, ``lga_int8_quantize_act``
    and the i8 MFMA GEMM ``lga_int8_gemm``. Nothing synchronises with the host."""

    threshold = ops.INT8_THRESHOLD

    def __init__(self, in_features: int, out_features: int, bias: Optional[torch.Tensor] = None, device=None):
        super().__init__()
        if in_features % 16:
            raise ValueError(f"in_features={in_features} is not a multiple of 16; the int8 kernels read 16-B chunks")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("qweight", torch.empty(out_features, in_features, dtype=torch.int8, device=device))
        self.register_buffer("scales", torch.empty(out_features, dtype=torch.float32, device=device))
        self.bias = None if bias is None else nn.Parameter(bias.to(torch.bfloat16), requires_grad=False)

    @property
    def weight(self) -> torch.Tensor:
        return self.qweight

    @classmethod
    def from_float(cls, weight: torch.Tensor, bias: Optional[torch.Tensor],
                   device: Optional[torch.device] = None, *, mode: str = "bnb.int8") -> "Int8Linear":
        N, K = weight.shape
        device = device or (weight.device if weight.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        m = cls(K, N, None if bias is None else bias.detach().to(device), device=device)
        qw, sc = ops.int8_quantize(weight.detach().to(device))
        m.qweight.copy_(qw)
        m.scales.copy_(sc)
        return m

    def pairs_with(self, o) -> bool:
        return super().pairs_with(o) and self.threshold == o.threshold

    def gemv(self, x, res, norm_weight, eps):
        return ops.int8_gemv(x, self.qweight, self.scales, bias=self.bias, residual=res, norm_weight=norm_weight,
                             eps=eps, threshold=self.threshold)

    def gemm(self, x, res):
        xq, sx, cols, count, _ = ops.int8_quantize_act(x, threshold=self.threshold)
        return ops.int8_gemm(x, xq, sx, cols, count, self.qweight, self.scales, bias=self.bias, residual=res)

    def gemv_swiglu(self, o, x, norm_weight, eps):  # one activation quantization for both
        return ops.int8_gemv_swiglu(x, self.qweight, self.scales, o.qweight, o.scales, norm_weight=norm_weight,
                                    eps=eps, threshold=self.threshold)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, int8, "
                f"threshold={self.threshold}")


class _DenseLinear(_Kernels):
    """The per-call adapter of a device ``nn.Linear`` (bf16 or fp32 weights) to the ``_Kernels`` skeleton."""

    kind = "Linear"

    def __init__(self, lin: nn.Linear) -> None:
        if lin.weight.dtype != self.act_dtype:
            raise TypeError("unquantized Linear on the MI355X path expects bf16 weights (bf16-true), got "
                            f"{lin.weight.dtype}")
        # build_model leaves the weight contiguous and the bias in the compute dtype; a strided view (a TP row shard
        # from generate/tp.py's tensor_split(dim=1)) or a bias of another dtype is converted once, in place: the
        # module (and its state_dict) then holds the converted tensor, so no later call or graph replay casts again
        if not lin.weight.is_contiguous():
            lin.weight.data = lin.weight.data.contiguous()
        if lin.bias is not None and lin.bias.dtype != self.act_dtype:
            lin.bias.data = lin.bias.data.to(self.act_dtype)
        self.lin, self.weight, self.bias = lin, lin.weight, lin.bias
        self.out_features, self.in_features = lin.weight.shape

    __call__ = _Kernels.forward


class F32Linear(_DenseLinear):
    """F.linear in float32 (the reference's --precision 32-true, BASELINE config 1): lga_f32_linear for any number
    of rows, no RMSNorm and no dual launch."""

    kind, act_dtype, expects = "fp32 Linear", torch.float32, "fp32 activations (32-true)"

    def gemv_fuses_norm(self, dual: bool = False) -> bool:
        raise NotImplementedError("fp32 path: RMSNorm-family blocks are not built in fp32 (GPT-NeoX LayerNorm is)")

    def pairs_with(self, o) -> bool:
        return False

    def gemm(self, x, res):
        return ops.f32_linear(x, self.weight, bias=self.bias, residual=res)

    def gemv(self, x, res, norm_weight, eps):  # no M split (gemv_fuses_norm has refused a norm)
        return self.gemm(x, res)


class Bf16Linear(_DenseLinear):
    """F.linear with bf16 weights (BASELINE config 2): one token -> lga_bf16_gemv (RMSNorm / residual fused),
    several -> the fused MFMA GEMM with the weight DMA'd as stored (csrc/gemm_q4f.hip, fmt 2) where the shape
    fits, else lga_bf16_gemm."""

    def pairs_with(self, o) -> bool:
        return super().pairs_with(o) and type(self.lin) is nn.Linear and type(o.lin) is nn.Linear

    def gemv(self, x, res, norm_weight, eps):
        return ops.bf16_gemv(x, self.weight, bias=self.bias, residual=res, norm_weight=norm_weight, eps=eps)

    def gemm(self, x, res):
        N, K = self.weight.shape
        if ops.q4f_fits(x.shape[0], N, K, 64, ops.FMT_BF16):
            return ops.q4_gemm_fused(x, self.weight, None, N, K, 64, ops.FMT_BF16, bias=self.bias, residual=res)
        return ops.bf16_gemm(x, self.weight, bias=self.bias, residual=res)

    def gemv_swiglu(self, o, x, norm_weight, eps):
        return ops.bf16_gemv_swiglu(x, self.weight, o.weight, norm_weight=norm_weight, eps=eps)

    def gemm_swiglu(self, o, x):
        N, K = self.weight.shape
        if ops.q4f_fits(x.shape[0], N, K, 64, ops.FMT_BF16):
            return ops.q4_gemm_swiglu(x, self.weight, None, o.weight, None, N, K, 64, ops.FMT_BF16)
        return None


def kernels(lin: nn.Module) -> _Kernels:
    """The format of a Linear: call it like the module, with the ``_Kernels.forward`` fusion hooks."""
    if isinstance(lin, _Kernels):
        return lin
    if isinstance(lin, nn.Linear) and lin.weight.is_cuda:
        return (F32Linear if lin.weight.dtype == torch.float32 else Bf16Linear)(lin)
    raise NotImplementedError(
        "Linear without MI355X weights: move the model to the GPU in bf16, or convert it with "
        "lit_gpt.quantize.QuantizedPrecision('int4-g128' | 'nf4' | 'bnb.int8').convert_module(model) (the --quantize "
        "flag)")


def swiglu(fc_1: nn.Module, fc_2: nn.Module, x: torch.Tensor, norm: Optional[nn.Module] = None, *,
           rows: bool = False) -> torch.Tensor:
    """bf16(silu(fc_1 n)) * fc_2 n for n = norm(x) (an RMSNorm; x itself without one), x (M, K) contiguous: one
    dual GEMV launch for one row and one fused GEMM launch for several where the pair is eligible and the format
    has the kernel, else the two Linears and ``lga_swiglu``. The norm runs once for the pair. ``rows`` (batched
    decode, M <= 8 rows): the dual rows GEMV, row r with the bits of the one-row launch on x[r]."""
    f1, f2 = kernels(fc_1), kernels(fc_2)
    norm_weight, norm_eps = (None, 1e-5) if norm is None else (norm.weight, norm.eps)
    M, pair = x.shape[0], f1.pairs_with(f2)
    if rows:
        if pair:
            if norm_weight is not None and not f1.gemv_fuses_norm(dual=True):
                x, norm_weight = ops.rmsnorm(x, norm_weight, norm_eps), None
            return f1.gemv_swiglu_rows(f2, x, norm_weight, norm_eps)
        # as the one-row path of an unpaired fc_1 / fc_2 (biases): the norm once, two Linears, lga_swiglu
        n = x if norm_weight is None else ops.rmsnorm(x, norm_weight, norm_eps)
        return ops.swiglu(f1(n, rows=True).contiguous(), f2(n, rows=True).contiguous())
    if M == 1 and pair:
        if norm_weight is not None and not f1.gemv_fuses_norm(dual=True):
            x, norm_weight = ops.rmsnorm(x, norm_weight, norm_eps), None
        return f1.gemv_swiglu(f2, x, norm_weight, norm_eps).view(1, -1)
    n = x if norm_weight is None else ops.rmsnorm(x, norm_weight, norm_eps)
    g = f1.gemm_swiglu(f2, n) if M > 1 and pair else None
    return g if g is not None else ops.swiglu(f1(n).contiguous(), f2(n).contiguous())


def head_argmax_supported(lin: nn.Module) -> bool:
    """Whether lga_q4_gemv_argmax_embed covers this lm_head: a 4-bit QuantLinear with K <= 4096, no bias."""
    return (isinstance(lin, QuantLinear) and lin.bias is None and lin.in_features <= 4096
            and lin.in_features % 32 == 0 and lin.qweight.is_cuda)


def gemv_allreduce_supported(lin: nn.Module, x: torch.Tensor) -> bool:
    """Whether lga_q4_gemv_allreduce covers ``lin(x)``: a 4-bit QuantLinear and one bf16 device row."""
    return (isinstance(lin, QuantLinear) and x.numel() == lin.in_features and x.dtype == torch.bfloat16
            and x.is_cuda)


class QuantizedPrecision:
    """Stand-in for Lightning's ``BitsandbytesPrecision(mode, dtype)`` (generate/base.py:128-134)."""

    def __init__(self, mode: str, dtype: torch.dtype = torch.bfloat16) -> None:
        parse_mode(mode)
        if dtype != torch.bfloat16:
            raise NotImplementedError("the MI355X quantized path computes in bf16 (precision bf16-true)")
        self.mode, self.dtype = mode, dtype

    def convert_module(self, module: nn.Module, device: Optional[torch.device] = None) -> nn.Module:
        """Replace every ``nn.Linear`` (lm_head included) by a ``QuantLinear`` (``Int8Linear`` for ``bnb.int8``)
        quantized on ``device``."""
        for name, child in list(module.named_children()):
            if isinstance(child, nn.Linear):
                cls = Int8Linear if self.mode == "bnb.int8" else QuantLinear
                setattr(module, name, cls.from_float(child.weight, child.bias, mode=self.mode, device=device))
            else:
                self.convert_module(child, device)
        return module
