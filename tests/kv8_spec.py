"""The fp8 (OCP e4m3) KV-cache format restated in torch — the specification the kernels are tested
against, bit for bit.

A row is the 128 bf16 values of one (slot, query group, position) of K (after RoPE) or V. amax = max |x_i| = m 2^E with
m in [0.5, 1) (frexp); e = E - 9 if m <= 0.875 else E - 8, clamped to [-126, 127]; s = 2^e (the smallest power of two
with amax / s <= 448); amax = 0 gives s = 1. code_i = e4m3fn(x_i / s), round to nearest even; the value read back is
float(code_i) * s. Rows with non-finite values or amax < 2^-100 are outside the contract.
"""

import torch

from oracle import model as om

E4M3_MAX = 448.0


def kv8_scale(amax: torch.Tensor) -> torch.Tensor:
    """fp32 row maxima -> fp32 scales (powers of two)."""
    amax = amax.float()
    m, E = torch.frexp(amax)
    e = torch.where(m <= 0.875, E - 9, E - 8).clamp(-126, 127)
    s = torch.ldexp(torch.ones_like(amax), e)
    return torch.where(amax == 0, torch.ones_like(amax), s)


def kv8_round(x: torch.Tensor):
    """Rows (..., n) of any float dtype -> (codes uint8 (..., n), scale fp32 (...), dequantized fp32 (..., n)). The
    rows are first rounded to bf16: the format quantizes what the bf16 cache would hold."""
    xb = x.to(torch.bfloat16).float()
    s = kv8_scale(xb.abs().amax(dim=-1))
    q = (xb / s.unsqueeze(-1)).to(torch.float8_e4m3fn)  # exact division, RNE conversion; |x / s| <= 448: no saturation
    return q.view(torch.uint8), s, q.float() * s.unsqueeze(-1)


def kv8_dequantize(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return codes.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1)


class Kv8Cache(om.Cache):
    """``OracleGPT.cache`` holding what an fp8 cache gives back: assign ``Kv8Cache(k=og.cache.k, v=og.cache.v)`` after
    ``og.set_kv_cache`` and every attention of the oracle reads quantized-then-dequantized K / V, its own rows
    included — the whole-model specification of ``--kv_cache fp8``."""

    def write(self, i: int, pos, k: torch.Tensor, v: torch.Tensor) -> None:
        self.k[i][:, pos] = kv8_round(k)[2].to(self.k[i].dtype)
        self.v[i][:, pos] = kv8_round(v)[2].to(self.v[i].dtype)
