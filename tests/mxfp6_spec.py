"""The MXFP6 (e2m3) weight format restated in torch (OCP MX v1.0 §5.3.2, §6.3) — the specification the
kernels are tested against, bit for bit.

A block is 32 consecutive weights of a row (fp32; bf16 input converts exactly). amax = max |w_i| = m 2^E with m in
[0.5, 1) (frexp), so floor(log2 amax) = E - 1; s = E - 3 clamped to [-123, 125], scale byte e = s + 127 in [4, 252]
(e8m0: 2^(e - 127)); amax = 0 gives e = 127 and all codes 0. code_i: the e2m3 magnitude nearest to |w_i| 2^-s, of two
equally near the one with the even code (magnitudes above 7.5 end at 7.5), with the sign bit of w_i in bit 5 — also where
the magnitude rounds to zero. A block's codes fill 24 bytes, code i in bits 6 i .. 6 i + 5 of the block's 192-bit
little-endian word. Blocks with non-finite values are outside the contract.
"""

import torch

# magnitude of code & 31: M / 8 for E = 0, 2^(E - 1) (1 + M / 8) for E = 1..3
E2M3 = torch.tensor([m / 8 for m in range(8)] + [2.0 ** (e - 1) * (1 + m / 8) for e in (1, 2, 3) for m in range(8)],
                    dtype=torch.float64)


def mx6_round(blocks: torch.Tensor):
    """Blocks (..., 32) of any float dtype -> (codes uint8 (..., 32), six bits each; scale bytes uint8 (...);
    dequantized fp32 (..., 32))."""
    w = blocks.float()
    amax = w.abs().amax(dim=-1)
    s = (torch.frexp(amax)[1] - 3).clamp(-123, 125)
    s = torch.where(amax == 0, torch.zeros_like(s), s)
    v = torch.ldexp(w.double().abs(), -s.unsqueeze(-1))  # exact in float64
    d = (v.unsqueeze(-1) - E2M3).abs()
    odd = (torch.arange(32) % 2).expand_as(d)
    mag = torch.where(d == d.amin(dim=-1, keepdim=True), odd, 2).argmin(dim=-1)  # nearest; of two, the even code
    sign = torch.signbit(w) & (amax != 0).unsqueeze(-1)
    deq = torch.ldexp(torch.where(sign, -E2M3[mag], E2M3[mag]), s.unsqueeze(-1)).float()
    return (mag + 32 * sign).to(torch.uint8), (s + 127).to(torch.uint8), deq


def mx6_pack(codes: torch.Tensor) -> torch.Tensor:
    """Six-bit codes (..., K) -> bytes (..., 3 K / 4): four codes are 24 bits, three little-endian bytes."""
    c = codes.to(torch.int32).unflatten(-1, (-1, 4))
    v = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return torch.stack([v & 255, (v >> 8) & 255, v >> 16], dim=-1).flatten(-2).to(torch.uint8)
