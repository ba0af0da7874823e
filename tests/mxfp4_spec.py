"""The MXFP4 weight format restated in torch (OCP MX v1.0 §6.3) — the specification the kernels are
tested against, bit for bit.

A block is 32 consecutive weights of a row (fp32; bf16 input converts exactly). amax = max |w_i| = m 2^E with m in
[0.5, 1) (frexp), so floor(log2 amax) = E - 1; s = E - 3 clamped to [-125, 125], scale byte e = s + 127 (e8m0: 2^(e -
127)); amax = 0 gives e = 127 and all codes 0. code_i: the e2m1 magnitude nearest to |w_i| 2^-s, of two equally near the
one with the even code (magnitudes above 6 end at 6), with the sign bit of w_i in bit 3 — also where the magnitude
rounds to zero. Two codes share a byte, the even column in the low nibble. Blocks with non-finite values are outside the
contract.
"""

import torch

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)  # magnitude of code & 7


def mx_round(blocks: torch.Tensor):
    """Blocks (..., 32) of any float dtype -> (codes uint8 (..., 32), one nibble each; scale bytes uint8 (...);
    dequantized fp32 (..., 32))."""
    w = blocks.float()
    amax = w.abs().amax(dim=-1)
    s = (torch.frexp(amax)[1] - 3).clamp(-125, 125)
    s = torch.where(amax == 0, torch.zeros_like(s), s)
    v = torch.ldexp(w.double().abs(), -s.unsqueeze(-1))  # exact in float64
    d = (v.unsqueeze(-1) - E2M1).abs()
    odd = (torch.arange(8) % 2).expand_as(d)
    mag = torch.where(d == d.amin(dim=-1, keepdim=True), odd, 2).argmin(dim=-1)  # nearest; of two, the even code
    code = mag + 8 * torch.signbit(w)
    code = torch.where((amax == 0).unsqueeze(-1), torch.zeros_like(code), code)
    return code.to(torch.uint8), (s + 127).to(torch.uint8), mx_dequantize(code, s + 127)


def mx_dequantize(codes: torch.Tensor, scale_bytes: torch.Tensor) -> torch.Tensor:
    """Nibble codes (..., 32), scale bytes (...) -> fp32 (..., 32)."""
    mag = E2M1[(codes & 7).long()] * torch.where((codes & 8) != 0, -1.0, 1.0)
    return torch.ldexp(mag, (scale_bytes.long() - 127).unsqueeze(-1)).float()


def mx_pack(codes: torch.Tensor) -> torch.Tensor:
    """Nibble codes (..., K) -> bytes (..., K / 2), the even column in the low nibble."""
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).to(torch.uint8)
