"""--quantize mxfp4 without a GPU: the mode table, the refusals of build_model before any weight is materialised, the
K % 32 check at conversion, and tests/mxfp4_spec.py on a block computed by hand."""

import types

import pytest
import torch

from mxfp4_spec import mx_pack, mx_round


def test_mode_is_registered():
    from lit_gpt import ops, quantize

    assert quantize.parse_mode("mxfp4") == (ops.FMT_MXFP4, 32) and ops.MXFP4_GROUP == 32
    for name in ("lga_mxfp4_quantize", "lga_mxfp4_gemv", "lga_mxfp4_gemv_swiglu", "lga_mxfp4_gemm"):
        assert name in ops.SIGNATURES


@pytest.mark.parametrize("name,fabric,match", [
    ("Mixtral-8x7B-v0.1", None, "sparse-MoE"),
    ("Llama-2-7b-hf", types.SimpleNamespace(world_size=2, global_rank=0), "tensor parallelism"),
])
def test_build_model_refuses_moe_and_tp_before_any_device_use(name, fabric, match):
    from generate.base import build_model
    from lit_gpt import Config

    cfg = Config.from_name(name, n_layer=1, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512,
                           vocab_size=1000, padding_multiple=64, block_size=64)
    with pytest.raises(NotImplementedError, match=f"mxfp4 with .*{match}"):  # (a device that does not exist)
        build_model(cfg, quantize="mxfp4", device=torch.device("cuda", 0), fabric=fabric)


def test_in_features_must_divide_by_32():
    from lit_gpt.quantize import Mxfp4Linear

    with pytest.raises(ValueError, match="multiple of 32"):
        Mxfp4Linear.from_float(torch.zeros(8, 48), None, mode="mxfp4")
    with pytest.raises(ValueError, match="multiple of 32"):
        Mxfp4Linear(48, 8, device="meta")


# amax = 7.5 = 1.875 * 2^2: s = 0, scale byte 127. By hand, value -> code: 7.5 in (6, 8) saturates to 6 (7); the ties
# 0.25 -> 0 (0), 0.75 -> 1 (2), 1.25 -> 1 (2), 1.75 -> 2 (4), 2.5 -> 2 (4), 3.5 -> 4 (6), 5 -> 4 (6) all go to the even
# code; -0.1 rounds to zero and keeps its sign (8); -3.2 -> -3 (13); 0.26 -> 0.5 (1); 5.01 -> 6 (7); the rest are zeros.
HAND = [7.5, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.1, -3.2, 0.26, 5.01] + [0.0] * 20
HAND_CODES = [7, 0, 2, 2, 4, 4, 6, 6, 8, 13, 1, 7] + [0] * 20
HAND_VALUES = [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -0.0, -3.0, 0.5, 6.0] + [0.0] * 20


def test_spec_on_a_hand_computed_block():
    blk = torch.tensor(HAND)
    codes, e, deq = mx_round(torch.stack([blk, blk * 2.0 ** -9, torch.zeros(32), -torch.zeros(32)]))
    assert e.tolist() == [127, 118, 127, 127]
    assert codes[0].tolist() == HAND_CODES and codes[1].tolist() == HAND_CODES
    assert codes[2:].count_nonzero() == 0  # amax = 0: all codes 0, whatever the signs
    assert torch.equal(deq[0], torch.tensor(HAND_VALUES)) and torch.equal(deq[1], deq[0] * 2.0 ** -9)
    assert torch.signbit(deq[0, 8]) and mx_pack(codes[0])[:6].tolist() == [0x07, 0x22, 0x44, 0x66, 0xD8, 0x71]


def test_dequantized_values_are_exact_in_bf16():
    g = torch.randn(64, 32, generator=torch.Generator().manual_seed(0)).clamp(-1.9, 1.9)
    g = g * torch.exp2(torch.linspace(-130, 127, 64)).unsqueeze(1)  # every clamp of the scale, fp32 subnormals too
    _, e, deq = mx_round(g)
    assert int(e.min()) == 2 and int(e.max()) == 252
    assert torch.equal(deq.bfloat16().float(), deq) and bool(((deq == 0) | (deq.abs() >= 2.0 ** -126)).all())
