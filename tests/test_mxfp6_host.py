"""--quantize mxfp6 without a GPU: the mode table, the refusals of build_model before any weight is materialised, the
K % 64 check at conversion and in the C entry points, and tests/mxfp6_spec.py on a block computed by hand."""

import ctypes
import types

import pytest
import torch

from mxfp6_spec import mx6_pack, mx6_round


def test_mode_is_registered():
    from lit_gpt import ops, quantize

    assert quantize.parse_mode("mxfp6") == (ops.FMT_MXFP6, 32) and ops.MXFP6_GROUP == 32
    for name in ("lga_mxfp6_quantize", "lga_mxfp6_gemv", "lga_mxfp6_gemv_swiglu", "lga_mxfp6_gemm"):
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
    with pytest.raises(NotImplementedError, match=f"mxfp6 with .*{match}"):  # (a device that does not exist)
        build_model(cfg, quantize="mxfp6", device=torch.device("cuda", 0), fabric=fabric)


def test_in_features_must_divide_by_64():
    from lit_gpt.quantize import Mxfp6Linear

    with pytest.raises(ValueError, match="multiple of 64"):
        Mxfp6Linear.from_float(torch.zeros(8, 96), None, mode="mxfp6")
    with pytest.raises(ValueError, match="multiple of 64"):
        Mxfp6Linear(96, 8, device="meta")
    m = Mxfp6Linear(128, 8, device="meta")
    assert m.qweight.shape == (8, 96) and m.scales.shape == (8, 4) and set(m.state_dict()) == {"qweight", "scales"}


@pytest.mark.parametrize("null,K,msg", [(True, 64, b"null pointer"), (False, 96, b"multiple of 64")])
def test_c_entry_points_refuse_before_any_launch(null, K, msg):
    from lit_gpt import ops

    lib, p = ops.load_library(), ctypes.c_void_p(4096)
    y = None if null else p
    for rc in (lib.lga_mxfp6_quantize(p, 1, y, p, 8, K, None),
               lib.lga_mxfp6_gemv(p, p, p, None, None, None, 1e-5, y, 8, K, None),
               lib.lga_mxfp6_gemv_swiglu(p, p, p, p, p, None, 1e-5, y, 8, K, None),
               lib.lga_mxfp6_gemm(p, p, p, None, None, y, 2, 8, K, None)):
        assert rc != 0 and msg in lib.lga_last_error_string()


# amax = 7.6 = 1.9 * 2^2: s = 0, scale byte 127. By hand, value -> code: 7.6 and 7.5 end at 7.5 (31); the ties 0.0625 ->
# 0 (0), 0.1875 -> 0.25 (2), 1.0625 -> 1 (8), 2.125 -> 2 (16), 4.25 -> 4 (24), 7.25 -> 7 (30) all go to the even code;
# -0.01 rounds to zero and keeps its sign (32); -3.3 -> -3.25 (32 + 21); 0.07 -> 0.125 (1); the rest are zeros.
HAND = [7.6, 7.5, 0.0625, 0.1875, 1.0625, 2.125, 4.25, 7.25, -0.01, -3.3, 0.07] + [0.0] * 21
HAND_CODES = [31, 31, 0, 2, 8, 16, 24, 30, 32, 53, 1] + [0] * 21
HAND_VALUES = [7.5, 7.5, 0.0, 0.25, 1.0, 2.0, 4.0, 7.0, -0.0, -3.25, 0.125] + [0.0] * 21


def test_spec_on_a_hand_computed_block():
    blk = torch.tensor(HAND)
    codes, e, deq = mx6_round(torch.stack([blk, blk * 2.0 ** -9, torch.zeros(32), -torch.zeros(32)]))
    assert e.tolist() == [127, 118, 127, 127]
    assert codes[0].tolist() == HAND_CODES and codes[1].tolist() == HAND_CODES
    assert codes[2:].count_nonzero() == 0  # amax = 0: all codes 0, whatever the signs
    assert torch.equal(deq[0], torch.tensor(HAND_VALUES)) and torch.equal(deq[1], deq[0] * 2.0 ** -9)
    # 31 | 31 << 6 | 0 << 12 | 2 << 18 = 0x0807DF, 8 | 16 << 6 | 24 << 12 | 30 << 18 = 0x798408, little-endian
    assert torch.signbit(deq[0, 8]) and mx6_pack(codes[0])[:6].tolist() == [0xDF, 0x07, 0x08, 0x08, 0x84, 0x79]
    assert mx6_pack(codes).shape == (4, 24)


def test_dequantized_values_are_exact_normal_bf16_and_the_scale_reaches_both_ends():
    g = torch.randn(64, 32, generator=torch.Generator().manual_seed(0)).clamp(-1.9, 1.9)
    g = g * torch.exp2(torch.linspace(-130, 127, 64)).unsqueeze(1)  # every clamp of the scale, fp32 subnormals too
    _, e, deq = mx6_round(g)
    assert int(e.min()) == 4 and int(e.max()) == 252
    assert torch.equal(deq.bfloat16().float(), deq) and bool(((deq == 0) | (deq.abs() >= 2.0 ** -126)).all())
