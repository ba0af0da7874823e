"""--quantize fp8-g128 without a GPU: the mode table, the refusals of build_model before any weight is materialised,
and the K % 128 check at conversion."""

import types

import pytest
import torch


def test_mode_is_registered():
    from lit_gpt import ops, quantize

    assert quantize.parse_mode("fp8-g128") == (ops.FMT_FP8, 128)
    for name in ("lga_fp8_quantize", "lga_fp8_gemv", "lga_fp8_gemv_swiglu", "lga_fp8_gemm"):
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
    with pytest.raises(NotImplementedError, match=match):  # (a device that does not exist: nothing may touch it)
        build_model(cfg, quantize="fp8-g128", device=torch.device("cuda", 0), fabric=fabric)


def test_in_features_must_divide_by_128():
    from lit_gpt.quantize import Fp8Linear

    with pytest.raises(ValueError, match="multiple of 128"):
        Fp8Linear.from_float(torch.zeros(8, 192), None, mode="fp8-g128")
    with pytest.raises(ValueError, match="multiple of 128"):
        Fp8Linear(64, 8, device="meta")
