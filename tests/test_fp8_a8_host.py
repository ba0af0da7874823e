"""--quantize fp8-g128-a8 without a GPU: the mode table, the refusals of build_model before any weight is materialised,
and the argument checks of the C entry point before any launch."""

import ctypes
import types

import pytest
import torch


def test_mode_is_registered():
    from lit_gpt import ops, quantize

    assert quantize.parse_mode("fp8-g128-a8") == (ops.FMT_FP8, 128)
    assert "lga_fp8_a8_gemm" in ops.SIGNATURES
    assert issubclass(quantize.Fp8A8Linear, quantize.Fp8Linear)


@pytest.mark.parametrize("name,fabric,match", [
    ("Mixtral-8x7B-v0.1", None, "sparse-MoE"),
    ("Llama-2-7b-hf", types.SimpleNamespace(world_size=2, global_rank=0), "tensor parallelism"),
])
def test_build_model_refuses_moe_and_tp_before_any_device_use(name, fabric, match):
    from generate.base import build_model
    from lit_gpt import Config

    cfg = Config.from_name(name, n_layer=1, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512,
                           vocab_size=1000, padding_multiple=64, block_size=64)
    with pytest.raises(NotImplementedError, match=f"fp8-g128-a8 with .*{match}"):
        build_model(cfg, quantize="fp8-g128-a8", device=torch.device("cuda", 0), fabric=fabric)


@pytest.mark.parametrize("null,K,msg", [(True, 128, b"null pointer"), (False, 64, b"multiple of 128")])
def test_c_entry_point_refuses_before_any_launch(null, K, msg):
    from lit_gpt import ops

    lib, p = ops.load_library(), ctypes.c_void_p(4096)
    assert lib.lga_fp8_a8_gemm(p, p, None if null else p, p, None, None, p, 2, 8, K, None) != 0
    assert msg in lib.lga_last_error_string()
