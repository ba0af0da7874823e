"""--quantize mxfp4-a8 without a GPU: the mode table, the refusals of build_model before any weight is materialised, and
the argument checks of the two C entry points before any launch."""

import ctypes
import types

import pytest
import torch


def test_mode_is_registered():
    from lit_gpt import ops, quantize

    assert quantize.parse_mode("mxfp4-a8") == (ops.FMT_MXFP4, 32)
    assert "lga_mx8_quantize" in ops.SIGNATURES and "lga_mxfp4_a8_gemm" in ops.SIGNATURES
    assert issubclass(quantize.Mxfp4A8Linear, quantize.Mxfp4Linear)


@pytest.mark.parametrize("name,fabric,match", [
    ("Mixtral-8x7B-v0.1", None, "sparse-MoE"),
    ("Llama-2-7b-hf", types.SimpleNamespace(world_size=2, global_rank=0), "tensor parallelism"),
])
def test_build_model_refuses_moe_and_tp_before_any_device_use(name, fabric, match):
    from generate.base import build_model
    from lit_gpt import Config

    cfg = Config.from_name(name, n_layer=1, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512,
                           vocab_size=1000, padding_multiple=64, block_size=64)
    with pytest.raises(NotImplementedError, match=f"mxfp4-a8 with .*{match}"):
        build_model(cfg, quantize="mxfp4-a8", device=torch.device("cuda", 0), fabric=fabric)


@pytest.mark.parametrize("null,M,K,msg", [(True, 2, 64, b"null pointer"), (False, 2, 48, b"multiple of 32"),
                                          (False, 0, 64, b"M >= 1")])
def test_c_entry_points_refuse_before_any_launch(null, M, K, msg):
    from lit_gpt import ops

    lib, p = ops.load_library(), ctypes.c_void_p(4096)
    q = None if null else p
    assert lib.lga_mx8_quantize(p, q, p, M, K, None) != 0
    assert msg in lib.lga_last_error_string()
    assert lib.lga_mxfp4_a8_gemm(p, p, q, p, None, None, p, M, 8, K, None) != 0
    assert msg in lib.lga_last_error_string()
