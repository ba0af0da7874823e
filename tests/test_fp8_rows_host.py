"""The fp8-g128 multi-row decode GEMVs without a GPU: the registered symbols, the mode list of the batched route, and the
argument checks of the C entry points (before any launch)."""

import ctypes
import types

import pytest


def test_symbols_and_rows_modes():
    from lit_gpt import ops, quantize

    assert "lga_fp8_gemv_rows" in ops.SIGNATURES and "lga_fp8_gemv_swiglu_rows" in ops.SIGNATURES
    assert quantize.ROWS_MODES.endswith(", fp8-g128")
    assert "int4-g128/64/32, nf4, bnb.nf4, bnb.nf4-dq, bnb.fp4, bnb.fp4-dq" in quantize.ROWS_MODES
    with pytest.raises(NotImplementedError, match="fp8-g128"):  # still no rows kernel for bnb.int8
        quantize.Int8Linear.gemv_rows(types.SimpleNamespace(kind="Int8Linear"), None, None, None, 1e-5)


@pytest.mark.parametrize("M,K,norm,msg", [(0, 256, False, b"1..8"), (9, 256, False, b"1..8"),
                                          (2, 192, False, b"multiple of 128"), (2, 12416, True, b"K <= 12288")])
def test_c_entry_points_refuse_before_any_launch(M, K, norm, msg):
    from lit_gpt import ops

    lib, p = ops.load_library(), ctypes.c_void_p(16)
    nw = p if norm else None
    assert lib.lga_fp8_gemv_rows(p, p, p, None, None, nw, 1e-5, p, M, 4, K, None) != 0
    assert msg in lib.lga_last_error_string()
    assert lib.lga_fp8_gemv_swiglu_rows(p, p, p, p, p, nw, 1e-5, p, M, 4, K, None) != 0
    assert msg in lib.lga_last_error_string()

