"""bnb.int8 without a GPU: properties of the numpy specification (tests/int8_spec.py), mode parsing, and the
argument validation of the int8 C entry points (they return before any launch)."""

import ctypes

import numpy as np
import pytest

import int8_spec as spec


def _w(N=48, K=256, seed=3):
    return spec.bf16_round(np.random.default_rng(seed).standard_normal((N, K), dtype=np.float32) * np.float32(0.02))


def _x(M=4, K=256, seed=4):
    x = spec.bf16_round(np.random.default_rng(seed).standard_normal((M, K), dtype=np.float32))
    assert np.abs(x).max() < spec.TAU
    return x


def test_spec_weight_roundtrip_error_bound():
    w = _w()
    w[5] = 0.0
    q, s = spec.quantize_weight(w)
    assert q.dtype == np.int8 and np.abs(q.astype(int)).max() <= 127 and s[5] == 0 and not q[5].any()
    # |q s_w / 127 - w| <= s_w / 254 (half a step), multiplied through by 254 so that every term is exact in float64
    # (bf16 inputs: exact ties are common and must not fail on the test's own rounding)
    s64, w64 = s.astype(np.float64)[:, None], w.astype(np.float64)
    assert np.all(np.abs(2.0 * q.astype(np.float64) * s64 - 254.0 * w64) <= s64)


def test_spec_reproduces_the_int8_grid():
    rng = np.random.default_rng(5)
    q0 = rng.integers(-127, 128, (32, 64)).astype(np.int8)
    q0[:, 0] = 127  # every row's absmax is 127 -> W = q exactly
    q, s = spec.quantize_weight(q0.astype(np.float32))
    np.testing.assert_array_equal(q, q0)
    np.testing.assert_array_equal(s, np.full(32, 127, np.float32))
    np.testing.assert_array_equal(spec.dequantize_weight(q, s), q0.astype(np.float64))


def test_spec_threshold_zero_equals_no_outliers():
    q, s = spec.quantize_weight(_w())
    x = _x()
    assert not spec.quantize_act(x)[2].any()
    np.testing.assert_array_equal(spec.bf16_bits(spec.linear(x, q, s)), spec.bf16_bits(spec.linear(x, q, s, tau=0.0)))
    np.testing.assert_array_equal(spec.linear_exact(x, q, s), spec.linear_exact(x, q, s, tau=0.0))


def test_spec_all_outlier_row_has_no_main_term():
    q, s = spec.quantize_weight(_w())
    x = spec.bf16_round(np.full((1, 256), 7.0, np.float32) * np.where(np.arange(256) % 2, -1, 1))
    a, s_x, O = spec.quantize_act(x)
    assert O.all() and s_x[0] == 0 and not a.any()
    assert not spec.int_product(a, q).any()
    # ... so y is the outlier term alone: the dequantized weights against x
    ref = x.astype(np.float64) @ spec.dequantize_weight(q, s).T
    np.testing.assert_allclose(spec.linear_exact(x, q, s), ref, rtol=1e-12, atol=1e-12)
    assert np.all(np.abs(spec.linear(x, q, s) - ref) <= np.abs(ref) * 2 ** -8 + 1e-4)


def test_spec_outlier_columns_are_per_call():
    x = _x()
    x[2, 9] = 6.0  # exactly tau: an outlier column for every row of the call
    x[1, 11] = 5.96875  # just below: not one
    a, s_x, O = spec.quantize_act(x)
    assert np.nonzero(O)[0].tolist() == [9] and not a[:, 9].any() and a[1, 11] == 127


def test_parse_mode_accepts_int8_and_rejects_unknown():
    from lit_gpt import ops
    from lit_gpt.quantize import QuantizedPrecision, parse_mode

    assert parse_mode("bnb.int8")[0] == ops.FMT_INT8 == 4
    assert QuantizedPrecision("bnb.int8").mode == "bnb.int8"
    with pytest.raises(NotImplementedError, match="not supported"):
        parse_mode("bnb.int3")
    with pytest.raises(NotImplementedError):
        parse_mode("gptq.int4")


@pytest.fixture(scope="module")
def lib():
    from lit_gpt import ops

    return ops.load_library()


P = ctypes.c_void_p(4096)  # a non-null, 16-B aligned address that is never dereferenced: validation fails first


def test_int8_gemv_validates_before_launch(lib):
    rc = lib.lga_int8_gemv(None, None, None, None, None, None, 1e-5, 6.0, None, 8, 16, None)
    assert rc != 0 and b"null" in lib.lga_last_error_string()
    rc = lib.lga_int8_gemv(P, P, P, None, None, None, 1e-5, 6.0, P, 8, 24, None)
    assert rc != 0 and b"multiple of 16" in lib.lga_last_error_string()
    rc = lib.lga_int8_gemv_swiglu(P, P, P, None, P, None, 1e-5, 6.0, P, 8, 16, None)
    assert rc != 0 and b"null" in lib.lga_last_error_string()
    rc = lib.lga_int8_gemv_swiglu(P, P, P, P, P, None, 1e-5, 6.0, P, 8, 40, None)
    assert rc != 0 and b"multiple of 16" in lib.lga_last_error_string()
    rc = lib.lga_int8_gemv(P, P, P, None, None, None, 1e-5, 6.0, P, 8, 32768, None)
    assert rc != 0 and b"16384" in lib.lga_last_error_string()


def test_int8_gemm_validates_before_launch(lib):
    rc = lib.lga_int8_gemm(P, None, P, P, P, P, P, None, None, P, 4, 8, 32, None)
    assert rc != 0 and b"null" in lib.lga_last_error_string()
    rc = lib.lga_int8_gemm(P, P, P, P, P, P, P, None, None, P, 4, 8, 24, None)
    assert rc != 0 and b"multiple of 16" in lib.lga_last_error_string()
    rc = lib.lga_int8_gemm(P, P, P, P, P, P, P, None, None, P, 1, 8, 32, None)
    assert rc != 0 and b"M >= 2" in lib.lga_last_error_string()
    rc = lib.lga_int8_quantize_act(P, P, P, P, P, None, 4, 32, 6.0, None)
    assert rc != 0 and b"null" in lib.lga_last_error_string()
    rc = lib.lga_int8_quantize(P, 1, P, P, 4, 20, None)
    assert rc != 0 and b"multiple of 16" in lib.lga_last_error_string()


def test_q4_entry_points_reject_the_int8_format(lib):
    rc = lib.lga_quantize(P, 0, P, P, 4, 128, 128, 4, None)
    assert rc != 0 and b"fmt" in lib.lga_last_error_string()


def test_build_model_refuses_int8_moe_and_tensor_parallel(monkeypatch):
    """Sparse MoE and tensor parallelism are refused before the model object exists (no weight materialised)."""
    import torch

    import generate.base as gb
    from lit_gpt import Config

    def boom(*a, **kw):
        raise AssertionError("the model was instantiated before the refusal")

    monkeypatch.setattr(gb, "GPT", boom)
    dev = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="bnb.int8"):
        gb.build_model(Config.from_name("Mixtral-8x7B-v0.1"), quantize="bnb.int8", device=dev)

    class Fabric:
        world_size, global_rank = 2, 0

    with pytest.raises(NotImplementedError, match="bnb.int8"):
        gb.build_model(Config.from_name("Llama-2-7b-hf"), quantize="bnb.int8", device=dev, fabric=Fabric())
