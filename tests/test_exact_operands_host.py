"""tests/exact_operands.py without a GPU: the order-free condition holds for every dense case of
tests/test_gpu_exact_linear.py (and refuses a case that is too large), an fp32 dot product of those operands has the
int64 product's bits in any order and chunking, the full-range family covers what it claims, and the packing goes back
through the formats' specifications."""

import numpy as np
import pytest
import torch

import exact_operands as xo
from mxfp4_spec import mx_round
from oracle import quant


def _dense_shapes(fmt):
    shapes = set(xo.gemv_shapes(fmt))
    if fmt in ("int4", "nf4", "fp4"):
        shapes |= set(xo.Q4_GEMV_VARIANT_SHAPES)
    for entry, fmts in xo.GEMM_FORMATS.items():
        if fmt in fmts:
            shapes |= set(xo.GEMM_SHAPES[entry])
    return sorted(shapes)


@pytest.mark.parametrize("fmt", xo.FORMATS)
def test_every_dense_case_is_order_free(fmt):
    for N, K in _dense_shapes(fmt):
        for positive in (False, True):  # the SwiGLU forms: positive fc_1 weights and activations
            w = xo.integer(fmt, N, K, seed=1, positive=positive)
            x = xo.activations((8, K), seed=2, positive=positive)
            xo.assert_order_free(x, w.deq, xo.small_ints((N,), 3), xo.UNIT[fmt])
            worst = float((x.abs().double() @ w.deq.abs().double().T).max()) / xo.UNIT[fmt]
            assert worst < 2 ** 24 - 4 / xo.UNIT[fmt]


def test_the_condition_refuses_what_is_too_large_or_not_whole():
    w = torch.full((2, 32768), 64.0)
    x = torch.full((32768,), 8.0)
    with pytest.raises(ValueError, match="not below 2\\^24"):
        xo.assert_order_free(x, w)
    xo.assert_order_free(x[:1024], w[:, :1024])
    with pytest.raises(ValueError, match="not below 2\\^24"):  # the bias counts
        xo.assert_order_free(x[:1024], w[:, :1024], torch.tensor([0.0, 2.0 ** 24]))
    with pytest.raises(ValueError, match="whole number of units"):
        xo.assert_order_free(torch.tensor([0.5, 1.0]), torch.ones(1, 2))
    with pytest.raises(ValueError, match="whole number of units"):
        xo.assert_order_free(torch.ones(2), torch.tensor([[0.25, 1.0]]), unit=0.5)


@pytest.mark.parametrize("fmt", xo.FORMATS)
def test_fp32_dot_has_the_integer_bits_in_any_order(fmt):
    N, K = 5, 32768
    w = xo.integer(fmt, N, K, seed=4)
    x = xo.activations((K,), seed=5)
    xo.assert_order_free(x, w.deq, None, xo.UNIT[fmt])
    unit = xo.UNIT[fmt]
    exact = (np.rint(w.deq.double().numpy() / unit).astype(np.int64) @ x.numpy().astype(np.int64)).astype(np.float64) * unit
    prod = w.deq.numpy() * x.numpy()[None, :]  # fp32 products, exact
    rng = np.random.default_rng(6)
    for chunk in (1, 8, 32, 4096):
        perm = rng.permutation(K)
        p = prod[:, perm].reshape(N, K // chunk, chunk)
        part = np.zeros((N, K // chunk), dtype=np.float32)
        for j in range(chunk):  # sequential fp32 accumulation inside a chunk ...
            part = (part + p[:, :, j]).astype(np.float32)
        tot = np.zeros(N, dtype=np.float32)
        for c in rng.permutation(K // chunk):  # ... then over the chunks in another order
            tot = (tot + part[:, c]).astype(np.float32)
        assert tot.dtype == np.float32 and np.array_equal(tot.astype(np.float64), exact)
    pair = prod.reshape(N, -1, 2).sum(axis=-1, dtype=np.float32)  # a pairwise tree
    while pair.shape[1] > 1:
        pair = pair.reshape(N, -1, 2).sum(axis=-1, dtype=np.float32)
    assert np.array_equal(pair[:, 0].astype(np.float64), exact)


@pytest.mark.parametrize("fmt,N,K", [(fmt, N, K) for fmt in xo.FORMATS for N, K in _dense_shapes(fmt)])
def test_full_range_covers_codes_and_scales(fmt, N, K):
    """Every shape the GPU tests build a full-range weight at (the dense cases run at the same ones)."""
    w = xo.full_range(fmt, N, K)
    nc, C = len(xo._code_list(fmt)), xo.CHUNK[fmt]
    m = xo._coprime_at_most(N, nc)
    for r in range(C):  # every code in every column residue of a 16-B chunk
        assert len(np.unique(w.index[:, r::C])) == nc, f"residue {r}"
    # ... and in the last chunk of a row: n + m r takes m (C - 1) + N values there, which falls short of the code list
    # only for the 5-row weights of the two long lists (fp8: 80 of 254, bf16: 40 of 74)
    last = len(np.unique(w.index[:, -C:]))
    assert last == min(nc, m * (C - 1) + N)
    assert last == nc or (N == 5 and fmt in ("fp8", "bf16"))
    assert bool((w.index[:, 1:] != w.index[:, :-1]).all())  # neighbours differ: a swapped pair shows
    if fmt == "fp8":
        assert not bool(((w.operands[0] & 0x7F) == 0x7F).any())  # never NaN
    if fmt != "bf16":
        lo, hi = xo.EXP_RANGE[fmt]
        assert int(w.exps.min()) == lo and int(w.exps.max()) == hi  # both ends at every shape
        assert len(np.unique(w.exps)) == min(w.exps.size, hi - lo + 1)
    else:
        mag = w.deq.abs()[w.deq != 0]
        assert float(mag.min()) == 2.0 ** -100 and float(mag.max()) == 1.9921875 * 2.0 ** 100
        assert bool((torch.signbit(w.deq) & (w.deq == 0)).any())  # -0
    assert bool(torch.isfinite(w.deq).all())
    assert torch.equal(w.deq.bfloat16().float(), w.deq)
    assert bool(((w.deq == 0) | (w.deq.abs() >= 2.0 ** -126)).all())  # no subnormal weight


def test_full_range_scale_ends_are_the_contract_ends():
    w = xo.full_range("mxfp4", 77, 128)
    assert int(w.operands[1].min()) == 2 and int(w.operands[1].max()) == 252
    w = xo.full_range("fp8", 77, 128)
    s = w.operands[1].float()
    assert float(s.min()) == 2.0 ** -100 and float(s.max()) == 2.0 ** 100
    assert float((w.deq.abs()[w.deq != 0]).min()) >= 2.0 ** -109  # the smallest e4m3 subnormal at the smallest scale
    w = xo.full_range("int4", 77, 128)
    bits = w.operands[1].view(torch.int16).numpy().astype(np.uint16)
    assert len(np.unique(bits & 0x7F)) > 32  # mantissas in use
    w = xo.full_range("nf4", 77, 128)
    assert len(np.unique(w.operands[1].view(torch.int32).numpy() & 0xFFFF)) > 32


@pytest.mark.parametrize("family", ["full_range", "integer"])
@pytest.mark.parametrize("fmt", xo.FORMATS)
def test_packing_round_trips_through_the_specs(fmt, family):
    N, K = 19, 256
    w = getattr(xo, family)(fmt, N, K)
    codes = xo._code_list(fmt)[w.index] if family == "full_range" else xo._integer_codes(fmt, False)[w.index]
    if fmt == "bf16":
        assert torch.equal(w.operands[0].float(), w.deq) and np.array_equal(w.deq.numpy(), codes)
    elif fmt in ("int4", "nf4", "fp4"):
        packed, sc = w.operands
        assert np.array_equal(quant._unpack_nibbles(packed.numpy()), codes)
        raw = sc.view(torch.int16).numpy().view(np.uint16) if fmt == "int4" else sc.numpy()
        deq = quant.dequantize_fmt(packed.numpy(), raw, xo.Q4_FMT[fmt], w.group)
        assert torch.equal(torch.from_numpy(deq).bfloat16().float(), w.deq)
    elif fmt == "fp8":
        c, s = w.operands
        assert np.array_equal(c.numpy(), codes)
        assert torch.equal(c.view(torch.float8_e4m3fn).float() * s.float().repeat_interleave(128, dim=1), w.deq)
    else:
        c, e = w.operands
        assert np.array_equal(np.stack([c.numpy() & 15, c.numpy() >> 4], axis=-1).reshape(N, K), codes)
        if family == "integer":  # what the format's quantizer makes of W' dequantizes to W' again
            assert torch.equal(mx_round(w.deq.view(-1, 32))[2].view(N, K), w.deq)
    if family == "integer":
        units = w.deq / xo.UNIT[fmt]
        assert torch.equal(units, units.round()) and float(units.abs().max()) <= 64


def test_expected_values_follow_the_rounding_points():
    x = torch.tensor([1.0, 2.0])
    w = torch.tensor([[128.0, 0.5], [3.0, -1.0]])
    assert xo.expect_linear(x, w).tolist() == [129.0, 1.0]
    # 129 + 0.5 = 129.5 -> bf16 130 (8 significant bits, the tie to even), then + 1 = 131, exact in 8 bits
    assert xo.expect_linear(x, w, bias=torch.tensor([0.5, 0.0]), residual=torch.tensor([1.0, 0.0])).tolist() == [131.0, 1.0]
    assert xo.expect_linear(x, w, bias=torch.tensor([128.5, 0.0])).tolist() == [258.0, 1.0]  # 257.5 -> 258 (9 bits)
    with pytest.raises(ValueError, match="a < 32"):
        xo.expect_swiglu(x, w, w)
    w1 = torch.tensor([[100.0, 1.5]])
    assert xo.expect_swiglu(x, w1, torch.tensor([[5.0, 0.0]])).tolist() == [516.0]  # 103 * 5 = 515 -> bf16 516


def test_one_hot_columns():
    assert xo.one_hot_columns(96) == list(range(96))
    for K in (4096, 11008, 32768):
        cols = xo.one_hot_columns(K)
        assert cols == sorted(set(cols)) and 0 <= cols[0] and cols[-1] == K - 1 and len(cols) <= 600
        assert {0, 511, 512, 513, 4095, K - 33, K - 2} <= set(cols)
