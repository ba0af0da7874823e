"""--quantize mxfp6 on the MI355X: the quantizer bit for bit against tests/mxfp6_spec.py; lga_mxfp6_gemv(_swiglu) bit for
bit on integer operands whose sum has one value in any order; the GEMVs and lga_mxfp6_gemm against float64 products on
the spec's dequantized weights with the bounds tests/test_gpu_mxfp4.py applies (the bf16 kernels' bounds: the weight is
exact in bf16); and a tiny Llama against the oracle on those weights."""

import pytest
import torch

from exact_operands import assert_order_free, expect_linear, expect_swiglu, small_ints
from lit_gpt import ops
from mxfp6_spec import E2M3, mx6_pack, mx6_round
from oracle import model as om
from oracle import synth
from parity import check_step
from test_gpu_fp8_weights import on_dev, rand_bf16
from test_mxfp6_host import HAND

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dequant(w):
    """(N, K) -> the weight an mxfp6 Linear holds (fp32, exact in bf16)."""
    return mx6_round(w.reshape(-1, 32))[2].view(w.shape)


@pytest.mark.parametrize("N,K", [(3, 64), (77, 192)])
@pytest.mark.parametrize("in_bf16", [True, False])
def test_quantizer_is_exact(N, K, in_bf16):
    g = torch.randn(N * K // 32, 32, generator=torch.Generator().manual_seed(K)) * 0.02
    g = g * torch.exp2((torch.arange(g.shape[0]) % 13 - 6).float()).unsqueeze(1)
    g[0] = 0.0  # amax = 0: scale byte 127, codes 0
    g[1] = torch.tensor(HAND)  # the ties, the saturating 7.6 and 7.5, the -0.01 that rounds to -0
    g[2] = g[1] * 2.0 ** -9
    w = g.view(N, K)
    if in_bf16:
        w = w.bfloat16()
    codes, scales = ops.mxfp6_quantize(w.to(DEV))
    ref_codes, ref_scales, _ = mx6_round(w.float().view(-1, 32))  # on what the kernel was given
    assert torch.equal(scales.cpu(), ref_scales.view(N, K // 32))
    assert torch.equal(codes.cpu(), mx6_pack(ref_codes.view(N, K)))


INT_CODE = torch.tensor([0, 8, 16, 20, 24, 26, 28, 30])  # the e2m3 codes of the magnitudes 0..7


def integer_weight(N, K, seed, positive=False):
    """Codes written directly (never through the quantizer): integers 0..7 (positive: 1..7, no sign) with random signs,
    scale bytes 124..130 -> (packed codes, scale bytes, W' fp32)."""
    gen = torch.Generator().manual_seed(seed)
    mag = torch.randint(1 if positive else 0, 8, (N, K), generator=gen)
    neg = torch.randint(0, 1 if positive else 2, (N, K), generator=gen).bool()
    e = torch.randint(124, 131, (N, K // 32), generator=gen)
    deq = torch.ldexp(torch.where(neg, -mag, mag).float(), (e - 127).repeat_interleave(32, dim=1))
    return mx6_pack(INT_CODE[mag] + 32 * neg), e.to(torch.uint8), deq


# every term is a multiple of 2^-3 and sum |term| <= 7 * 8 * 8 K: below 2^24 units for K <= 4096 (asserted on the
# operands), so any fp32 summation order gives the exact sum. K = 64 is one unit (every other lane idle), K = 4096 every
# lane of the one-pass class; N = 1 and 77 leave a wave's rows past N.
@pytest.mark.parametrize("N", [1, 77])
@pytest.mark.parametrize("K", [64, 4096])
def test_gemv_and_swiglu_are_exact_on_integer_operands(N, K):
    assert torch.equal(E2M3[INT_CODE], torch.arange(8.0, dtype=torch.float64))
    gen = torch.Generator().manual_seed(N + K)
    c1, s1, w1 = integer_weight(N, K, K + N)
    x = torch.randint(-8, 9, (K,), generator=gen).float()
    b, r = (small_ints((N,), 5), small_ints((N,), 6)) if N == 77 else (None, None)
    assert_order_free(x, w1, b, unit=2.0 ** -3)
    y = ops.mxfp6_gemv(on_dev(x), c1.to(DEV), s1.to(DEV), bias=on_dev(b), residual=on_dev(r))
    assert torch.equal(y.float().cpu(), expect_linear(x, w1, b, r))
    # the pair: fc_1 positive against x in 4..8, so that a >= 64 * 4 * 2^-3 = 32 and bf16(silu(bf16 a)) == bf16 a
    cp, sp, wp = integer_weight(N, K, K + N + 1, positive=True)
    xp = torch.randint(4, 9, (K,), generator=gen).float()
    assert_order_free(xp, wp, unit=2.0 ** -3)
    assert_order_free(xp, w1, unit=2.0 ** -3)
    y = ops.mxfp6_gemv_swiglu(on_dev(xp), cp.to(DEV), sp.to(DEV), c1.to(DEV), s1.to(DEV))
    assert torch.equal(y.float().cpu(), expect_swiglu(xp, wp, w1))


# one row of each dispatch class: a single pass (K <= 4096, 8 rows per wave), several passes (K <= 12288, 4 rows per
# wave; K = 11008 is 172 units, no multiple of the pass of 64) and the long rows that never fuse the norm; K = 64 is one
# unit, every other lane clamped; N = 77 and N = 6 leave a wave's rows past N
GEMV_CASES = [(77, 64, False, False, False), (77, 4096, True, False, True), (77, 11008, False, True, True),
              (77, 11008, True, True, True), (5, 32768, False, False, False), (6, 16384, False, True, True)]


@pytest.mark.parametrize("N,K,norm,bias,res", GEMV_CASES)
def test_gemv_matches_fp64(N, K, norm, bias, res):
    w = rand_bf16((N, K), N + K, 0.02)
    x = rand_bf16((K,), K, 2.0 if norm or res else 1.0)
    nw = 1.0 + rand_bf16((K,), 1, 0.2) if norm else None
    b = rand_bf16((N,), 2, 0.1) if bias else None
    r = rand_bf16((N,), 3, 1.0) if res else None
    codes, scales = ops.mxfp6_quantize(on_dev(w))
    y = ops.mxfp6_gemv(on_dev(x), codes, scales, bias=on_dev(b), residual=on_dev(r), norm_weight=on_dev(nw),
                       eps=1e-5).float().cpu().double()
    xn = om.rms_norm(x.bfloat16(), nw.bfloat16(), 1e-5).float() if norm else x
    h = dequant(w).double() @ xn.double() + (b.double() if bias else 0.0)
    if not (norm or bias or res):  # test_bf16_gemv_matches_reference: output rounding + fp32 accumulation order
        tol = h.abs() * 2 ** -7 + 1e-3 * (K / 4096) ** 0.5 * 0.02 * float(x.abs().mean()) * 4
        err = float(((y - h).abs() - tol).max())
        print(f"gemv N={N} K={K}: max |y - ref| - tol = {err:.3g}")
        assert err <= 0
    else:  # test_bf16_gemv_fused_norm_residual_bias
        h = h.float().bfloat16().double()
        ref = h + (r.double() if res else 0.0)
        err = float(((y - ref).abs() - ref.abs() * 2 ** -7 - h.abs() * 2 ** -7).max())
        print(f"gemv N={N} K={K} norm={norm} bias={bias} res={res}: excess {err:.3g}")
        assert err <= 2e-3


@pytest.mark.parametrize("N,K,norm", [(77, 64, False), (77, 4096, True), (77, 11008, True), (77, 11008, False),
                                      (6, 16384, False)])
def test_gemv_swiglu_matches_fp64(N, K, norm):
    w1, w2 = rand_bf16((N, K), N + K, 0.02), rand_bf16((N, K), N + K + 1, 0.02)
    x = rand_bf16((K,), K, 1.0)
    nw = 1.0 + rand_bf16((K,), 1, 0.1) if norm else None
    c1, s1 = ops.mxfp6_quantize(on_dev(w1))
    c2, s2 = ops.mxfp6_quantize(on_dev(w2))
    y = ops.mxfp6_gemv_swiglu(on_dev(x), c1, s1, c2, s2, norm_weight=on_dev(nw)).float().cpu().double()
    xn = (om.rms_norm(x.bfloat16(), nw.bfloat16(), 1e-5).float() if norm else x).double()
    a, b = dequant(w1).double() @ xn, dequant(w2).double() @ xn
    ref = a / (1 + torch.exp(-a)) * b
    err = float(((y - ref).abs() - ref.abs() * 2 ** -6).max())  # test_bf16_gemv_swiglu
    print(f"swiglu N={N} K={K} norm={norm}: excess {err:.3g}")
    assert err <= 1e-3


# K = 64 is half a K step of 128 (k-groups 2 and 3 multiply zero codes), K = 192 a whole step then a half one, K = 1152
# nine whole steps; N = 200 and the Ms leave rows of a tile past N and M; M = 129 takes the 128-row tile
@pytest.mark.parametrize("M", [2, 17, 129])
@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("K", [64, 192, 1152])
@pytest.mark.parametrize("epilogue", [False, True])
def test_gemm_matches_fp64(M, N, K, epilogue):
    w = rand_bf16((N, K), N + K, 0.02)
    x = rand_bf16((M, K), M + K, 1.0)
    b = rand_bf16((N,), 2, 0.1) if epilogue else None
    r = rand_bf16((M, N), 3, 1.0) if epilogue else None
    codes, scales = ops.mxfp6_quantize(on_dev(w))
    y = ops.mxfp6_gemm(on_dev(x), codes, scales, bias=on_dev(b), residual=on_dev(r)).float().cpu().double()
    h = x.double() @ dequant(w).double().T + (b.double() if epilogue else 0.0)
    ref = h.float().bfloat16().double() + (r.double() if epilogue else 0.0)
    err = float(((y - ref).abs() - (ref.abs() + h.abs()) * 2 ** -7).max())  # test_bf16_gemm_matches_reference
    print(f"gemm M={M} N={N} K={K} epilogue={epilogue}: excess {err:.3g}")
    assert err <= 2e-3


@torch.inference_mode()
def test_tiny_llama_matches_oracle_graph_equals_eager_and_batches_are_refused():
    from generate.base import generate, generate_batch
    from lit_gpt import GPT, Config
    from lit_gpt.quantize import Mxfp6Linear, QuantizedPrecision

    cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512,
                           vocab_size=1000, padding_multiple=64, block_size=64)
    sd = synth.state_dict(cfg, seed=21)
    T, N = 12, 9
    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = QuantizedPrecision("mxfp6").convert_module(model.to(device=DEV, dtype=torch.bfloat16), DEV).eval()
    assert all(isinstance(m, Mxfp6Linear) for m in model.modules() if hasattr(m, "in_features"))
    assert isinstance(model.lm_head, Mxfp6Linear) and isinstance(model.transformer.h[1].mlp.fc_2, Mxfp6Linear)
    model.max_seq_length = 40
    model.set_kv_cache(1, device=DEV)
    prompt = torch.from_numpy(synth.token_ids(T, cfg.vocab_size, seed=21))
    stream = torch.from_numpy(synth.token_ids(N, cfg.vocab_size, seed=22))  # forced continuation
    steps = [(prompt, torch.arange(T))] + [(stream[i:i + 1], torch.tensor([T + i])) for i in range(N - 1)]
    got = [model(idx.view(1, -1).to(DEV), pos.to(DEV))[0, -1].float().cpu() for idx, pos in steps]

    def deq(k, v):  # as test_gpu_model.py's oracle_for: every Linear weight, as the bf16 model holds it, quantized
        if k.endswith(".weight") and v.ndim == 2 and not k.startswith("transformer.wte"):
            return dequant(torch.from_numpy(v).bfloat16().float()).numpy()
        return v

    exp = {}
    for dt in (torch.bfloat16, torch.float64):
        ref = om.OracleGPT(cfg, sd, dtype=dt, weight_override=deq)
        ref.set_kv_cache(T + N)
        exp[dt] = [ref.forward(idx, pos)[-1] for idx, pos in steps]
    for s, g in enumerate(got):
        check_step(g, exp[torch.bfloat16][s], exp[torch.float64][s], f"mxfp6 step {s}")

    for kv in (None, torch.float8_e4m3fn):  # the bf16 cache, then --kv_cache fp8: graph replay == eager
        model.set_kv_cache(1, device=DEV, dtype=kv)
        y = {}
        for graph in (True, False):
            for b in model.transformer.h:
                b.attn.kv_cache.reset_parameters()
            y[graph] = generate(model, prompt.to(DEV), 32, temperature=0.0, use_graph=graph).cpu()
        assert y[True].shape == (32,) and torch.equal(y[True], y[False])

    with pytest.raises(NotImplementedError, match="batch size > 1"):  # no multi-row mxfp6 GEMV
        generate_batch(model, [prompt.to(DEV), prompt.to(DEV)], 4, temperature=0.0)
