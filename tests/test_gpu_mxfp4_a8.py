"""--quantize mxfp4-a8 on the MI355X: lga_mx8_quantize bit for bit against tests/kv8_spec.py on blocks of 32,
lga_mxfp4_a8_gemm bit for bit on integer-exact operands (tests/exact_operands.py) and against float64 on random ones,
the Linear's dispatch (one row: mxfp4's GEMVs; several: quantize + the block-scaled MFMA GEMM), and a tiny Llama."""

import pytest
import torch

import exact_operands as xo
from kv8_spec import kv8_round
from mxfp4_spec import mx_round
from oracle import synth
from test_gpu_fp8_weights import on_dev, ops, rand_bf16  # noqa: F401 (ops: the loaded-library fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def a8_gemm(ops, x, w, **kw):
    """x (M, K) fp32 exact in bf16, w = (codes, scales) on the device -> quantize + GEMM."""
    return ops.mxfp4_a8_gemm(*ops.mx8_quantize(on_dev(x)), *w, **kw)


@pytest.mark.parametrize("M,K", [(3, 32), (17, 160)])
def test_quantizer_is_exact(ops, M, K):
    g = torch.randn(M * K // 32, 32, generator=torch.Generator().manual_seed(K))
    g = g * torch.exp2((torch.arange(g.shape[0]) % 13 - 6).float()).unsqueeze(1)
    g[0] = 0.0  # amax = 0: s = 1, byte 127
    g[1] = g[1].clamp(-0.5, 0.5) * 2.0 ** -3
    g[1, 5] = -0.875 * 2.0 ** -3  # amax exactly 0.875 2^k: the finer scale
    x = g.view(M, K).bfloat16()
    codes, scales = ops.mx8_quantize(x.to(DEV))
    ref_codes, ref_s, _ = kv8_round(x.reshape(-1, 32))
    assert torch.equal(scales.cpu().int() - 127, torch.frexp(ref_s)[1].view(M, K // 32) - 1)
    assert torch.equal(codes.cpu(), ref_codes.view(M, K))


@pytest.mark.parametrize("M", [2, 17, 129])
@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("K", [96, 160, 1152])  # less than one MFMA step; one step plus one block; nine steps
def test_gemm_is_exact_on_integer_operands(ops, M, N, K):
    w = xo.integer("mxfp4", N, K)
    wd = tuple(t.to(DEV) for t in w.operands)
    x = xo.activations((M, K), seed=K + M)  # {-2 .. 2}: exact in e4m3 under any block scale, mx8(X) = X
    assert torch.equal(kv8_round(x.reshape(-1, 32))[2].view(M, K), x)
    for epilogue in (False, True):
        bias = xo.small_ints((N,), 11) if epilogue else None
        res = xo.small_ints((M, N), 12) if epilogue else None
        xo.assert_order_free(x, w.deq, bias, unit=xo.UNIT["mxfp4"])
        y = a8_gemm(ops, x, wd, bias=on_dev(bias), residual=on_dev(res)).float().cpu()
        assert torch.equal(y, xo.expect_linear(x, w.deq, bias, res)), f"M={M} N={N} K={K} epilogue={epilogue}"


def test_identity_gemm_returns_the_weight(ops):
    """X = I against the full-range weight: one term per output, every code and scale byte in every lane position."""
    N, K = 64, 160
    w = xo.full_range("mxfp4", N, K)
    y = a8_gemm(ops, torch.eye(K), tuple(t.to(DEV) for t in w.operands)).float().cpu()
    bad = ~(y == w.deq.T)
    assert not bool(bad.any()), f"{int(bad.sum())} outputs differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("M", [2, 129])
@pytest.mark.parametrize("K", [160, 1152])
@pytest.mark.parametrize("epilogue", [False, True])
def test_gemm_matches_fp64(ops, M, K, epilogue):
    N = 200
    w = rand_bf16((N, K), N + K, 0.02)
    x = rand_bf16((M, K), M + K, 1.0)
    b = rand_bf16((N,), 2, 0.1) if epilogue else None
    r = rand_bf16((M, N), 3, 1.0) if epilogue else None
    y = a8_gemm(ops, x, ops.mxfp4_quantize(on_dev(w)), bias=on_dev(b), residual=on_dev(r)).float().cpu().double()
    xq = kv8_round(x.reshape(-1, 32))[2].view(M, K)
    wq = mx_round(w.reshape(-1, 32))[2].view(N, K)
    h = xq.double() @ wq.double().T + (b.double() if epilogue else 0.0)
    ref = h.float().bfloat16().double() + (r.double() if epilogue else 0.0)
    err = float(((y - ref).abs() - (ref.abs() + h.abs()) * 2 ** -7).max())  # test_gpu_mxfp4.test_gemm_matches_fp64
    print(f"a8 gemm M={M} N={N} K={K} epilogue={epilogue}: excess {err:.3g}")
    assert err <= 2e-3


@torch.inference_mode()
def test_linear_shares_weights_and_the_one_row_path_with_mxfp4(ops):
    from lit_gpt.quantize import QuantizedPrecision

    lins = {}
    for mode in ("mxfp4", "mxfp4-a8"):
        torch.manual_seed(5)
        holder = torch.nn.Sequential(torch.nn.Linear(160, 200, bias=True)).to(device=DEV, dtype=torch.bfloat16)
        lins[mode] = QuantizedPrecision(mode).convert_module(holder, DEV)[0]
    m4, a8 = lins["mxfp4"], lins["mxfp4-a8"]
    assert torch.equal(m4.qweight, a8.qweight) and torch.equal(m4.scales, a8.scales)
    x = on_dev(rand_bf16((5, 160), 7, 1.0))
    nw = on_dev(1.0 + rand_bf16((160,), 8, 0.1))
    assert torch.equal(a8(x[:1]), m4(x[:1]))
    assert torch.equal(a8(x[:1], norm_weight=nw), m4(x[:1], norm_weight=nw))
    expected = ops.mxfp4_a8_gemm(*ops.mx8_quantize(x), a8.qweight, a8.scales, bias=a8.bias)
    assert torch.equal(a8(x), expected)


@torch.inference_mode()
def test_tiny_llama_graph_equals_eager_and_batches_are_refused():
    from generate.base import generate, generate_batch
    from lit_gpt import GPT, Config
    from lit_gpt.quantize import Mxfp4A8Linear, QuantizedPrecision

    cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512,
                           vocab_size=1000, padding_multiple=64, block_size=64)
    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(cfg, seed=21).items()})
    model = QuantizedPrecision("mxfp4-a8").convert_module(model.to(device=DEV, dtype=torch.bfloat16), DEV).eval()
    assert type(model.lm_head) is Mxfp4A8Linear and type(model.transformer.h[1].mlp.fc_2) is Mxfp4A8Linear
    model.max_seq_length = 40
    prompt = torch.from_numpy(synth.token_ids(12, cfg.vocab_size, seed=21)).to(DEV)
    for kv in (None, torch.float8_e4m3fn):  # the bf16 cache, then --kv_cache fp8: graph replay == eager
        model.set_kv_cache(1, device=DEV, dtype=kv)
        y = {}
        for graph in (True, False):
            for b in model.transformer.h:
                b.attn.kv_cache.reset_parameters()
            y[graph] = generate(model, prompt, 32, temperature=0.0, use_graph=graph).cpu()
        assert y[True].shape == (32,) and torch.equal(y[True], y[False])
    with pytest.raises(NotImplementedError, match="batch size > 1"):
        generate_batch(model, [prompt, prompt], 4, temperature=0.0)
