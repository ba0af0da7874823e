"""--quantize fp8-g128-a8 on the MI355X: lga_fp8_a8_gemm bit for bit on integer-exact operands (tests/exact_operands.py)
and on X = I against the full-range weight (which settles the B operand's lane layout), against float64 on random
operands, the Linear's dispatch (one row: fp8-g128's GEMV; several: lga_mx8_quantize + the fp8 x fp8 MFMA GEMM), and a
tiny Llama: graph replay against eager, and a batch against generate."""

import pytest
import torch

import exact_operands as xo
from kv8_spec import kv8_round
from oracle import synth
from test_gpu_fp8_weights import on_dev, ops, rand_bf16  # noqa: F401 (ops: the loaded-library fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def a8_gemm(ops, x, w, **kw):
    """x (M, K) fp32 exact in bf16, w = (codes, scales) on the device -> quantize + GEMM."""
    return ops.fp8_a8_gemm(*ops.mx8_quantize(on_dev(x)), *w, **kw)


@pytest.mark.parametrize("M", [2, 17, 129])  # a row tail in the 64-row and in the 128-row tile
@pytest.mark.parametrize("N", [64, 200])
@pytest.mark.parametrize("K", [128, 384, 1152])  # one step, three, nine
def test_gemm_is_exact_on_integer_operands(ops, M, N, K):
    w = xo.integer("fp8", N, K)
    wd = tuple(t.to(DEV) for t in w.operands)
    x = xo.activations((M, K), seed=K + M)  # {-2 .. 2}: exact in e4m3 under any block scale, mx8(X) = X
    assert torch.equal(kv8_round(x.reshape(-1, 32))[2].view(M, K), x)
    for epilogue in (False, True):
        bias = xo.small_ints((N,), 11) if epilogue else None
        res = xo.small_ints((M, N), 12) if epilogue else None
        xo.assert_order_free(x, w.deq, bias, unit=xo.UNIT["fp8"])
        y = a8_gemm(ops, x, wd, bias=on_dev(bias), residual=on_dev(res)).float().cpu()
        assert torch.equal(y, xo.expect_linear(x, w.deq, bias, res)), f"M={M} N={N} K={K} epilogue={epilogue}"


def test_identity_gemm_returns_the_weight(ops):
    """X = I against the full-range weight: one term per output, every code and scale byte in every lane position of
    the B operand."""
    N, K = 64, 256
    w = xo.full_range("fp8", N, K)
    y = a8_gemm(ops, torch.eye(K), tuple(t.to(DEV) for t in w.operands)).float().cpu()
    bad = ~(y == w.deq.T)
    assert not bool(bad.any()), f"{int(bad.sum())} outputs differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("M", [2, 129])
@pytest.mark.parametrize("K", [256, 1152])
@pytest.mark.parametrize("epilogue", [False, True])
def test_gemm_matches_fp64(ops, M, K, epilogue):
    N = 200
    w = rand_bf16((N, K), N + K, 0.02)
    x = rand_bf16((M, K), M + K, 1.0)
    b = rand_bf16((N,), 2, 0.1) if epilogue else None
    r = rand_bf16((M, N), 3, 1.0) if epilogue else None
    y = a8_gemm(ops, x, ops.fp8_quantize(on_dev(w)), bias=on_dev(b), residual=on_dev(r)).float().cpu().double()
    xq = kv8_round(x.reshape(-1, 32))[2].view(M, K)
    wq = kv8_round(w.reshape(-1, 128))[2].view(N, K)
    h = xq.double() @ wq.double().T + (b.double() if epilogue else 0.0)
    ref = h.float().bfloat16().double() + (r.double() if epilogue else 0.0)
    err = float(((y - ref).abs() - (ref.abs() + h.abs()) * 2 ** -7).max())  # test_gpu_mxfp4_a8.test_gemm_matches_fp64
    print(f"fp8 a8 gemm M={M} N={N} K={K} epilogue={epilogue}: excess {err:.3g}")
    assert err <= 2e-3


@torch.inference_mode()
def test_linear_shares_weights_and_the_one_row_path_with_fp8_g128(ops):
    from lit_gpt.quantize import QuantizedPrecision

    lins = {}
    for mode in ("fp8-g128", "fp8-g128-a8"):
        torch.manual_seed(5)
        holder = torch.nn.Sequential(torch.nn.Linear(256, 200, bias=True)).to(device=DEV, dtype=torch.bfloat16)
        lins[mode] = QuantizedPrecision(mode).convert_module(holder, DEV)[0]
    f8, a8 = lins["fp8-g128"], lins["fp8-g128-a8"]
    assert torch.equal(f8.qweight, a8.qweight) and torch.equal(f8.scales, a8.scales)
    x = on_dev(rand_bf16((5, 256), 7, 1.0))
    nw = on_dev(1.0 + rand_bf16((256,), 8, 0.1))
    assert torch.equal(a8(x[:1]), f8(x[:1]))
    assert torch.equal(a8(x[:1], norm_weight=nw), f8(x[:1], norm_weight=nw))
    expected = ops.fp8_a8_gemm(*ops.mx8_quantize(x), a8.qweight, a8.scales, bias=a8.bias)
    assert torch.equal(a8(x), expected)


@torch.inference_mode()
def test_tiny_llama_graph_equals_eager_and_a_batch_equals_generate():
    from generate.base import generate, generate_batch
    from lit_gpt import GPT, Config
    from lit_gpt.quantize import Fp8A8Linear, QuantizedPrecision

    cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512,
                           vocab_size=1000, padding_multiple=64, block_size=64)
    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict(cfg, seed=21).items()})
    model = QuantizedPrecision("fp8-g128-a8").convert_module(model.to(device=DEV, dtype=torch.bfloat16), DEV).eval()
    assert type(model.lm_head) is Fp8A8Linear and type(model.transformer.h[1].mlp.fc_2) is Fp8A8Linear
    model.max_seq_length = 40
    prompts = [torch.from_numpy(synth.token_ids(T, cfg.vocab_size, seed=21 + T)).to(DEV) for T in (12, 5)]
    for kv in (None, torch.float8_e4m3fn):  # the bf16 cache, then --kv_cache fp8: graph replay == eager
        model.set_kv_cache(1, device=DEV, dtype=kv)
        y = {}
        for graph in (True, False):
            for b in model.transformer.h:
                b.attn.kv_cache.reset_parameters()
            y[graph] = generate(model, prompts[0], 32, temperature=0.0, use_graph=graph).cpu()
        assert y[True].shape == (32,) and torch.equal(y[True], y[False])
    single = []
    for p in prompts:
        model.set_kv_cache(1, device=DEV)
        single.append(generate(model, p, p.numel() + 16, temperature=0.0).cpu())
    outs = generate_batch(model, prompts, 16, temperature=0.0)
    for b, one in enumerate(single):
        assert torch.equal(outs[b].cpu(), one), b
