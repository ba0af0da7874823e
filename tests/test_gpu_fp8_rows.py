"""The fp8-g128 multi-row decode GEMVs on the MI355X: lga_fp8_gemv_rows / lga_fp8_gemv_swiglu_rows bit for bit against the
one-row launches on every row (each dispatch class, with N and K tails), against float64 products on the dequantized
weights, and the routes built on them (batched, continuous, samples, speculative) token for token against generate."""

import pytest
import torch

from oracle import model as om
from oracle import synth
from test_gpu_fp8_weights import dequant, on_dev, rand_bf16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S_MAX, NEW = 96, 24
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops
    _ops.load_library()
    return _ops


def _case(ops, N, K, norm, bias, res, dual=False):
    """CPU inputs (8 activation rows, each with its own seed and scale) and the quantized weights, once per shape."""
    key = (N, K, norm, bias, res, dual)
    if key not in _CACHE:
        w = [rand_bf16((N, K), N + K + i, 0.02) for i in range(2 if dual else 1)]
        std = 2.0 if (norm or res) and not dual else 1.0
        x = torch.stack([rand_bf16((K,), 100 * K + r, std * (1 + 0.5 * r)) for r in range(8)])
        c = {"w": w, "x": x, "q": [t for wi in w for t in ops.fp8_quantize(on_dev(wi))],
             "nw": 1.0 + rand_bf16((K,), 1, 0.2) if norm else None,
             "b": rand_bf16((N,), 2, 0.1) if bias else None, "r": rand_bf16((8, N), 3, 1.0) if res else None}
        _CACHE[key] = c
    return _CACHE[key]


# one shape per dispatch class: K = 128 clamps all but 8 lanes, 4096 is one pass, 11008 several (no multiple of the
# pass), 16384 the long rows without the norm; N = 77 and N = 6 leave a wave's rows past N
@pytest.mark.parametrize("N,K,norm,bias,res", [(77, 128, False, False, False), (77, 4096, True, False, True),
                                               (77, 11008, True, True, True), (6, 16384, False, True, True)])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
def test_rows_equal_the_one_row_launch(ops, M, N, K, norm, bias, res):
    c = _case(ops, N, K, norm, bias, res)
    x, r = on_dev(c["x"][:M]), on_dev(c["r"][:M]) if res else None
    kw = dict(bias=on_dev(c["b"]), norm_weight=on_dev(c["nw"]), eps=1e-5)
    y = ops.fp8_gemv_rows(x, *c["q"], residual=r, **kw)
    assert y.shape == (M, N)
    for i in range(M):
        one = ops.fp8_gemv(x[i], *c["q"], residual=r[i] if res else None, **kw)
        assert torch.equal(y[i].view(torch.int16), one.view(torch.int16)), i


@pytest.mark.parametrize("N,K,norm", [(77, 128, False), (77, 4096, True), (77, 11008, True), (6, 16384, False)])
@pytest.mark.parametrize("M", [2, 5, 8])
def test_swiglu_rows_equal_the_one_row_launch(ops, M, N, K, norm):
    c = _case(ops, N, K, norm, False, False, dual=True)
    x, nw = on_dev(c["x"][:M]), on_dev(c["nw"])
    y = ops.fp8_gemv_swiglu_rows(x, *c["q"], norm_weight=nw)
    assert y.shape == (M, N)
    for i in range(M):
        one = ops.fp8_gemv_swiglu(x[i], *c["q"], norm_weight=nw)
        assert torch.equal(y[i].view(torch.int16), one.view(torch.int16)), i


def _normed(c, i):
    x = c["x"][i]
    return (x if c["nw"] is None else om.rms_norm(x.bfloat16(), c["nw"].bfloat16(), 1e-5).float()).double()


@pytest.mark.parametrize("N,K,norm", [(77, 128, False), (77, 4096, True)])
@pytest.mark.parametrize("dual", [False, True], ids=["gemv", "swiglu"])
def test_rows_match_fp64(ops, N, K, norm, dual):
    """test_gpu_fp8_weights' bounds (test_gemv_matches_fp64's two, test_gemv_swiglu_matches_fp64's), row by row, M = 3."""
    res = norm and not dual
    c = _case(ops, N, K, norm, False, res, dual=dual)
    x, nw = on_dev(c["x"][:3]), on_dev(c["nw"])
    y = (ops.fp8_gemv_swiglu_rows(x, *c["q"], norm_weight=nw) if dual else
         ops.fp8_gemv_rows(x, *c["q"], residual=on_dev(c["r"][:3]) if res else None, norm_weight=nw, eps=1e-5))
    y = y.float().cpu().double()
    for i in range(3):
        xn = _normed(c, i)
        h = dequant(c["w"][0]).double() @ xn
        if dual:
            ref = h / (1 + torch.exp(-h)) * (dequant(c["w"][1]).double() @ xn)
            err, bound = float(((y[i] - ref).abs() - ref.abs() * 2 ** -6).max()), 1e-3
        elif not res:
            tol = h.abs() * 2 ** -7 + 1e-3 * (K / 4096) ** 0.5 * 0.02 * float(c["x"][i].abs().mean()) * 4
            err, bound = float(((y[i] - h).abs() - tol).max()), 0.0
        else:
            h = h.float().bfloat16().double()
            ref = h + c["r"][i].double()
            err, bound = float(((y[i] - ref).abs() - ref.abs() * 2 ** -7 - h.abs() * 2 ** -7).max()), 2e-3
        print(f"rows dual={dual} N={N} K={K} norm={norm} row {i}: excess {err:.3g} (bound {bound})")
        assert err <= bound


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def model():
    from generate.base import build_model
    from lit_gpt import Config
    cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=8, intermediate_size=2816)
    return build_model(cfg, quantize="fp8-g128", device=DEV, max_seq_length=S_MAX)


def _prompts(model, lens):
    return [torch.from_numpy(synth.token_ids(T, model.config.vocab_size, seed=20 + T)).to(DEV) for T in lens]


def _single(model, prompt, new=NEW, seed=None, kv=None, **kw):
    """``generate`` alone on a fresh one-slot cache (``kv``: the cache dtype)."""
    from generate.base import SamplerRNG, generate
    model.set_kv_cache(batch_size=1, device=DEV, dtype=kv)
    rng = None if seed is None else SamplerRNG(DEV, seed=seed)
    return generate(model, prompt, prompt.numel() + new, rng=rng, **kw).cpu()


@pytest.mark.parametrize("kv", [None, torch.float8_e4m3fn], ids=["bf16", "fp8"])
def test_generate_batch_greedy_equals_generate(model, kv):
    from generate.base import generate_batch
    prompts = _prompts(model, (5, 33, 18))
    single = [_single(model, p, kv=kv, temperature=0.0) for p in prompts]
    outs = generate_batch(model, prompts, NEW, temperature=0.0)
    for b, one in enumerate(single):
        assert torch.equal(outs[b].cpu(), one), b
    model.set_kv_cache(batch_size=1, device=DEV)


def test_generate_batch_sampling_equals_generate_per_seed(model):
    from generate.base import generate_batch
    prompt, seeds = _prompts(model, (9,))[0], [1234, 99]
    outs = generate_batch(model, [prompt, prompt.clone()], NEW, temperature=0.8, top_k=50, seeds=seeds)
    assert not torch.equal(outs[0], outs[1])
    for b, s in enumerate(seeds):
        assert torch.equal(outs[b].cpu(), _single(model, prompt, seed=s, temperature=0.8, top_k=50)), b


def test_generate_continuous_equals_generate(model):
    from generate.base import generate_continuous
    prompts, budgets = _prompts(model, (5, 33, 18, 7, 12)), [10, 24, 6, 16, 12]
    outs = generate_continuous(model, prompts, budgets, batch_size=2, temperature=0.0)
    for i, (p, n) in enumerate(zip(prompts, budgets)):
        assert torch.equal(outs[i].cpu(), _single(model, p, new=n, temperature=0.0)), i


def test_generate_speculative_equals_generate(model):
    from generate.speculative import NgramDrafter, generate_speculative
    prompt = _prompts(model, (6,))[0].repeat(4)  # repeats: the drafter proposes from the first round on
    ref = _single(model, prompt, temperature=0.0)
    model.set_kv_cache(batch_size=1, device=DEV)
    stats = {}
    y = generate_speculative(model, prompt, prompt.numel() + NEW, NgramDrafter(), speculate=4, stats=stats)
    assert torch.equal(y.cpu(), ref)
    assert stats["proposed"] > 0 and stats["rounds"] < NEW, stats  # windows of more than one row ran and paid


@pytest.mark.parametrize("share", [True, False])
def test_generate_samples_equal_generate_per_seed(model, share):
    from generate.base import generate_samples
    prompt, seeds = _prompts(model, (33,))[0], [1234, 99, 7]
    ones = [_single(model, prompt, seed=s, temperature=0.8, top_k=50) for s in seeds]
    model.set_kv_cache(batch_size=1, device=DEV)
    outs = generate_samples(model, prompt, NEW, 3, temperature=0.8, top_k=50, seeds=seeds, share=share)
    for y, one in zip(outs, ones):
        assert torch.equal(y.cpu(), one)
    model.set_kv_cache(batch_size=1, device=DEV)
