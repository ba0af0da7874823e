"""Batched decode on the MI355X: the multi-row 4-bit GEMVs (lga_q4_gemv_rows, lga_q4_gemv_swiglu_rows), the batched
model step, ``BatchDecodeGraph`` and ``generate_batch``.

The promise under test: batching never changes a sequence's result. Row r of a rows launch has the bits of the one-row
launch on x[r] (``torch.equal``, every geometry the default dispatch picks), and sequence b of a batch gets the tokens
``generate`` gives that prompt alone. The one-row path is pinned to the oracle elsewhere (tests/test_gpu_kernels.py,
tests/test_gpu_model.py), so only one fp64 check is repeated here.
"""

import numpy as np
import pytest
import torch

from oracle import quant, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORMATS = [(0, 128), (1, 64), (3, 64), (0, 32)]
ROWS = [1, 2, 3, 5, 8]
MAX_M = 8


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def bf16_np(x: np.ndarray) -> np.ndarray:
    return quant.bf16_bits_to_f32(quant.f32_to_bf16_bits(x))


def to_dev_bf16(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(torch.bfloat16)


_CACHE = {}


def _weights(N, K, name):
    """(N, K) fp32 device weight from oracle.synth: at most 1024 generated rows, tiled with a per-tile gain so tall
    matrices cost no more host time than small ones (every row still differs from its neighbours)."""
    key = ("w", N, K, name)
    if key not in _CACHE:
        n0 = min(N, 1024)
        base = torch.from_numpy(synth.normal((n0, K), f"{name}{N}x{K}", 7, 0.02)).to(DEV)
        reps = (N + n0 - 1) // n0
        gain = 1.0 + 0.03 * torch.arange(reps, device=DEV, dtype=torch.float32)
        _CACHE[key] = (base.unsqueeze(0) * gain.view(-1, 1, 1)).reshape(reps * n0, K)[:N].contiguous()
    return _CACHE[key]


def _quantized(ops, N, K, fmt, group, name="w"):
    key = ("q", N, K, fmt, group, name)
    if key not in _CACHE:
        _CACHE[key] = ops.quantize(_weights(N, K, name), fmt, group)
    return _CACHE[key]


def _vec(shape, name, std=1.0):
    key = ("v", shape, name, std)
    if key not in _CACHE:
        _CACHE[key] = to_dev_bf16(synth.normal(shape, name, 5, std))
    return _CACHE[key]


# (N, K, residual, bias, norm): the smallest shapes that select each geometry of the default dispatch
SHAPES = [
    (1000, 256, False, False, False),    # 4 rows per wave, 1 chunk per lane
    (77, 1376, False, False, False),     # N tail; 43 chunks: clamped lanes
    (2048, 512, True, False, False),     # "half" form, out-projection class
    (4096, 512, False, False, True),     # "half" form, qkv class
    (8, 512, False, False, False),       # N <= 64 gate class
    (640, 11008, True, True, False),     # 6 chunks per lane; a row too long to stage 8 at once
    (130, 18432, False, False, False),   # 16 chunks per lane
    (24000, 4128, False, False, False),  # "big" one-shot
    (24000, 256, False, False, False),   # streaming, 1 chunk per lane
    (24000, 2080, False, False, True),   # streaming, 2 chunks per lane
]


def _case(ops, shape, fmt, group):
    """Inputs of one shape (8 activation rows) and the one-row launches' outputs, computed once per (shape, format)."""
    key = ("case", shape, fmt, group)
    if key not in _CACHE:
        N, K, res, bias, norm = shape
        qw, sc = _quantized(ops, N, K, fmt, group)
        kw = dict(bias=_vec((N,), "bias", 0.1) if bias else None,
                  norm_weight=(1.0 + _vec((K,), "nw", 0.2).float()).to(torch.bfloat16) if norm else None, eps=1e-5)
        x = _vec((MAX_M, K), f"x{K}", 1.0)
        r = _vec((MAX_M, N), f"r{N}", 1.0) if res else None
        one = torch.stack([ops.q4_gemv(x[i], qw, sc, N, K, group, fmt, residual=None if r is None else r[i],
                                       variant=-1, **kw) for i in range(MAX_M)])
        _CACHE[key] = (qw, sc, x, r, kw, one)
    return _CACHE[key]


@pytest.mark.parametrize("fmt,group", FORMATS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_bit_identical_to_one_row_launch(ops, shape, M, fmt, group):
    N, K = shape[:2]
    if K % group:
        pytest.skip("group does not divide K")
    qw, sc, x, r, kw, one = _case(ops, shape, fmt, group)
    y = ops.q4_gemv_rows(x[:M].contiguous(), qw, sc, N, K, group, fmt,
                         residual=None if r is None else r[:M].contiguous(), **kw)
    assert y.shape == (M, N)
    for i in range(M):
        assert torch.equal(y[i], one[i]), (i, int((y[i] != one[i]).sum()))


# (N, K, norm): one-shot, one-shot with the norm, streaming, "big"
DUAL_SHAPES = [(1000, 256, False), (1376, 1024, True), (8192, 256, False), (12000, 4128, False)]


@pytest.mark.parametrize("fmt,group", FORMATS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("shape", DUAL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_swiglu_rows_bit_identical_to_one_row_launch(ops, shape, M, fmt, group):
    N, K, norm = shape
    if K % group:
        pytest.skip("group does not divide K")
    key = ("dual", shape, fmt, group)
    if key not in _CACHE:
        q1, s1 = _quantized(ops, N, K, fmt, group, "w1")
        q2, s2 = _quantized(ops, N, K, fmt, group, "w2")
        nw = (1.0 + _vec((K,), "nw", 0.2).float()).to(torch.bfloat16) if norm else None
        x = _vec((MAX_M, K), f"x{K}", 1.0)
        one = torch.stack([ops.q4_gemv_swiglu(x[i], q1, s1, q2, s2, N, K, group, fmt, norm_weight=nw, variant=-1)
                           for i in range(MAX_M)])
        _CACHE[key] = (q1, s1, q2, s2, nw, x, one)
    q1, s1, q2, s2, nw, x, one = _CACHE[key]
    y = ops.q4_gemv_swiglu_rows(x[:M].contiguous(), q1, s1, q2, s2, N, K, group, fmt, norm_weight=nw)
    assert y.shape == (M, N)
    for i in range(M):
        assert torch.equal(y[i], one[i]), (i, int((y[i] != one[i]).sum()))


@pytest.mark.parametrize("shape", [SHAPES[5], SHAPES[9]], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_batch_invariance(ops, shape):
    """Row r of an M = 8 launch equals the same row launched at M = 2, in slot 0 and in slot 1."""
    N, K = shape[:2]
    fmt, group = 0, 32
    qw, sc, x, r, kw, _ = _case(ops, shape, fmt, group)
    y8 = ops.q4_gemv_rows(x, qw, sc, N, K, group, fmt, residual=r, **kw)
    for i in (0, 3, 7):
        j = (i + 1) % MAX_M
        for pair in ((i, j), (j, i)):
            sel = torch.tensor(pair, device=DEV)
            y2 = ops.q4_gemv_rows(x[sel].contiguous(), qw, sc, N, K, group, fmt,
                                  residual=None if r is None else r[sel].contiguous(), **kw)
            assert torch.equal(y2[pair.index(i)], y8[i])


@pytest.mark.parametrize("fmt,group", FORMATS)
def test_rows_match_fp64_reference(ops, fmt, group):
    """(640, 4096), M = 5 against fp64 on the same bf16 inputs, the tolerance of test_gemv_matches_reference."""
    N, K, M = 640, 4096, 5
    w = synth.normal((N, K), "ref640", 7, 0.02)
    x = bf16_np(synth.normal((M, K), "xref", 5, 1.0))
    qw, sc = ops.quantize(torch.from_numpy(w).to(DEV), fmt, group)
    y = ops.q4_gemv_rows(to_dev_bf16(x), qw, sc, N, K, group, fmt).float().cpu().numpy()
    wdeq = quant.dequantize_fmt(*quant.quantize_fmt(w, fmt, group), fmt, group)
    for i in range(M):
        ref = x[i].astype(np.float64) @ wdeq.astype(np.float64).T
        # bf16 output rounding (2^-8 relative) + fp32 accumulation differences
        tol = np.abs(ref) * 2 ** -7 + 1e-3 * np.sqrt(K / 4096) * 0.02 * np.abs(x[i]).mean() * 4
        print(f"row {i}: max excess {float(np.max(np.abs(y[i] - ref) - tol)):.3e}")
        assert np.all(np.abs(y[i] - ref) <= tol), float(np.max(np.abs(y[i] - ref) - tol))


def test_rows_argument_errors(ops):
    N, K, group, fmt = 64, 256, 128, 0
    qw, sc = _quantized(ops, N, K, fmt, group)
    x = _vec((MAX_M + 1, K), "xerr", 1.0)
    err = (ValueError, RuntimeError)
    with pytest.raises(err):
        ops.q4_gemv_rows(x[:0], qw, sc, N, K, group, fmt)  # M = 0
    with pytest.raises(err):
        ops.q4_gemv_rows(x, qw, sc, N, K, group, fmt)  # M = 9
    with pytest.raises(err):
        ops.q4_gemv_rows(_vec((K, 2), "xt", 1.0).t(), qw, sc, N, K, group, fmt)  # (2, K), not contiguous
    with pytest.raises(err):
        ops.q4_gemv_rows(x[:2].contiguous(), qw, sc, N, K, group, fmt, residual=_vec((3, N), "rerr", 1.0))
    with pytest.raises(err):
        ops.q4_gemv_rows(x[:2].contiguous(), qw, sc, N, K, group, 2)  # fmt 2: bf16 weights have no rows GEMV
    with pytest.raises(err):
        ops.q4_gemv_rows(x[:2].contiguous(), qw, sc, N, K, group, fmt,
                         out=torch.empty(3, N, dtype=torch.bfloat16, device=DEV))
    for bad in (x[:0], x, _vec((K, 2), "xt", 1.0).t()):
        with pytest.raises(err):
            ops.q4_gemv_swiglu_rows(bad, qw, sc, qw, sc, N, K, group, fmt)
    with pytest.raises(err):
        ops.q4_gemv_swiglu_rows(x[:2].contiguous(), qw, sc, qw, sc, N, K, group, 2)
    lib = ops.load_library()  # the C entry points check the same before any launch
    p = torch.zeros(64, dtype=torch.uint8, device=DEV).data_ptr()
    for M in (0, 9):
        assert lib.lga_q4_gemv_rows(p, p, p, None, None, None, 1e-5, p, M, N, K, group, fmt, None) != 0
        assert b"1..8" in lib.lga_last_error_string()
        assert lib.lga_q4_gemv_swiglu_rows(p, p, p, p, p, None, 1e-5, p, M, N, K, group, fmt, None) != 0
    assert lib.lga_q4_gemv_rows(p, p, p, None, None, None, 1e-5, p, 2, N, K, group, 2, None) != 0


# ------------------------------------------------------------------------------------------------ model
S_MAX = 96
PROMPT_LENS = (5, 16, 33)
MODELS = [("int4-g128", 8), ("nf4", 8), ("int4-g128", 4)]  # (mode, n_query_groups): MHA in both formats, one GQA


def _model(mode, groups):
    from generate.base import build_model
    from lit_gpt import Config

    key = ("model", mode, groups)
    if key not in _CACHE:
        cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=groups,
                               intermediate_size=2816)
        _CACHE[key] = build_model(cfg, quantize=mode, device=torch.device(DEV), max_seq_length=S_MAX)
    return _CACHE[key]


def _prompts(vocab, lens=PROMPT_LENS):
    return [torch.from_numpy(synth.token_ids(T, vocab, seed=20 + T)).to(DEV) for T in lens]


def _cache(model, B):
    model.set_kv_cache(batch_size=B, device=torch.device(DEV))


@pytest.mark.parametrize("mode,groups", MODELS)
def test_batched_step_logits_equal_single_sequence(ops, mode, groups):
    model = _model(mode, groups)
    prompts = _prompts(model.config.vocab_size)
    single = []
    with torch.inference_mode():
        for p in prompts:
            _cache(model, 1)
            T = p.numel()
            pre = model(p.view(1, -1), torch.arange(T, device=DEV), last_token_only=True)
            tok = ops.argmax(pre.view(-1).contiguous()).to(torch.int32)
            single.append((pre, tok, model(tok.view(1, 1), torch.tensor([T], device=DEV))))
        _cache(model, len(prompts))
        for b, p in enumerate(prompts):
            T = p.numel()
            pre = model(p.view(1, -1), torch.arange(T, device=DEV), last_token_only=True, kv_slot=b)
            assert torch.equal(pre, single[b][0])
        idx = torch.cat([s[1] for s in single]).view(-1, 1)
        pos = torch.tensor([p.numel() for p in prompts], device=DEV)
        for shape in ((len(prompts),), (len(prompts), 1)):  # one position per sequence, either layout
            logits = model(idx, pos.view(shape))
            assert logits.shape == (len(prompts), 1, model.config.padded_vocab_size)
            for b in range(len(prompts)):
                assert torch.equal(logits[b], single[b][2][0]), b
        # shared positions: (B, T > 1) rows are the B = 1 prefill on slot b; (B, 1) with a (1,) position
        T = prompts[0].numel()
        two = torch.stack([prompts[0], prompts[1][:T]])
        full = model(two, torch.arange(T, device=DEV))
        last = model(two, torch.arange(T, device=DEV), last_token_only=True)
        assert full.shape[:2] == (2, T) and last.shape[:2] == (2, 1)
        assert torch.equal(last[0], single[0][0][0])
        shared = model(idx[:2], torch.tensor([T], device=DEV))
        assert torch.equal(shared[0], single[0][2][0])
    _cache(model, 1)


def _single_runs(model, prompts, new, **kw):
    from generate.base import generate

    outs = []
    for p in prompts:
        _cache(model, 1)
        outs.append(generate(model, p, p.numel() + new, **kw).cpu())
    return outs


@pytest.mark.parametrize("mode,groups", MODELS)
def test_generate_batch_greedy_equals_generate(mode, groups):
    from generate.base import generate_batch

    model = _model(mode, groups)
    prompts = _prompts(model.config.vocab_size)
    new = 24
    single = _single_runs(model, prompts, new, temperature=0.0)
    outs = generate_batch(model, prompts, new, temperature=0.0)
    for b, p in enumerate(prompts):
        assert outs[b].numel() == p.numel() + new
        assert torch.equal(outs[b].cpu(), single[b]), b
    # an eos from sequence 1's own decoded tokens (the prefill's token is never tested, as in generate)
    T1 = prompts[1].numel()
    eos = int(single[1][T1 + 1 + 9])
    cut = _single_runs(model, prompts, new, temperature=0.0, eos_id=eos)
    assert cut[1].numel() < T1 + new and int(cut[1][-1]) == eos
    outs = generate_batch(model, prompts, new, temperature=0.0, eos_id=eos)
    for b in range(len(prompts)):
        assert torch.equal(outs[b].cpu(), cut[b]), b
    _cache(model, 1)


def test_batched_graph_equals_eager():
    from generate.base import generate_batch

    model = _model("int4-g128", 8)
    prompts = _prompts(model.config.vocab_size)
    graph = generate_batch(model, prompts, 24, temperature=0.0)
    eager = generate_batch(model, prompts, 24, temperature=0.0, use_graph=False)
    for g, e in zip(graph, eager):
        assert torch.equal(g, e)
    _cache(model, 1)


def test_generate_batch_sampling_equals_single_path_per_seed():
    from generate.base import SamplerRNG, generate, generate_batch

    model = _model("nf4", 8)
    prompt = _prompts(model.config.vocab_size, (9,))[0]
    seeds = [1234, 99]
    outs = generate_batch(model, [prompt, prompt.clone()], 24, temperature=0.8, top_k=200, seeds=seeds)
    assert not torch.equal(outs[0], outs[1])
    for b, s in enumerate(seeds):
        _cache(model, 1)
        one = generate(model, prompt, prompt.numel() + 24, temperature=0.8, top_k=200, rng=SamplerRNG(DEV, seed=s))
        assert torch.equal(outs[b], one), b
    _cache(model, 1)


def test_batch_refusals():
    from generate.base import build_model, generate_batch
    from lit_gpt import Config

    dev = torch.device(DEV)
    model = _model("int4-g128", 8)
    _cache(model, 9)
    with pytest.raises(NotImplementedError, match="at most 4"):
        model(torch.zeros(9, 1, dtype=torch.int32, device=DEV), torch.tensor([0], device=DEV))
    with pytest.raises(NotImplementedError, match="at most 4"):
        generate_batch(model, _prompts(model.config.vocab_size, (4,)) * 9, 4, temperature=0.0)
    _cache(model, 1)
    tiny = dict(n_layer=1, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512, vocab_size=1000,
                padding_multiple=64, block_size=64)
    two = torch.zeros(2, 1, dtype=torch.int32, device=DEV)
    for name, mode in (("Llama-2-7b-hf", None), ("Llama-2-7b-hf", "bnb.int8"), ("Mixtral-8x7B-v0.1", "int4-g128")):
        m = build_model(Config.from_name(name, **tiny), quantize=mode, device=dev, max_seq_length=32)
        m.set_kv_cache(batch_size=2, device=dev)
        with pytest.raises(NotImplementedError, match="batch size > 1"):
            m(two, torch.tensor([0], device=DEV))
