"""n samples of one prompt (``generate_samples``) on the MI355X: one prefill, the samples decoded together behind the
one prefix, through the shared-prefix attention launch (``share=True``) or copies of the prompt's rows
(``share=False``).

The promise under test: sample i is, token for token, what ``generate`` returns for that prompt with sample i's seed.
"""

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
S_MAX = 96
NEW = 24
PROMPT_LENS = (5, 33)
MODELS = [("int4-g128", 8), ("int4-g128", 4)]  # (mode, n_query_groups): MHA and one GQA
SEEDS = [1234, 99, 7, 1234]

_CACHE = {}


def _model(mode, groups, kv_cache="bf16", n_embd=1024):
    from generate.base import build_model
    from lit_gpt import Config

    key = (mode, groups, kv_cache, n_embd)
    if key not in _CACHE:
        cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=n_embd, n_head=8, n_query_groups=groups,
                               intermediate_size=2816)
        _CACHE[key] = build_model(cfg, quantize=mode, device=torch.device(DEV), max_seq_length=S_MAX,
                                  kv_cache=kv_cache)
    return _CACHE[key]


def _prompt(vocab, T):
    return torch.from_numpy(synth.token_ids(T, vocab, seed=20 + T)).to(DEV)


def _reset(model):
    kv = model.transformer.h[0].attn.kv_cache
    model.set_kv_cache(batch_size=1, device=torch.device(DEV), dtype=kv.cache_dtype)


def _single(model, prompt, seeds=None, **kw):
    """``generate`` per seed (None: greedy, once), each on a fresh one-slot cache; memoised per setting."""
    from generate.base import SamplerRNG, generate

    key = ("single", id(model), prompt.numel(), None if seeds is None else tuple(seeds), tuple(sorted(kw.items())))
    if key not in _CACHE:
        outs = {}
        for s in ([None] if seeds is None else sorted(set(seeds))):
            _reset(model)
            rng = None if s is None else SamplerRNG(DEV, seed=s)
            outs[s] = generate(model, prompt, prompt.numel() + NEW, rng=rng, **kw).cpu()
        _CACHE[key] = outs
    return _CACHE[key]


@pytest.mark.parametrize("mode,groups", MODELS)
@pytest.mark.parametrize("share", [True, False])
def test_greedy_samples_all_equal_generate(mode, groups, share):
    from generate.base import generate_samples

    model = _model(mode, groups)
    for T in PROMPT_LENS:
        prompt = _prompt(model.config.vocab_size, T)
        one = _single(model, prompt, temperature=0.0)[None]
        _reset(model)
        outs = generate_samples(model, prompt, NEW, 3, temperature=0.0, share=share)
        assert len(outs) == 3
        for y in outs:
            assert torch.equal(y.cpu(), one)
    _reset(model)


@pytest.mark.parametrize("mode,groups", MODELS)
@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_sampled_samples_equal_generate_per_seed(mode, groups, share, use_graph):
    from generate.base import generate_samples

    model = _model(mode, groups)
    for T in PROMPT_LENS:
        prompt = _prompt(model.config.vocab_size, T)
        ones = _single(model, prompt, SEEDS, temperature=0.8, top_k=200)
        _reset(model)
        outs = generate_samples(model, prompt, NEW, 4, temperature=0.8, top_k=200, seeds=SEEDS, share=share,
                                use_graph=use_graph)
        for y, s in zip(outs, SEEDS):
            assert y.numel() == T + NEW and torch.equal(y.cpu(), ones[s]), (T, s)
        assert torch.equal(outs[0], outs[3]) and not torch.equal(outs[0], outs[1])
    _reset(model)


@pytest.mark.parametrize("share", [True, False])
def test_nucleus_samples_equal_generate_per_seed(share):
    from generate.base import generate_samples

    model = _model("int4-g128", 8)
    prompt = _prompt(model.config.vocab_size, 33)
    ones = _single(model, prompt, SEEDS[:3], temperature=0.8, top_k=200, top_p=0.9)
    _reset(model)
    outs = generate_samples(model, prompt, NEW, 3, temperature=0.8, top_k=200, top_p=0.9, seeds=SEEDS[:3], share=share)
    for y, s in zip(outs, SEEDS):
        assert torch.equal(y.cpu(), ones[s]), s
    _reset(model)


@pytest.mark.parametrize("share", [True, False])
def test_six_samples_run_two_waves_behind_one_prefix(share):
    from generate.base import generate_samples

    model = _model("int4-g128", 4)
    prompt = _prompt(model.config.vocab_size, 33)
    seeds = [5, 6, 7, 8, 9, 10]
    ones = _single(model, prompt, seeds, temperature=0.8, top_k=200)
    _reset(model)
    outs = generate_samples(model, prompt, NEW, 6, temperature=0.8, top_k=200, seeds=seeds, share=share)
    assert len(outs) == 6
    for y, s in zip(outs, seeds):
        assert torch.equal(y.cpu(), ones[s]), s
    # five samples: the last wave holds one
    outs = generate_samples(model, prompt, NEW, 5, temperature=0.8, top_k=200, seeds=seeds[:5], share=share)
    for y, s in zip(outs, seeds):
        assert torch.equal(y.cpu(), ones[s]), s
    _reset(model)


@pytest.mark.parametrize("share", [True, False])
def test_eos_truncates_as_generate_does(share):
    from generate.base import SamplerRNG, generate, generate_samples

    model = _model("int4-g128", 8)
    T = 33
    prompt = _prompt(model.config.vocab_size, T)
    ones = _single(model, prompt, SEEDS, temperature=0.8, top_k=200)
    eos = int(ones[SEEDS[1]][T + 1 + 9])  # from sample 1's own decoded tokens (the prefill's token is never tested)
    cut = {}
    for s in set(SEEDS):
        _reset(model)
        cut[s] = generate(model, prompt, T + NEW, temperature=0.8, top_k=200, eos_id=eos,
                          rng=SamplerRNG(DEV, seed=s)).cpu()
    assert cut[SEEDS[1]].numel() < T + NEW and int(cut[SEEDS[1]][-1]) == eos
    _reset(model)
    outs = generate_samples(model, prompt, NEW, 4, temperature=0.8, top_k=200, seeds=SEEDS, eos_id=eos, share=share)
    for y, s in zip(outs, SEEDS):
        assert torch.equal(y.cpu(), cut[s]), s
    _reset(model)


def test_fp8_cache_takes_the_copy_route():
    from generate.base import generate_samples

    model = _model("int4-g128", 8, kv_cache="fp8")
    prompt = _prompt(model.config.vocab_size, 33)
    ones = _single(model, prompt, SEEDS, temperature=0.8, top_k=200)
    _reset(model)
    with pytest.raises(NotImplementedError, match="bf16 KV cache"):
        generate_samples(model, prompt, NEW, 4, temperature=0.8, top_k=200, seeds=SEEDS, share=True)
    for share in (False, "auto"):
        _reset(model)
        outs = generate_samples(model, prompt, NEW, 4, temperature=0.8, top_k=200, seeds=SEEDS, share=share)
        assert model.transformer.h[0].attn.kv_cache.fp8
        for y, s in zip(outs, SEEDS):
            assert torch.equal(y.cpu(), ones[s]), (share, s)
    # the model step refuses the same, before any launch
    model.set_kv_cache(batch_size=2, device=torch.device(DEV), dtype=torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="fp8"):
        model(torch.zeros(2, 1, dtype=torch.int32, device=DEV), torch.tensor([33], device=DEV),
              shared_prefix=torch.tensor([33], device=DEV))
    _reset(model)


def test_head_size_64_takes_the_copy_route():
    from generate.base import generate_samples

    model = _model("int4-g128", 8, n_embd=512)
    assert model.config.head_size == 64
    prompt = _prompt(model.config.vocab_size, 33)
    ones = _single(model, prompt, SEEDS, temperature=0.8, top_k=200)
    _reset(model)
    with pytest.raises(NotImplementedError, match="geometry"):
        generate_samples(model, prompt, NEW, 4, temperature=0.8, top_k=200, seeds=SEEDS, share=True)
    for share in (False, "auto"):
        _reset(model)
        outs = generate_samples(model, prompt, NEW, 4, temperature=0.8, top_k=200, seeds=SEEDS, share=share)
        for y, s in zip(outs, SEEDS):
            assert torch.equal(y.cpu(), ones[s]), (share, s)
    model.set_kv_cache(batch_size=2, device=torch.device(DEV))
    with pytest.raises(NotImplementedError, match="head_size"):
        model(torch.zeros(2, 1, dtype=torch.int32, device=DEV), torch.tensor([33], device=DEV),
              shared_prefix=torch.tensor([33], device=DEV))
    _reset(model)


def test_shared_step_leaves_the_other_slots_prefix_rows_alone():
    """The samples' slots never receive the prompt under share=True: rows [0, T) of slots 1.. stay as they were."""
    from generate.base import generate_samples

    model = _model("int4-g128", 8)
    T = 33
    prompt = _prompt(model.config.vocab_size, T)
    model.set_kv_cache(batch_size=4, device=torch.device(DEV))
    for blk in model.transformer.h:
        for t in (blk.attn.kv_cache.k, blk.attn.kv_cache.v):
            t[1:, :, :T].view(torch.int16).fill_(0x7FC0)  # bf16 NaN: a read would show in the tokens
    outs = generate_samples(model, prompt, NEW, 4, temperature=0.8, top_k=200, seeds=SEEDS, share=True)
    ones = _single(model, prompt, SEEDS, temperature=0.8, top_k=200)
    for y, s in zip(outs, SEEDS):
        assert torch.equal(y.cpu(), ones[s]), s
    _reset(model)


def test_share_prompt_flag_prints_the_same_samples(monkeypatch, capsys):
    from generate import base
    from lit_gpt import Config

    cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=8,
                           intermediate_size=2816)
    monkeypatch.setattr(base.Config, "from_name", classmethod(lambda cls, name, **kw: cfg))
    kw = dict(num_samples=3, batch_size=2, max_new_tokens=12, synthetic="Llama-2-7b-hf", quantize="int4-g128",
              prompt_len=16)
    base.main(**kw)
    plain = capsys.readouterr().out
    base.main(share_prompt=True, **kw)
    shared = capsys.readouterr().out
    assert plain.count("[") == 3 and shared == plain
    lines = plain.strip().splitlines()
    assert lines[0] != lines[1]  # (sampled at the default temperature: the seeds differ)
