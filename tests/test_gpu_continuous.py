"""Continuous batching on the MI355X: the batched model step on the one-launch batch attention, ``SlotDecodeGraph``
and ``generate_continuous``.

The promise under test is the batched decode's: batching never changes a sequence's result. Whatever slot a prompt
lands in, whenever it enters, whoever its neighbours are and however the steps are chunked, ``result[i]`` is
``torch.equal`` to what ``generate`` returns for that prompt alone.
"""

import types

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
S_MAX = 96
LENS = (5, 16, 33, 9, 21, 3, 12)
BUDGETS = (30, 24, 20, 28, 18, 34, 26)  # new tokens per prompt; 33 + 20 - 1 = 52 <= S_MAX
MODELS = [("int4-g128", 8), ("nf4", 8), ("int4-g128", 4)]  # (mode, n_query_groups), as tests/test_gpu_batch.py

_CACHE = {}


def _model(mode, groups, kv_cache="bf16"):
    from generate.base import build_model
    from lit_gpt import Config

    key = ("model", mode, groups, kv_cache)
    if key not in _CACHE:
        cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=groups,
                               intermediate_size=2816)
        _CACHE[key] = build_model(cfg, quantize=mode, device=torch.device(DEV), max_seq_length=S_MAX,
                                  kv_cache=kv_cache)
    return _CACHE[key]


def _prompts(vocab, lens=LENS):
    return [torch.from_numpy(synth.token_ids(T, vocab, seed=20 + T)).to(DEV) for T in lens]


def _cache(model, B):
    kv = model.transformer.h[0].attn.kv_cache
    model.set_kv_cache(batch_size=B, device=torch.device(DEV), dtype=kv.cache_dtype)


def _single_runs(model, prompts, budgets, **kw):
    from generate.base import generate

    outs = []
    for p, m in zip(prompts, budgets):
        _cache(model, 1)
        outs.append(generate(model, p, p.numel() + m, **kw).cpu())
    return outs


def _pick_eos(free, prompts):
    """A token from the free-running single streams that ends at least two sequences at different decode steps and
    leaves at least one to its budget. (The prefill's token is never tested against eos, as in ``generate``.)"""
    decoded = [o[p.numel() + 1:].tolist() for o, p in zip(free, prompts)]
    best = None
    for tok in sorted({t for d in decoded for t in d}):
        first = [d.index(tok) if tok in d else None for d in decoded]
        hits = {f for f in first if f is not None}
        n_hit = sum(f is not None for f in first)
        if len(hits) >= 2 and n_hit < len(decoded):
            score = (min(n_hit, len(decoded) - n_hit), len(hits))
            if best is None or score > best[0]:
                best = (score, tok)
    assert best is not None, f"no token of the single runs serves as an eos: {decoded}"
    return best[1]


def _greedy_reference(mode, groups, kv_cache="bf16"):
    """Per model, once: the prompts, the eos and what ``generate`` returns for every prompt alone under it. Random
    prompts give streams with no token in common, so prompts 3 and 6 (9 and 12 tokens) are prompt 0 (5 tokens) plus
    the first 4 and 7 tokens of its own greedy continuation: the three sequences walk one stream at different steps,
    and a token of it ends them at different steps."""
    from generate.base import generate

    key = ("ref", mode, groups, kv_cache)
    if key not in _CACHE:
        model = _model(mode, groups, kv_cache)
        prompts = _prompts(model.config.vocab_size)
        _cache(model, 1)
        walk = generate(model, prompts[0], LENS[6] + 1, temperature=0.0)
        prompts[3], prompts[6] = walk[:LENS[3]].clone(), walk[:LENS[6]].clone()
        free = _single_runs(model, prompts, BUDGETS, temperature=0.0)
        eos = _pick_eos(free, prompts)
        single = _single_runs(model, prompts, BUDGETS, temperature=0.0, eos_id=eos)
        by_eos = [i for i, (o, p, m) in enumerate(zip(single, prompts, BUDGETS)) if o.numel() < p.numel() + m]
        ends = {single[i].numel() - prompts[i].numel() for i in by_eos}
        # the precondition: at least two sequences end by eos at different steps, at least one by its budget
        assert len(by_eos) >= 2 and len(ends) >= 2 and len(by_eos) < len(prompts), (eos, by_eos, ends)
        for i in by_eos:
            assert int(single[i][-1]) == eos
        _CACHE[key] = (prompts, eos, single)
    return _CACHE[key]


def _spy_scheduler(monkeypatch):
    """Record the SlotScheduler that generate_continuous builds."""
    import lit_gpt.scheduler as sch

    made = []

    class Spy(sch.SlotScheduler):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(sch, "SlotScheduler", Spy)
    return made


@pytest.mark.parametrize("mode,groups", MODELS)
def test_batched_step_logits_batch_launch_equals_loop_and_single(monkeypatch, mode, groups):
    import lit_gpt.model as lm
    from lit_gpt import ops

    model = _model(mode, groups)
    prompts = _prompts(model.config.vocab_size, LENS[:3])
    with torch.inference_mode():
        single = []
        for p in prompts:
            _cache(model, 1)
            T = p.numel()
            pre = model(p.view(1, -1), torch.arange(T, device=DEV), last_token_only=True)
            tok = ops.argmax(pre.view(-1).contiguous()).to(torch.int32)
            single.append((tok, model(tok.view(1, 1), torch.tensor([T], device=DEV))))
        idx = torch.cat([s[0] for s in single]).view(-1, 1)
        pos = torch.tensor([p.numel() for p in prompts], device=DEV)
        logits = {}
        for on in (True, False):
            monkeypatch.setattr(lm, "batch_attention", on)
            _cache(model, len(prompts))
            for b, p in enumerate(prompts):
                model(p.view(1, -1), torch.arange(p.numel(), device=DEV), last_token_only=True, kv_slot=b)
            logits[on] = model(idx, pos).clone()
        assert torch.equal(logits[True], logits[False])
        for b in range(len(prompts)):
            assert torch.equal(logits[True][b], single[b][1][0]), b
        # idle rows: the active rows' logits do not move, the idle row's cache slot is not written
        _cache(model, len(prompts))
        for b, p in enumerate(prompts):
            model(p.view(1, -1), torch.arange(p.numel(), device=DEV), last_token_only=True, kv_slot=b)
        kv = model.transformer.h[0].attn.kv_cache
        before = kv.k[1].clone()
        active = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
        part = model(idx, pos, active=active)
        assert torch.equal(part[0], logits[True][0]) and torch.equal(part[2], logits[True][2])
        assert torch.equal(kv.k[1], before)
    _cache(model, 1)


@pytest.mark.parametrize("chunk,use_graph", [(8, True), (1, True), (8, False), (1, False)],
                         ids=["graph-chunk8", "graph-chunk1", "eager-chunk8", "eager-chunk1"])
@pytest.mark.parametrize("mode,groups", MODELS)
def test_generate_continuous_greedy_equals_generate(monkeypatch, mode, groups, chunk, use_graph):
    from generate.base import generate_continuous

    model = _model(mode, groups)
    prompts, eos, single = _greedy_reference(mode, groups)
    made = _spy_scheduler(monkeypatch)
    outs = generate_continuous(model, prompts, list(BUDGETS), batch_size=3, temperature=0.0, eos_id=eos,
                               use_graph=use_graph, chunk=chunk)
    assert len(outs) == len(prompts)
    for i in range(len(prompts)):
        assert torch.equal(outs[i].cpu(), single[i]), (i, outs[i].tolist(), single[i].tolist())
    assert len(made) == 1 and made[0].n_slots == 3
    assert any(len(s) >= 2 for s in made[0].served)  # some slot served at least two prompts
    _cache(model, 1)


def test_generate_continuous_fp8_cache_equals_generate():
    from generate.base import generate_continuous

    model = _model("int4-g128", 4, "fp8")
    assert model.transformer.h[0].attn.kv_cache.fp8
    prompts, eos, single = _greedy_reference("int4-g128", 4, "fp8")
    for chunk in (8, 1):
        outs = generate_continuous(model, prompts, list(BUDGETS), batch_size=3, temperature=0.0, eos_id=eos,
                                   chunk=chunk)
        assert model.transformer.h[0].attn.kv_cache.fp8  # the rebuilt cache kept its format
        for i in range(len(prompts)):
            assert torch.equal(outs[i].cpu(), single[i]), (chunk, i)
    _cache(model, 1)


@pytest.mark.parametrize("chunk", [8, 1])
def test_generate_continuous_sampling_equals_single_path_per_seed(chunk):
    from generate.base import SamplerRNG, generate, generate_continuous

    model = _model("nf4", 8)
    prompts = _prompts(model.config.vocab_size)
    seeds = [1234, 99, 7, 2**40 + 5, 31337, 1, 77]
    key = ("sampled", "nf4", 8)
    if key not in _CACHE:
        ref = []
        for p, m, s in zip(prompts, BUDGETS, seeds):
            _cache(model, 1)
            ref.append(generate(model, p, p.numel() + m, temperature=0.8, top_k=50, rng=SamplerRNG(DEV, seed=s)).cpu())
        _CACHE[key] = ref
    ref = _CACHE[key]
    outs = generate_continuous(model, prompts, list(BUDGETS), batch_size=3, temperature=0.8, top_k=50, seeds=seeds,
                               chunk=chunk)
    for i in range(len(prompts)):
        assert torch.equal(outs[i].cpu(), ref[i]), (i, outs[i].tolist(), ref[i].tolist())
    _cache(model, 1)


def test_generate_continuous_fewer_prompts_than_slots_and_int_budget():
    from generate.base import generate_continuous

    model = _model("int4-g128", 8)
    prompts = _prompts(model.config.vocab_size, LENS[:2])
    single = _single_runs(model, prompts, (12, 12), temperature=0.0)
    outs = generate_continuous(model, prompts, 12, batch_size=4, temperature=0.0)
    for i in range(2):
        assert torch.equal(outs[i].cpu(), single[i]), i
    one = generate_continuous(model, prompts[:1], 12, temperature=0.0)  # one prompt: one slot, the single path
    assert torch.equal(one[0].cpu(), single[0])
    _cache(model, 1)


def test_generate_batch_on_the_batch_launch_equals_generate(monkeypatch):
    import lit_gpt.model as lm
    from generate.base import generate_batch

    monkeypatch.setattr(lm, "batch_attention", True)
    model = _model("int4-g128", 4)
    prompts = _prompts(model.config.vocab_size, LENS[:3])
    single = _single_runs(model, prompts, (24,) * 3, temperature=0.0)
    outs = generate_batch(model, prompts, 24, temperature=0.0)
    for b in range(3):
        assert torch.equal(outs[b].cpu(), single[b]), b
    _cache(model, 1)


def test_continuous_refusals():
    from generate.base import MAX_BATCH, build_model, generate_continuous
    from lit_gpt import Config

    model = _model("int4-g128", 8)
    prompts = _prompts(model.config.vocab_size)
    with pytest.raises(NotImplementedError, match=f"at most {MAX_BATCH}"):
        generate_continuous(model, prompts, 4, batch_size=MAX_BATCH + 1, temperature=0.0)
    with pytest.raises(NotImplementedError, match=f"max_seq_length {S_MAX} needs to be >= {33 + 70 - 1}"):
        generate_continuous(model, prompts, 70, batch_size=3, temperature=0.0)
    with pytest.raises(ValueError, match="no prompts"):
        generate_continuous(model, [], 4)
    tiny = dict(n_layer=1, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512, vocab_size=1000,
                padding_multiple=64, block_size=64)
    m = build_model(Config.from_name("Llama-2-7b-hf", **tiny), quantize=None, device=torch.device(DEV),
                    max_seq_length=32)
    with pytest.raises(NotImplementedError, match="batch size > 1"):  # bf16 weights
        generate_continuous(m, _prompts(1000, (4, 5, 6)), 4, batch_size=2, temperature=0.0)


def test_prompts_file_cli_prints_completions_in_file_order(monkeypatch, tmp_path, capsys):
    import generate.base as gb

    cfg = gb.Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=8,
                              intermediate_size=2816)
    monkeypatch.setattr(gb, "Config", types.SimpleNamespace(from_name=lambda name: cfg))
    lens = [5, 12, 3, 9, 7]
    f = tmp_path / "prompts.txt"
    f.write_text("".join(f"{n}\n" for n in lens))
    new = 10
    gb._cli(["--synthetic", "Llama-2-7b-hf", "--quantize", "int4-g128", "--prompts_file", str(f), "--batch_size", "3",
             "--max_new_tokens", str(new), "--temperature", "0"])
    cap = capsys.readouterr()
    printed = [ln for ln in cap.out.splitlines() if ln.startswith("[")]
    assert len(printed) == len(lens)
    assert "tokens/sec" in cap.err and "5 prompts through 3 slots" in cap.err
    # the same ids as --prompt_len draws them, line after line from one generator; each completion is generate's
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g, dtype=torch.int32).to(DEV) for n in lens]
    model = gb.build_model(cfg, quantize="int4-g128", device=torch.device(DEV), max_seq_length=max(lens) + new)
    for line, p in zip(printed, prompts):
        model.set_kv_cache(batch_size=1, device=torch.device(DEV))
        assert line == str(gb.generate(model, p, p.numel() + new, temperature=0.0).tolist())
