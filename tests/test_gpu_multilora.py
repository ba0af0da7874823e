"""Several LoRA adapters in one batched decode step on the MI355X: ``lga_lora_gemv_rows`` against the one-row kernel it
shares its body with, and ``lit_gpt.lora.attach_many`` models through ``generate`` / ``generate_batch`` /
``generate_continuous``.

The promise under test is the batched decode's, extended to adapters: batching never changes a sequence's result.
Every comparison is ``torch.equal``: a row of the rows launch against ``ops.lora_gemv`` on that row with that adapter's
views, a sequence of a batch against ``generate`` alone under ``model.lora_adapters.select(i)``, and that against a
model carrying adapter i alone (``lora.attach``).
"""

import types

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"

# ------------------------------------------------------------------------------------------------ kernel
SHAPES = [(1536, 1024, 8, 2), (1004, 264, 16, 3), (4096, 2816, 64, 1)]  # (N, K, r, segments)
N_ADAPTERS = 3
IDS = [2, -1, 0, 2, 1, 3, -7, 0]  # 3 and -7: out of range, they pass through like -1

_KERNEL = {}


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def _operands(N, K, r, segs):
    """Seeded operands for 8 rows, on the device: x (8, K), norm weight, stacked A (3, R, K) and B (3, N, r), row_off
    (segs > 1: the rows dealt to the segments in blocks of 5, every 7th block without adapter — the qkv layout's -1
    rows), base and residual (8, N)."""
    key = (N, K, r, segs)
    if key not in _KERNEL:
        _KERNEL.clear()
        g = torch.Generator().manual_seed(N * 31 + K * 7 + r * 3 + segs)
        rnd = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(torch.bfloat16).to(DEV)  # noqa: E731
        block = torch.arange(N) // 5
        off = None if segs == 1 else torch.where(block % 7 == 6, -1, (block % segs) * r).to(torch.int32).to(DEV)
        _KERNEL[key] = dict(x=rnd(8, K), nw=(1.0 + torch.randn(K, generator=g) * 0.2).to(torch.bfloat16).to(DEV),
                            A=rnd(N_ADAPTERS, r * segs, K, std=K ** -0.5), B=rnd(N_ADAPTERS, N, r, std=0.05), off=off,
                            base=rnd(8, N), res=rnd(8, N), scaling=16.0 / r)
    return _KERNEL[key]


def _row_reference(ops, c, m, a, x, norm, res):
    """Row m as the contract states it: the one-row launch with adapter a's views, or the pass-through."""
    if 0 <= a < N_ADAPTERS:
        return ops.lora_gemv(x[m], c["A"][a], c["B"][a], c["off"], c["scaling"], base=c["base"][m],
                             residual=c["res"][m] if res else None, **norm)
    return ops.add(c["base"][m], c["res"][m]) if res else c["base"][m]


@pytest.mark.parametrize("M", [1, 2, 4, 8])
@pytest.mark.parametrize("N,K,r,segs", SHAPES)
def test_rows_launch_has_the_one_row_launch_bits_per_row(ops, N, K, r, segs, M):
    c = _operands(N, K, r, segs)
    ids = torch.tensor(IDS[:M], dtype=torch.int32, device=DEV)
    x, base = c["x"][:M].contiguous(), c["base"][:M].contiguous()
    for with_norm in (True, False):
        norm = dict(norm_weight=c["nw"], eps=1e-5) if with_norm else {}
        for with_res in (True, False):
            res = c["res"][:M].contiguous() if with_res else None
            y = ops.lora_gemv_rows(x, c["A"], c["B"], c["off"], ids, c["scaling"], base=base, residual=res, **norm)
            assert y.shape == (M, N) and y.data_ptr() != base.data_ptr()
            for m, a in enumerate(IDS[:M]):
                assert torch.equal(y[m], _row_reference(ops, c, m, a, x, norm, with_res)), (with_norm, with_res, m, a)
            # out aliasing base: the same bits, in place
            alias = base.clone()
            assert ops.lora_gemv_rows(x, c["A"], c["B"], c["off"], ids, c["scaling"], base=alias, residual=res,
                                      out=alias, **norm) is alias
            assert torch.equal(alias, y)
            if M >= 2:
                # another row's x and id changed: every other row keeps its bits, the changed row follows its new id
                for victim in {0, M - 1}:
                    x2, ids2 = x.clone(), ids.clone()
                    x2[victim] = c["x"][(victim + 3) % 8]
                    new_id = (IDS[victim] + 1) % N_ADAPTERS if 0 <= IDS[victim] < N_ADAPTERS else 1
                    ids2[victim] = new_id
                    y2 = ops.lora_gemv_rows(x2, c["A"], c["B"], c["off"], ids2, c["scaling"], base=base, residual=res,
                                            **norm)
                    keep = [m for m in range(M) if m != victim]
                    assert torch.equal(y2[keep], y[keep]), (with_norm, with_res, victim)
                    assert torch.equal(y2[victim], _row_reference(ops, c, victim, new_id, x2, norm, with_res))
    # the adapters differ: a wrong choice could not pass
    for m, a in enumerate(IDS[:M]):
        if 0 <= a < N_ADAPTERS:
            other = _row_reference(ops, c, m, (a + 1) % N_ADAPTERS, x, {}, False)
            assert not torch.equal(other, _row_reference(ops, c, m, a, x, {}, False))


def test_pass_through_rows_read_no_adapter_and_equal_base(ops):
    """Rows without an adapter equal base (+ residual) even when A and B hold NaN everywhere."""
    N, K, r, segs = SHAPES[0]
    c = _operands(N, K, r, segs)
    nan_A, nan_B = torch.full_like(c["A"], float("nan")), torch.full_like(c["B"], float("nan"))
    ids = torch.tensor([-1, 3, -7, 2**31 - 1], dtype=torch.int32, device=DEV)
    x, base, res = c["x"][:4].contiguous(), c["base"][:4].contiguous(), c["res"][:4].contiguous()
    y = ops.lora_gemv_rows(x, nan_A, nan_B, c["off"], ids, c["scaling"], base=base, norm_weight=c["nw"])
    assert torch.equal(y, base)
    y = ops.lora_gemv_rows(x, nan_A, nan_B, c["off"], ids, c["scaling"], base=base, residual=res)
    assert torch.equal(y, ops.add(base, res))


def test_a_captured_launch_follows_the_ids_on_the_device(ops):
    N, K, r, segs = SHAPES[0]
    c = _operands(N, K, r, segs)
    M = 4
    x, base, res = c["x"][:M].contiguous(), c["base"][:M].contiguous(), c["res"][:M].contiguous()
    ids = torch.tensor(IDS[:M], dtype=torch.int32, device=DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    kw = dict(base=base, residual=res, norm_weight=c["nw"], eps=1e-5)
    ops.lora_gemv_rows(x, c["A"], c["B"], c["off"], ids, c["scaling"], out=out, **kw)
    first = out.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.lora_gemv_rows(x, c["A"], c["B"], c["off"], ids, c["scaling"], out=out, **kw)
    new = [1, 0, -1, 0]
    assert all(a != b for a, b in zip(new, IDS[:M]))
    ids.copy_(torch.tensor(new, dtype=torch.int32))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = ops.lora_gemv_rows(x, c["A"], c["B"], c["off"], torch.tensor(new, dtype=torch.int32, device=DEV),
                              c["scaling"], **kw)
    assert torch.equal(out, want)
    assert all(not torch.equal(out[m], first[m]) for m in range(M))


# ------------------------------------------------------------------------------------------------ model
S_MAX = 96
LENS = (5, 16, 33, 9, 21, 3, 12)
BUDGETS = (30, 24, 20, 28, 18, 34, 26)  # new tokens per prompt, as tests/test_gpu_continuous.py
IDS7 = [0, 1, None, 2, 1, 0, 2]  # the adapter of each of the 7 prompts
SEEDS = (11, 12, 13)  # random_adapter seeds of the set's three adapters
# lora_B's standard deviation. The precondition (_reference) needs the three adapters and the base to part ways on
# every prompt; fixed here, starting from the 0.05 of tests/lora_spec.py, never searched at run time
B_STD = 0.05
LORA = {"q+v": dict(r=8, alpha=16, to_query=True, to_value=True),
        "all": dict(r=16, alpha=16, to_query=True, to_key=True, to_value=True, to_projection=True, to_mlp=True,
                    to_head=True)}
# (mode, n_query_groups, adapter config): both formats, both groupings and both configs twice each
COMBOS = [("int4-g128", 8, "q+v"), ("nf4", 8, "all"), ("int4-g128", 4, "all"), ("nf4", 4, "q+v")]

_CACHE = {}


def _config(groups, targets):
    from lit_gpt import lora

    return lora.Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=groups,
                                 intermediate_size=2816, **LORA[targets])


def _states(cfg):
    from lit_gpt import lora

    return [lora.random_adapter(cfg, seed=s, b_std=B_STD) for s in SEEDS]


def _base_model(mode, groups, targets, kv_cache="bf16"):
    from generate.base import build_model

    return build_model(_config(groups, targets), quantize=mode, device=torch.device(DEV), max_seq_length=S_MAX,
                       kv_cache=kv_cache)


def _multi(mode, groups, targets, kv_cache="bf16"):
    """The ``attach_many`` model of a combination (same seeded base weights on every build)."""
    from lit_gpt import lora

    key = ("multi", mode, groups, targets, kv_cache)
    if key not in _CACHE:
        model = _base_model(mode, groups, targets, kv_cache)
        lora.attach_many(model, _states(model.config), model.config)
        _CACHE[key] = model
    return _CACHE[key]


def _cache(model, B):
    kv = model.transformer.h[0].attn.kv_cache
    model.set_kv_cache(batch_size=B, device=torch.device(DEV), dtype=kv.cache_dtype)


def _single(model, prompt, budget, adapter, **kw):
    """``generate`` alone on a one-sequence cache, under ``select(adapter)`` where the model carries a set."""
    from generate.base import generate

    _cache(model, 1)
    aset = getattr(model, "lora_adapters", None)
    if aset is not None:
        aset.select(adapter)
    try:
        return generate(model, prompt, prompt.numel() + budget, **kw).cpu()
    finally:
        if aset is not None:
            aset.select(None)


def _pick_eos(free, prompts):
    """As tests/test_gpu_continuous.py: a token of the free-running single streams that ends at least two sequences at
    different decode steps and leaves at least one to its budget."""
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


def _reference(mode, groups, targets, kv_cache="bf16"):
    """Per combination, once: the 7 prompts, the eos, and what ``generate`` returns for every prompt alone under its
    adapter of IDS7, free-running and under the eos. Random prompts give streams with no token in common, so two pairs
    of prompts walk one stream each under one adapter: prompt 0 (5 tokens) is prompt 5 (3 tokens) plus the first two
    tokens of its greedy continuation under adapter 0, prompt 6 (12) is prompt 3 (9) plus three under adapter 2.
    Asserts the PRECONDITION on the single-adapter path alone: for every prompt, the continuations under adapters 0, 1,
    2 and under none are four pairwise different streams, so a wrong adapter choice anywhere cannot pass."""
    key = ("ref", mode, groups, targets, kv_cache)
    if key not in _CACHE:
        model = _multi(mode, groups, targets, kv_cache)
        prompts = [torch.from_numpy(synth.token_ids(T, model.config.vocab_size, seed=20 + T)).to(DEV) for T in LENS]
        prompts[0] = _single(model, prompts[5], LENS[0] - LENS[5], 0, temperature=0.0)[:LENS[0]].to(DEV)
        prompts[6] = _single(model, prompts[3], LENS[6] - LENS[3], 2, temperature=0.0)[:LENS[6]].to(DEV)
        assert IDS7[0] == IDS7[5] == 0 and IDS7[3] == IDS7[6] == 2
        free = []
        for i, (p, m) in enumerate(zip(prompts, BUDGETS)):
            streams = {a: _single(model, p, m, a, temperature=0.0) for a in (0, 1, 2, None)}
            assert len({tuple(s.tolist()) for s in streams.values()}) == 4, \
                f"prompt {i}: the adapters do not part ways (B_STD {B_STD})"
            free.append(streams[IDS7[i]])
        eos = _pick_eos(free, prompts)
        single = [_single(model, p, m, a, temperature=0.0, eos_id=eos) for p, m, a in zip(prompts, BUDGETS, IDS7)]
        by_eos = [i for i, (o, p, m) in enumerate(zip(single, prompts, BUDGETS)) if o.numel() < p.numel() + m]
        ends = {single[i].numel() - prompts[i].numel() for i in by_eos}
        assert len(by_eos) >= 2 and len(ends) >= 2 and len(by_eos) < len(prompts), (eos, by_eos, ends)
        _CACHE[key] = (prompts, eos, free, single)
    return _CACHE[key]


def _detach(model):
    """Put the base Linears back (test only: one second model serves every single-adapter comparison)."""
    from lit_gpt import lora

    for parent in list(model.modules()):
        for name, m in list(parent.named_children()):
            if isinstance(m, lora.LoraLinear):
                setattr(parent, name, m.base)


@pytest.mark.parametrize("mode,groups,targets", COMBOS)
def test_select_equals_the_single_adapter_model_and_none_the_plain_model(mode, groups, targets):
    from lit_gpt import lora

    multi = _multi(mode, groups, targets)
    prompts, _, free, _ = _reference(mode, groups, targets)
    n_targets = {"q+v": 1, "all": 5}[targets] * multi.config.n_layer + (targets == "all")
    assert sum(isinstance(m, lora.MultiLoraLinear) for m in multi.modules()) == n_targets
    other = _base_model(mode, groups, targets)  # the same seeded base weights
    states = _states(other.config)
    checked = set()
    for i in (1, 2, 4, 6):  # one prompt per id of IDS7: adapters 1, None, 1, 2 ...
        p, m, a = prompts[i], BUDGETS[i], IDS7[i]
        if a is not None:
            lora.attach(other, states[a], other.config)
        assert torch.equal(_single(other, p, m, None, temperature=0.0), free[i]), (i, a)
        _detach(other)
        checked.add(a)
    p, m = prompts[0], BUDGETS[0]  # ... and adapter 0
    lora.attach(other, states[0], other.config)
    assert torch.equal(_single(other, p, m, None, temperature=0.0), free[0])
    _detach(other)
    assert checked | {0} == {0, 1, 2, None}
    # sampling goes the same way: a seeded run under select(2) against the single-adapter model
    from generate.base import SamplerRNG

    kw = dict(temperature=0.8, top_k=50)
    got = _single(multi, prompts[3], 12, 2, rng=SamplerRNG(DEV, seed=5), **kw)
    lora.attach(other, states[2], other.config)
    assert torch.equal(_single(other, prompts[3], 12, None, rng=SamplerRNG(DEV, seed=5), **kw), got)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("mode,groups,targets", COMBOS)
def test_generate_batch_with_an_adapter_per_sequence_equals_the_single_runs(mode, groups, targets, use_graph):
    from generate.base import generate_batch

    model = _multi(mode, groups, targets)
    prompts, _, free, _ = _reference(mode, groups, targets)
    pick, ids = [0, 2, 3, 5], [0, None, 2, 0]  # lengths 5, 33, 9, 3
    assert [IDS7[i] for i in pick] == ids
    new = 18
    outs = generate_batch(model, [prompts[i] for i in pick], new, temperature=0.0, adapters=ids, use_graph=use_graph)
    for b, i in enumerate(pick):
        assert torch.equal(outs[b].cpu(), free[i][:LENS[i] + new]), (b, i)
    assert model.lora_adapters.rows[:4].tolist() == [0, -1, 2, 0] and model.lora_adapters.selected is None
    _cache(model, 1)


@pytest.mark.parametrize("chunk,use_graph", [(8, True), (1, True), (8, False), (1, False)],
                         ids=["graph-chunk8", "graph-chunk1", "eager-chunk8", "eager-chunk1"])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("mode,groups,targets", COMBOS)
def test_generate_continuous_greedy_with_adapters_equals_the_single_runs(mode, groups, targets, B, chunk, use_graph):
    from generate.base import generate_continuous

    model = _multi(mode, groups, targets)
    prompts, eos, _, single = _reference(mode, groups, targets)
    outs = generate_continuous(model, prompts, list(BUDGETS), batch_size=B, temperature=0.0, eos_id=eos,
                               use_graph=use_graph, chunk=chunk, adapters=IDS7)
    for i in range(len(prompts)):
        assert torch.equal(outs[i].cpu(), single[i]), (i, IDS7[i], outs[i].tolist(), single[i].tolist())
    assert model.lora_adapters.selected is None
    _cache(model, 1)


@pytest.mark.parametrize("chunk", [8, 1])
@pytest.mark.parametrize("mode,groups,targets", [COMBOS[1], COMBOS[3]])
def test_generate_continuous_sampling_with_adapters_equals_the_single_path_per_seed(mode, groups, targets, chunk):
    from generate.base import SamplerRNG, generate_continuous

    model = _multi(mode, groups, targets)
    prompts = _reference(mode, groups, targets)[0]
    seeds = [1234, 99, 7, 2**40 + 5, 31337, 1, 77]
    key = ("sampled", mode, groups, targets)
    if key not in _CACHE:
        _CACHE[key] = [_single(model, p, m, a, temperature=0.8, top_k=50, rng=SamplerRNG(DEV, seed=s))
                       for p, m, a, s in zip(prompts, BUDGETS, IDS7, seeds)]
    ref = _CACHE[key]
    outs = generate_continuous(model, prompts, list(BUDGETS), batch_size=3, temperature=0.8, top_k=50, seeds=seeds,
                               chunk=chunk, adapters=IDS7)
    for i in range(len(prompts)):
        assert torch.equal(outs[i].cpu(), ref[i]), (i, IDS7[i], outs[i].tolist(), ref[i].tolist())
    _cache(model, 1)


def test_generate_continuous_fp8_cache_with_adapters_equals_the_single_runs():
    from generate.base import generate_continuous

    mode, groups, targets = COMBOS[2]
    model = _multi(mode, groups, targets, "fp8")
    assert model.transformer.h[0].attn.kv_cache.fp8
    prompts, eos, _, single = _reference(mode, groups, targets, "fp8")
    outs = generate_continuous(model, prompts, list(BUDGETS), batch_size=3, temperature=0.0, eos_id=eos,
                               adapters=IDS7)
    assert model.transformer.h[0].attn.kv_cache.fp8
    for i in range(len(prompts)):
        assert torch.equal(outs[i].cpu(), single[i]), (i, IDS7[i])
    _cache(model, 1)


class Recorder:
    """Stands in for ``ops._lib`` (as tests/test_gpu_lora.py): logs the name of every ``lga_*`` call."""

    def __init__(self, ops):
        self.lib, self.calls = ops.load_library(), []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("lga_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


@pytest.mark.parametrize("mode,groups,targets", COMBOS[:2])
@torch.inference_mode()
def test_one_rows_launch_per_adapted_linear_per_batched_step(monkeypatch, mode, groups, targets):
    from lit_gpt import lora, ops

    model = _multi(mode, groups, targets)
    prompts = _reference(mode, groups, targets)[0][:3]
    n_adapted = sum(isinstance(m, lora.MultiLoraLinear) for m in model.modules())
    _cache(model, 3)
    for b, p in enumerate(prompts):
        model.lora_adapters.select(IDS7[b])
        model(p.view(1, -1), torch.arange(p.numel(), device=DEV), last_token_only=True, kv_slot=b)
        model.lora_adapters.assign(b, IDS7[b])
    model.lora_adapters.select(None)
    rec = Recorder(ops)
    monkeypatch.setattr(ops, "_lib", rec)
    idx = torch.tensor([[1], [2], [3]], dtype=torch.int32, device=DEV)
    model(idx, torch.tensor([p.numel() for p in prompts], device=DEV))
    step = rec.calls
    assert step.count("lga_lora_gemv_rows") == n_adapted and "lga_lora_gemv" not in step
    assert "lga_lora_down" not in step and "lga_lora_up" not in step
    for i, name in enumerate(step):  # two launches per adapted Linear: the base's rows GEMV, then the adapters'
        if name == "lga_lora_gemv_rows":
            assert step[i - 1] == "lga_q4_gemv_rows", step[max(0, i - 2):i + 1]
    monkeypatch.undo()
    _cache(model, 1)


def test_batched_step_refusals():
    from generate.base import generate_batch
    from lit_gpt import lora

    mode, groups, targets = COMBOS[0]
    model = _base_model(mode, groups, targets)
    prompts = [torch.from_numpy(synth.token_ids(T, model.config.vocab_size, seed=20 + T)).to(DEV) for T in (4, 6)]
    with pytest.raises(ValueError, match="no adapter set"):
        generate_batch(model, prompts, 4, temperature=0.0, adapters=[0, None])
    lora.attach(model, _states(model.config)[0], model.config)  # a single-adapter model stays refused for batches
    with pytest.raises(NotImplementedError, match="batch size > 1"):
        generate_batch(model, prompts, 4, temperature=0.0)
    multi = _multi(mode, groups, targets)  # ... and so does the speculative verify window for either kind
    _cache(multi, 1)
    with pytest.raises(NotImplementedError, match="speculative verify window"):
        multi.decode_window(torch.tensor([1, 2], dtype=torch.int32, device=DEV), torch.tensor([0], device=DEV))


def test_multi_adapter_cli_serves_a_prompts_file_in_file_order(monkeypatch, tmp_path, capsys):
    """generate/lora.py --lora_paths ... --prompts_file ... --synthetic: the adapter files are missing, so adapter i is
    ``random_adapter(config, seed=1234 + i)``; every printed completion is ``generate`` under that line's adapter."""
    import generate.lora as gl
    from generate.base import build_model
    from lit_gpt import lora

    cfg = _config(8, "q+v")  # generate/lora.py's module-level lora_* defaults are this config's: r 8, alpha 16, q + v
    assert gl._lora_kwargs()["r"] == cfg.r and gl._lora_kwargs()["alpha"] == cfg.alpha
    monkeypatch.setattr(gl.lora, "Config", types.SimpleNamespace(from_name=lambda name, **kw: cfg))
    lens, ids, new = [5, 12, 3, 9], [1, None, 0, 1], 10
    f = tmp_path / "requests.txt"
    f.write_text("".join(f"{'-' if a is None else a}\t{n}\n" for a, n in zip(ids, lens)))
    gl._cli(["--synthetic", "Llama-2-7b-hf", "--checkpoint_dir", str(tmp_path), "--quantize", "int4-g128",
             "--lora_paths", str(tmp_path / "a0.pth"), str(tmp_path / "a1.pth"), "--prompts_file", str(f),
             "--batch_size", "3", "--max_new_tokens", str(new), "--temperature", "0"])
    cap = capsys.readouterr()
    printed = [ln for ln in cap.out.splitlines() if ln.startswith("[")]
    assert len(printed) == len(lens) and "tokens/sec over 4 requests" in cap.err
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g, dtype=torch.int32).to(DEV) for n in lens]
    model = build_model(cfg, quantize="int4-g128", device=torch.device(DEV), max_seq_length=max(lens) + new)
    lora.attach_many(model, [lora.random_adapter(cfg, seed=1234 + i) for i in range(2)], cfg)
    for line, p, a in zip(printed, prompts, ids):
        assert line == str(_single(model, p, new, a, temperature=0.0).tolist()), a
