"""Speculative decoding under top-k sampling on the MI355X: the window sampler + acceptance entry
(lga_spec_accept_sample), ``WindowDecodeGraph(temperature > 0)``, the coupled ``ModelDrafter`` and
``generate_speculative(temperature, top_k, rng)``.

The promise under test is the greedy one extended to sampling: speculation never changes the result. Row r of a window
is sampled by the one-row sampler's own code under draw number counter + r, a draft is accepted iff it equals that
sample, so ``generate_speculative`` returns ``generate``'s tokens for the same seed whatever the drafter proposes.
Every comparison here is ``==``: both sides are the same arithmetic.
"""

import pytest
import torch

from test_gpu_sample import _logits
from test_gpu_speculative import DEV, NEW, S, _fresh, _model, _prompt

pytestmark = pytest.mark.gpu

SEED = 1234
MS = (1, 2, 3, 5, 8)
TEMPS = (0.8, 1.7)
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def _rows(n):
    """8 rows built like tests/test_gpu_sample.py's: row 1 rounded (heavy ties), row 2 peaked (the radix fallback)."""
    if ("rows", n) not in _CACHE:
        kinds = {1: True, 2: "peaked"}
        _CACHE[("rows", n)] = torch.stack([_logits(n, 100 * n + r, kinds.get(r, False)) for r in range(8)]).to(DEV)
    return _CACHE[("rows", n)]


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _counter(c):
    return torch.tensor([c], dtype=torch.int64, device=DEV)


def _one_row_uniform(ops, logits, k, T, u):
    """The reference, explicit uniforms: the one-row sampler on each row with that row's uniform."""
    out = torch.zeros(logits.shape[0], dtype=torch.int64, device=DEV)
    for r in range(logits.shape[0]):
        ops.sample_topk(logits[r], k, T, uniform=u[r:r + 1], out_idx=out[r:r + 1])
    return out.tolist()


def _one_row_counter(ops, logits, k, T, c0, seed=SEED):
    """The reference, counter path: the one-row sampler on row r with its counter preset to c0 + r."""
    out = torch.zeros(logits.shape[0], dtype=torch.int64, device=DEV)
    for r in range(logits.shape[0]):
        ops.sample_topk(logits[r], k, T, seed=seed, counter=_counter(c0 + r), out_idx=out[r:r + 1])
    return out.tolist()


def _window_samples(ops, logits, k, T, **kw):
    """One window call -> (a, out[1:]). ``out`` lists t_r only up to the first wrong draft, so the callers pass a
    window made of the REFERENCE's tokens: the call then reports all M samples iff each equals the reference's."""
    M = logits.shape[0]
    out = ops.spec_accept_sample(logits, kw.pop("window"), k, T, **kw).tolist()
    return out[0], out[1:M + 1]


@pytest.mark.parametrize("n", [32000, 50304, 1000, 7])  # EPT 32 / 64 / 16; at n = 7 odd rows are not 4-B aligned
@pytest.mark.parametrize("k", [1, 200, 1024])
def test_window_samples_equal_the_one_row_sampler(ops, n, k):
    rows = _rows(n)
    u = torch.tensor([0.013, 0.37, 0.5, 0.93, 0.9999, 0.2, 0.66, 0.81], dtype=torch.float32, device=DEV)
    for T in TEMPS:
        ref_u = _one_row_uniform(ops, rows, k, T, u)
        ref_c = {c0: _one_row_counter(ops, rows, k, T, c0) for c0 in (0, 41)}
        for M in MS:
            logits = rows[:M]  # (a contiguous prefix: row r starts 2 n r bytes in)
            # (a) explicit uniforms: a window of the reference tokens is accepted whole iff every t_r is the
            # reference's, and then out lists all M of them
            a, t = _window_samples(ops, logits, k, T, window=_i32([5] + ref_u[:M - 1]), uniform=u[:M].contiguous())
            assert t == ref_u[:M] and a == M - 1, (T, M, t, ref_u[:M])
            # (b) the counter path from c0
            for c0, ref in ref_c.items():
                c = _counter(c0)
                a, t = _window_samples(ops, logits, k, T, window=_i32([5] + ref[:M - 1]), seed=SEED, counter=c)
                assert t == ref[:M] and a == M - 1, (T, M, c0, t, ref[:M])
                assert int(c) == c0 + M


@pytest.mark.parametrize("M", [1, 2, 5, 8])
def test_acceptance_and_bookkeeping(ops, M):
    n, k, T, c0, pos0 = 1000, 200, 0.8, 41, 17
    logits = _rows(n)[:M]
    before = logits.clone()
    t = _one_row_counter(ops, logits, k, T, c0)
    good = [7] + t[:M - 1]
    # draft i wrong -> a == i; a change of window[0] (the last emitted token, no draft) or none -> a == M - 1
    cases = [(M - 1, list(good)), (M - 1, [8] + good[1:])]
    for i in range(M - 1):
        w = list(good)
        w[1 + i] = (w[1 + i] + 1) % n
        cases.append((i, w))
    for want, w in cases:
        window = _i32(w)
        tok, pos, c = _i32([-5]), torch.tensor([pos0], dtype=torch.int64, device=DEV), _counter(c0)
        out = ops.spec_accept_sample(logits, window, k, T, seed=SEED, counter=c, token_inout=tok, pos_inout=pos)
        out = out.tolist()
        a = out[0]
        assert a == want, (w, out)
        assert out[1:a + 2] == t[:a + 1] and all(v == -1 for v in out[a + 2:]) and len(out) == M + 1
        assert int(tok) == t[a] and int(pos) == pos0 + a + 1 and int(c) == c0 + a + 1
        assert window.tolist() == w and torch.equal(logits, before)
    # the executor's aliasing: token_inout is window[0]
    window = _i32(good + [0] * (8 - M))
    c = _counter(c0)
    out = ops.spec_accept_sample(logits, window[:M], k, T, seed=SEED, counter=c, token_inout=window[:1]).tolist()
    assert out[0] == M - 1 and window.tolist() == [t[M - 1]] + good[1:] + [0] * (8 - M)
    if M == 1:  # a plain sampled step
        one = ops.sample_topk(logits[0], k, T, seed=SEED, counter=_counter(c0))
        assert out == [0, int(one)] and int(c) == c0 + 1
    # explicit uniforms leave a counter alone, as the one-row sampler does
    u = torch.full((M,), 0.4, dtype=torch.float32, device=DEV)
    c = _counter(c0)
    ops.spec_accept_sample(logits, _i32(good), k, T, uniform=u, counter=c)
    assert int(c) == c0


def test_counter_draws_follow_the_host_formula(ops):
    """Draw n of a seed is the draw under uniform = ops.sampler_uniform(seed, n), also past 2**32."""
    n, k, T, M = 32000, 200, 0.8, 3
    logits = _rows(n)[:M]
    wrong = _i32([0])  # a one-row window: no drafts, out = [0, t_0]
    seen = set()
    for seed, c0 in ((SEED, 0), (SEED, 41), (99, 2**32 + 5), (2**62 - 1, 2**40), (7, 2**33 - 1)):
        for r in range(M):  # row r of the window alone, at draw c0 + r: t_0 of a one-row window
            u = torch.tensor([ops.sampler_uniform(seed, c0 + r)], dtype=torch.float32, device=DEV)
            assert float(u) == ops.sampler_uniform(seed, c0 + r)
            by_u = ops.spec_accept_sample(logits[r:r + 1], wrong, k, T, uniform=u).tolist()[1]
            by_c = ops.spec_accept_sample(logits[r:r + 1], wrong, k, T, seed=seed,
                                          counter=_counter(c0 + r)).tolist()[1]
            one = int(ops.sample_topk(logits[r], k, T, uniform=u))
            assert by_u == by_c == one, (seed, c0, r)
            seen.add(by_c)
        # and as rows of one window: the reference tokens are accepted whole
        ref = _one_row_uniform(ops, logits, k, T, torch.tensor([ops.sampler_uniform(seed, c0 + r) for r in range(M)],
                                                                dtype=torch.float32, device=DEV))
        out = ops.spec_accept_sample(logits, _i32([0] + ref[:M - 1]), k, T, seed=seed, counter=_counter(c0)).tolist()
        assert out == [M - 1] + ref
    assert len(seen) > 3  # the draws differ


def test_graph_replay_equals_eager(ops):
    n, k, T, M, rounds = 1000, 200, 0.8, 4, 20
    logits = _rows(n)[:M]
    # the schedule: round j wants j % M drafts accepted. The eager pass builds each round's window from the row
    # samples at that round's counter (host formula + the one-row sampler) and records what the call leaves behind
    windows, eager = [], []
    tok, pos, c = _i32([9]), torch.tensor([30], dtype=torch.int64, device=DEV), _counter(1)
    window = torch.zeros(M, dtype=torch.int32, device=DEV)
    out = torch.zeros(M + 1, dtype=torch.int32, device=DEV)
    sampled = torch.zeros(8, dtype=torch.int32, device=DEV)
    count = 1
    for j in range(rounds):
        u = torch.tensor([ops.sampler_uniform(SEED, count + r) for r in range(M)], dtype=torch.float32, device=DEV)
        t = _one_row_uniform(ops, logits, k, T, u)
        w = [int(tok)] + t[:M - 1]
        want = j % M
        if want < M - 1:
            w[1 + want] = (w[1 + want] + 1) % n
        windows.append(w)
        window.copy_(_i32(w))
        ops.spec_accept_sample(logits, window, k, T, seed=SEED, counter=c, out=out, token_inout=tok, pos_inout=pos,
                               sampled=sampled)
        eager.append((out.tolist(), int(tok), int(pos), int(c)))
        assert eager[-1][0][0] == want
        count += want + 1
        assert int(c) == count
    # the captured call, replayed over the same windows from the same start
    tok.fill_(9)
    pos.fill_(30)
    c.fill_(1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spec_accept_sample(logits, window, k, T, seed=SEED, counter=c, out=out, token_inout=tok, pos_inout=pos,
                               sampled=sampled)
    replayed = []
    for w in windows:
        window.copy_(_i32(w))
        g.replay()
        replayed.append((out.tolist(), int(tok), int(pos), int(c)))
    assert replayed == eager


def test_bad_arguments(ops):
    x = _rows(1000)
    w = torch.zeros(8, dtype=torch.int32, device=DEV)
    c = _counter(0)
    with pytest.raises(ValueError):
        ops.spec_accept_sample(torch.cat([x, x[:1]]), torch.zeros(9, dtype=torch.int32, device=DEV), 200, 0.8,
                               counter=c)
    for k in (0, 2000):
        with pytest.raises(ValueError):
            ops.spec_accept_sample(x[:4], w[:4], k, 0.8, counter=c)
    with pytest.raises(ValueError):
        ops.spec_accept_sample(x[:4], w[:3], 200, 0.8, counter=c)
    with pytest.raises(ValueError):
        ops.spec_accept_sample(x[:4], w[:4], 200, 0.8)
    with pytest.raises(ValueError):
        ops.spec_accept_sample(x[:4], w[:4], 200, 0.0, counter=c)
    assert int(c) == 0
    # the raw entry refuses too (nothing is launched)
    lib = ops.load_library()
    out = torch.zeros(9, dtype=torch.int32, device=DEV)
    tmp = torch.zeros(8, dtype=torch.int32, device=DEV)

    def raw(M, top_k, temperature, counter):
        return lib.lga_spec_accept_sample(x.data_ptr(), M, 1000, top_k, temperature, None, 0, counter, w.data_ptr(),
                                          tmp.data_ptr(), out.data_ptr(), None, None, None)

    assert raw(0, 200, 0.8, c.data_ptr()) != 0
    assert raw(9, 200, 0.8, c.data_ptr()) != 0
    assert raw(4, 200, 0.0, c.data_ptr()) != 0
    assert raw(4, 0, 0.8, c.data_ptr()) != 0
    assert raw(4, 200, 0.8, None) != 0
    torch.cuda.synchronize()
    assert int(c) == 0 and not out.any()


# ------------------------------------------------------------------------------------------------ end to end
TEMP, TOP_K = 0.8, 200


def _reference(model, prompt, seed=SEED, tag="bf16", **kw):
    """``generate`` under sampling with the seed (computed once per setting, on whatever cache the model holds)."""
    from generate.base import SamplerRNG, generate

    kw = {"temperature": TEMP, "top_k": TOP_K, **kw}
    key = ("gen", id(model), tuple(prompt.tolist()), seed, tag, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = generate(model, prompt, prompt.numel() + NEW, rng=SamplerRNG(torch.device(DEV), seed=seed),
                               **kw).cpu()
    return _CACHE[key]


def _spec(model, prompt, drafter, seed=SEED, **kw):
    from generate.base import SamplerRNG
    from generate.speculative import generate_speculative

    kw = {"temperature": TEMP, "top_k": TOP_K, **kw}
    return generate_speculative(model, prompt, prompt.numel() + NEW, drafter,
                                rng=SamplerRNG(torch.device(DEV), seed=seed), **kw).cpu()


@pytest.mark.parametrize("mode,groups", [("int4-g128", 8), ("nf4", 8), ("int4-g128", 4)])
@pytest.mark.parametrize("gamma", [1, 3, 7])
def test_scripted_drafter_equals_sampled_generate(mode, groups, gamma):
    from generate.speculative import ScriptedDrafter

    model = _model(mode, groups)
    V = model.config.vocab_size
    prompt = _prompt(V, 33)
    T = prompt.numel()
    _fresh(model)
    ref = _reference(model, prompt)
    assert ref.numel() == T + NEW and len(set(ref[T:].tolist())) > NEW // 2
    steps = NEW - 1
    schedules = {"never": lambda rnd, i: False, "always": lambda rnd, i: True}
    for j in range(gamma):
        schedules[f"index{j}"] = (lambda j: lambda rnd, i: i == j)(j)
    for name, wrong in schedules.items():
        stats = {}
        _fresh(model)
        y = _spec(model, prompt, ScriptedDrafter(ref.tolist(), wrong, V), speculate=gamma, stats=stats)
        assert torch.equal(y, ref), (name, gamma)
        assert stats["tokens"] == steps
        if name == "never":
            assert stats["accepted"] == stats["proposed"] and stats["rounds"] == -(-steps // (gamma + 1))
        if name == "always":
            assert stats["accepted"] == 0 and stats["rounds"] == steps
    eos = int(ref[T + 1 + 9])  # from the middle of the output
    _fresh(model)
    cut = _reference(model, prompt, eos_id=eos)
    assert cut.numel() < T + NEW and int(cut[-1]) == eos
    for wrong in (schedules["never"], schedules["index0"]):
        _fresh(model)
        y = _spec(model, prompt, ScriptedDrafter(ref.tolist(), wrong, V), speculate=gamma, eos_id=eos)
        assert torch.equal(y, cut), gamma
    _fresh(model)


def test_graph_equals_eager_and_seeds_differ():
    from generate.speculative import ScriptedDrafter

    model = _model("int4-g128", 8)
    V = model.config.vocab_size
    prompt = _prompt(V, 5)
    _fresh(model)
    ref = _reference(model, prompt)
    for use_graph in (True, False):
        _fresh(model)
        d = ScriptedDrafter(ref.tolist(), lambda rnd, i: (rnd + i) % 3 == 2, V)
        assert torch.equal(_spec(model, prompt, d, speculate=3, use_graph=use_graph), ref), use_graph
    _fresh(model)
    other = _reference(model, prompt, seed=4321)
    assert not torch.equal(other, ref)
    _fresh(model)
    d = ScriptedDrafter(ref.tolist(), lambda rnd, i: False, V)  # drafts of ANOTHER seed's run: they only cost rounds
    assert torch.equal(_spec(model, prompt, d, seed=4321, speculate=3), other)
    _fresh(model)


def test_rng_from_torch_generator_as_generate():
    """``rng=None`` seeds from torch's generator exactly as ``generate`` does."""
    from generate.base import generate
    from generate.speculative import NgramDrafter, generate_speculative

    model = _model("int4-g128", 8)
    prompt = _prompt(model.config.vocab_size, 5)
    _fresh(model)
    torch.manual_seed(7)
    ref = generate(model, prompt, 5 + NEW, temperature=TEMP, top_k=TOP_K).cpu()
    _fresh(model)
    torch.manual_seed(7)
    y = generate_speculative(model, prompt, 5 + NEW, NgramDrafter(), temperature=TEMP, top_k=TOP_K).cpu()
    assert torch.equal(y, ref)
    _fresh(model)


def test_ngram_drafter_on_repeated_prompt_equals_sampled_generate():
    from generate.speculative import NgramDrafter

    model = _model("int4-g128", 4)
    prompt = _prompt(model.config.vocab_size, 9).repeat(4)
    _fresh(model)
    ref = _reference(model, prompt)
    stats = {}
    _fresh(model)
    y = _spec(model, prompt, NgramDrafter(3), speculate=3, stats=stats)
    assert torch.equal(y, ref)
    assert stats["proposed"] > 0
    _fresh(model)


@pytest.mark.parametrize("draft", ["same", "other-seed", "nf4-twin"])
@pytest.mark.parametrize("coupled", [True, False])
def test_model_drafter_equals_sampled_generate(draft, coupled):
    from generate.speculative import ModelDrafter

    model = _model("int4-g128", 8)
    dm = {"same": lambda: _model("int4-g128", 8, copy=1), "other-seed": lambda: _model("int4-g128", 8, seed=77),
          "nf4-twin": lambda: _model("nf4", 8)}[draft]()
    assert dm is not model
    prompt = _prompt(model.config.vocab_size, 33)
    _fresh(model)
    ref = _reference(model, prompt)
    for gamma in (3, 7):
        stats = {}
        _fresh(model)
        _fresh(dm)
        y = _spec(model, prompt, ModelDrafter(dm, coupled=coupled), speculate=gamma, stats=stats)
        assert torch.equal(y, ref), (draft, coupled, gamma)
        print(f"{draft} coupled={coupled} gamma {gamma}: accepted {stats['accepted']} of {stats['proposed']} in "
              f"{stats['rounds']} rounds")
        if draft == "same" and coupled:  # the same logits under the same uniforms: every draft is the target's sample
            assert stats["accepted"] == stats["proposed"] and stats["rounds"] == -(-(NEW - 1) // (gamma + 1))
    _fresh(model)
    _fresh(dm)


def test_windows_shortened_by_the_cache_end():
    """A prompt that leaves the cache exactly the rows the run needs: the last windows shrink to what still fits."""
    from generate.speculative import ScriptedDrafter

    model = _model("int4-g128", 8)
    V = model.config.vocab_size
    T = S - NEW + 1  # max_returned_tokens - 1 == max_seq_length
    prompt = _prompt(V, T)
    _fresh(model)
    ref = _reference(model, prompt)
    for wrong in (lambda rnd, i: False, lambda rnd, i: i == 2):
        _fresh(model)
        assert torch.equal(_spec(model, prompt, ScriptedDrafter(ref.tolist(), wrong, V), speculate=7), ref)
    _fresh(model)


def test_fp8_kv_cache_target():
    from generate.speculative import NgramDrafter, ScriptedDrafter

    model = _model("int4-g128", 8)
    V = model.config.vocab_size
    fp8 = dict(batch_size=1, device=torch.device(DEV), dtype=torch.float8_e4m3fn)
    prompt = _prompt(V, 9).repeat(4)
    try:
        model.set_kv_cache(**fp8)
        ref = _reference(model, prompt, tag="fp8")
        for drafter in (NgramDrafter(3), ScriptedDrafter(ref.tolist(), lambda rnd, i: i == 1, V)):
            model.set_kv_cache(**fp8)
            assert torch.equal(_spec(model, prompt, drafter, speculate=4), ref)
    finally:
        _fresh(model)


def test_top_k_1_is_greedy():
    from generate.speculative import NgramDrafter, generate_speculative

    model = _model("int4-g128", 4)
    prompt = _prompt(model.config.vocab_size, 9).repeat(4)
    _fresh(model)
    greedy = generate_speculative(model, prompt, prompt.numel() + NEW, NgramDrafter(3)).cpu()
    for temperature in (0.8, 1.7):
        _fresh(model)
        y = _spec(model, prompt, NgramDrafter(3), temperature=temperature, top_k=1)
        assert torch.equal(y, greedy), temperature
    _fresh(model)


def test_refusals():
    from generate.speculative import NgramDrafter, generate_speculative

    model = _model("int4-g128", 8)
    prompt = _prompt(model.config.vocab_size, 5)
    for top_k in (None, 0, 2000):
        with pytest.raises(NotImplementedError):
            generate_speculative(model, prompt, 12, NgramDrafter(), temperature=0.8, top_k=top_k)
