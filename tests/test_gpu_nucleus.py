"""Nucleus (top-p) sampling on the MI355X: the one-row kernel (csrc/sample.hip lga_sample_nucleus) against the integer
specification (tests/nucleus_spec.py), the window entry (lga_spec_accept_sample_nucleus) against the one-row kernel,
and ``top_p`` through generate / generate_batch / generate_continuous / generate_speculative.

The specification is exact from the probabilities on, so the nucleus flags and the token are compared with ``==`` on
the kernel's own probabilities; the probabilities themselves (one fp32 sum of unspecified order) within one bf16 ulp.
"""

import numpy as np
import pytest
import torch

import nucleus_spec as ns
from test_gpu_sample import _logits
from test_gpu_speculative import DEV, NEW, _fresh, _model, _prompt

pytestmark = pytest.mark.gpu

SEED = 1234
TEMP, TOP_P = 0.8, 0.9
US = (0.013, 0.37, 0.5, 0.93, 0.9999)
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _counter(c):
    return torch.tensor([c], dtype=torch.int64, device=DEV)


def _on_device(x):
    """The row on the device; 7 logits as row 1 of a (3, 7) tensor, which starts 14 bytes in (not 4-B aligned)."""
    if x.numel() == 7:
        return torch.stack([x, x, x]).to(DEV)[1]
    return x.to(DEV)


def _launch(ops, xd, k, top_p, T, u, outputs=True):
    n = xd.numel()
    c = min(k, n) if k else n
    uni = torch.tensor([u], dtype=torch.float32, device=DEV)
    if not outputs:
        return int(ops.sample_nucleus(xd, k, top_p, T, uniform=uni).item())
    kept = torch.full((c,), -1, dtype=torch.int32, device=DEV) if k else None
    probs = torch.full((c,), -1.0, dtype=torch.bfloat16, device=DEV)
    flags = torch.full((c,), 7, dtype=torch.uint8, device=DEV)
    tok = ops.sample_nucleus(xd, k, top_p, T, uniform=uni, kept_out=kept, probs_out=probs, nucleus_out=flags)
    return (int(tok.item()), None if kept is None else kept.cpu().numpy(), probs.float().cpu().numpy(),
            flags.cpu().numpy().astype(bool))


NK = [(32000, 200), (32000, None), (50304, None), (65536, None), (1000, 1000), (1000, None), (7, 200), (7, None),
      (32000, 1024), (32000, 1)]


@pytest.mark.parametrize("n,k", NK)
def test_kernel_matches_the_spec(ops, n, k):
    for ties in (False, True, "peaked", "ninf"):
        x = _logits(n, n * 7 + (k or 0), ties)
        xd = _on_device(x)
        cand = ns.candidates(x, k)
        values = x.float().numpy()[cand]
        for T in (0.8, 1.7):
            p_spec = ns.probabilities(x, cand, T)
            w_spec = ns.weights(p_spec)
            for top_p in (0.05, 0.5, 0.9, 0.999, 1.0):
                what = (n, k, ties, T, top_p)
                tok, kept, p, flags = _launch(ops, xd, k, top_p, T, US[0])
                if k:
                    assert np.array_equal(kept, cand), what  # the oracle's kept set, in index order
                assert np.allclose(p, p_spec, rtol=2 ** -7, atol=0), what  # one bf16 ulp
                w = ns.weights(p)
                own, W, _ = ns.nucleus_flags(values, w, top_p)
                assert W < 2 ** 31
                assert np.array_equal(flags, own), what  # the spec's flags on the kernel's own probabilities
                ref, _, _ = ns.nucleus_flags(values, w_spec, top_p)
                steps = np.cumsum(np.where(ref, w_spec, 0)).astype(np.float64)
                if ties == "peaked":
                    assert flags.sum() == 1 and cand[flags][0] == n // 3, what
                for u in US:
                    t = tok if u == US[0] else _launch(ops, xd, k, top_p, T, u, outputs=False)
                    j, tau, Wn = ns.draw(w, own, u)
                    assert 1 <= tau <= Wn and t == int(cand[j]), (what, u)
                    if ties == "peaked":
                        assert t == n // 3
                    if np.array_equal(own, ref) and np.min(np.abs(steps - u * steps[-1])) > 2.0 ** -10 * steps[-1]:
                        assert t == int(cand[ns.draw(w_spec, ref, u)[0]]), (what, u)


@pytest.mark.parametrize("k", [200, None])
def test_bookkeeping_and_embedding(ops, k):
    n, C = 32000, 4096
    x = _logits(n, 5).to(DEV)
    table = (torch.randn(n, C, generator=torch.Generator().manual_seed(2)) * 0.02).bfloat16().to(DEV)
    emb = torch.empty(C, dtype=torch.bfloat16, device=DEV)
    tok = torch.zeros(1, dtype=torch.int32, device=DEV)
    pos = torch.tensor([41], device=DEV)
    uni = torch.tensor([0.6], dtype=torch.float32, device=DEV)
    c = _counter(5)
    idx = ops.sample_nucleus(x, k, TOP_P, 0.8, uniform=uni, counter=c, token_out=tok, pos_inout=pos, table=table,
                             emb_out=emb)
    t = int(idx.item())
    assert tok.item() == t and pos.item() == 42 and int(c) == 5  # explicit uniforms leave the counter alone
    assert torch.equal(emb, table[t])
    assert t == _launch(ops, x, k, TOP_P, 0.8, 0.6, outputs=False)


@pytest.mark.parametrize("k", [None, 8])
def test_counter_rng_stays_in_the_nucleus_and_replays_in_a_graph(ops, k):
    x = torch.full((1000,), -30.0)
    vals = torch.tensor([2.0, 1.5, 1.0, 0.5, 0.0, -0.5, -1.0, -1.5])
    where = torch.tensor([900, 3, 500, 77, 78, 10, 999, 0])
    x[where] = vals
    x = x.bfloat16()
    cand = ns.candidates(x, k)
    p = ns.probabilities(x, cand, 1.0)
    w = ns.weights(p)
    order = np.argsort(-p, kind="stable")
    top_p = float((w[order[:2]].sum() + w[order[:3]].sum()) / 2 / w.sum())  # between the top 2's and the top 3's mass
    flags, _, _ = ns.nucleus_flags(x.float().numpy()[cand], w, top_p)
    nucleus = sorted(int(cand[i]) for i in np.flatnonzero(flags))
    assert nucleus == [3, 500, 900]
    xd = x.to(DEV)
    counter = _counter(0)
    out = torch.zeros(4000, dtype=torch.int64, device=DEV)
    for i in range(4000):
        ops.sample_nucleus(xd, k, top_p, 1.0, seed=1234, counter=counter, out_idx=out[i:i + 1])
    assert counter.item() == 4000
    got = out.cpu()
    assert set(got.tolist()) <= set(nucleus)
    pn = torch.tensor([float(w[list(cand).index(j)]) for j in nucleus], dtype=torch.float64)
    pn = pn / pn.sum()  # the renormalised probabilities
    freq = torch.tensor([(got == j).sum().item() for j in nucleus], dtype=torch.float64) / 4000
    sd = torch.sqrt(pn * (1 - pn) / 4000)
    assert torch.all((freq - pn).abs() < 5 * sd + 1e-3), (freq, pn)
    # draw i is the draw under the host's uniform for (seed, i)
    for i in (0, 1, 17):
        assert int(got[i]) == _launch(ops, xd, k, top_p, 1.0, ops.sampler_uniform(1234, i), outputs=False)
    c2, o2 = _counter(0), torch.zeros(1, dtype=torch.int64, device=DEV)
    g = torch.cuda.CUDAGraph()
    ops.sample_nucleus(xd, k, top_p, 1.0, seed=1234, counter=c2, out_idx=o2)  # warm
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        ops.sample_nucleus(xd, k, top_p, 1.0, seed=1234, counter=c2, out_idx=o2)
    c2.fill_(0)
    seq = []
    for _ in range(50):
        g.replay()
        seq.append(int(o2.item()))
    assert c2.item() == 50 and seq == got[:50].tolist()


# ------------------------------------------------------------------------------------------------ the window entry
def _rows(n):
    if ("rows", n) not in _CACHE:
        kinds = {1: True, 2: "peaked"}
        _CACHE[("rows", n)] = torch.stack([_logits(n, 100 * n + r, kinds.get(r, False)) for r in range(8)]).to(DEV)
    return _CACHE[("rows", n)]


def _one_row(ops, logits, k, T, u=None, c0=None):
    out = torch.zeros(logits.shape[0], dtype=torch.int64, device=DEV)
    for r in range(logits.shape[0]):
        if u is not None:
            ops.sample_nucleus(logits[r], k, TOP_P, T, uniform=u[r:r + 1], out_idx=out[r:r + 1])
        else:
            ops.sample_nucleus(logits[r], k, TOP_P, T, seed=SEED, counter=_counter(c0 + r), out_idx=out[r:r + 1])
    return out.tolist()


@pytest.mark.parametrize("n", [32000, 50304, 1000, 7])
@pytest.mark.parametrize("k", [None, 200])
def test_window_rows_equal_the_one_row_sampler(ops, n, k):
    rows = _rows(n)
    u = torch.tensor([0.013, 0.37, 0.5, 0.93, 0.9999, 0.2, 0.66, 0.81], dtype=torch.float32, device=DEV)
    T = TEMP
    ref_u = _one_row(ops, rows, k, T, u=u)
    ref_c = _one_row(ops, rows, k, T, c0=41)
    for M in (1, 2, 5, 8):
        logits = rows[:M]
        out = ops.spec_accept_sample_nucleus(logits, _i32([5] + ref_u[:M - 1]), k, TOP_P, T,
                                             uniform=u[:M].contiguous()).tolist()
        assert out[0] == M - 1 and out[1:M + 1] == ref_u[:M], (M, out, ref_u)
        c = _counter(41)
        out = ops.spec_accept_sample_nucleus(logits, _i32([5] + ref_c[:M - 1]), k, TOP_P, T, seed=SEED,
                                             counter=c).tolist()
        assert out[0] == M - 1 and out[1:M + 1] == ref_c[:M] and int(c) == 41 + M, (M, out, ref_c)


@pytest.mark.parametrize("M", [1, 2, 5, 8])
@pytest.mark.parametrize("k", [None, 200])
def test_window_acceptance_and_bookkeeping(ops, M, k):
    n, T, c0, pos0 = 1000, 0.8, 41, 17
    logits = _rows(n)[:M]
    before = logits.clone()
    t = _one_row(ops, logits, k, T, c0=c0)
    good = [7] + t[:M - 1]
    cases = [(M - 1, list(good)), (M - 1, [8] + good[1:])]
    for i in range(M - 1):
        w = list(good)
        w[1 + i] = (w[1 + i] + 1) % n
        cases.append((i, w))
    for want, w in cases:
        window = _i32(w)
        tok, pos, c = _i32([-5]), torch.tensor([pos0], dtype=torch.int64, device=DEV), _counter(c0)
        out = ops.spec_accept_sample_nucleus(logits, window, k, TOP_P, T, seed=SEED, counter=c, token_inout=tok,
                                             pos_inout=pos).tolist()
        a = out[0]
        assert a == want, (w, out)
        assert out[1:a + 2] == t[:a + 1] and all(v == -1 for v in out[a + 2:]) and len(out) == M + 1
        assert int(tok) == t[a] and int(pos) == pos0 + a + 1 and int(c) == c0 + a + 1
        assert window.tolist() == w and torch.equal(logits, before)
    window = _i32(good + [0] * (8 - M))  # the executor's aliasing: token_inout is window[0]
    c = _counter(c0)
    out = ops.spec_accept_sample_nucleus(logits, window[:M], k, TOP_P, T, seed=SEED, counter=c,
                                         token_inout=window[:1]).tolist()
    assert out[0] == M - 1 and window.tolist() == [t[M - 1]] + good[1:] + [0] * (8 - M)
    u = torch.full((M,), 0.4, dtype=torch.float32, device=DEV)
    c = _counter(c0)
    ops.spec_accept_sample_nucleus(logits, _i32(good), k, TOP_P, T, uniform=u, counter=c)
    assert int(c) == c0


def test_refusals(ops):
    x = _rows(1000)
    w = torch.zeros(8, dtype=torch.int32, device=DEV)
    c = _counter(0)
    for bad in (dict(top_k=0), dict(top_k=2000), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5),
                dict(temperature=0.0), dict(counter=None)):
        kw = {"top_k": 200, "top_p": 0.9, "temperature": 0.8, "counter": c, **bad}
        with pytest.raises(ValueError):
            ops.sample_nucleus(x[0], kw["top_k"], kw["top_p"], kw["temperature"], counter=kw["counter"])
        with pytest.raises(ValueError):
            ops.spec_accept_sample_nucleus(x[:4], w[:4], kw["top_k"], kw["top_p"], kw["temperature"],
                                           counter=kw["counter"])
    with pytest.raises(ValueError):
        ops.sample_nucleus(_logits(70000, 1).to(DEV), None, 0.9, 0.8, counter=c)
    with pytest.raises(ValueError):
        ops.spec_accept_sample_nucleus(x[:4], w[:3], 200, 0.9, 0.8, counter=c)
    lib = ops.load_library()
    out = torch.zeros(9, dtype=torch.int32, device=DEV)
    tmp = torch.zeros(8, dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, dtype=torch.int64, device=DEV)

    def one(n=1000, top_k=200, top_p=0.9, temperature=0.8, counter=c.data_ptr()):
        return lib.lga_sample_nucleus(x.data_ptr(), n, top_k, top_p, temperature, None, 0, counter, idx.data_ptr(),
                                      None, None, None, 0, 0, None, None, None, None, None)

    def window(M=4, n=1000, top_k=200, top_p=0.9, temperature=0.8, counter=c.data_ptr()):
        return lib.lga_spec_accept_sample_nucleus(x.data_ptr(), M, n, top_k, top_p, temperature, None, 0, counter,
                                                  w.data_ptr(), tmp.data_ptr(), out.data_ptr(), None, None, None)

    for raw in (one, window):
        for bad in (dict(n=0), dict(n=65537), dict(top_k=-1), dict(top_k=1025), dict(top_p=0.0), dict(top_p=1.5),
                    dict(temperature=0.0), dict(counter=None)):
            assert raw(**bad) != 0, (raw.__name__, bad)
    assert window(M=0) != 0 and window(M=9) != 0
    torch.cuda.synchronize()
    assert int(c) == 0 and not out.any() and not idx.any() and not tmp.any()


# ------------------------------------------------------------------------------------------------ end to end
def _generate(model, prompt, seed=SEED, new=NEW, **kw):
    from generate.base import SamplerRNG, generate

    kw = {"temperature": TEMP, "top_p": TOP_P, **kw}
    return generate(model, prompt, prompt.numel() + new, rng=SamplerRNG(torch.device(DEV), seed=seed), **kw).cpu()


def _reference(model, prompt, top_k, seed=SEED, tag="bf16", **kw):
    key = ("gen", id(model), tuple(prompt.tolist()), top_k, seed, tag, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = _generate(model, prompt, seed, top_k=top_k, **kw)
    return _CACHE[key]


@pytest.mark.parametrize("mode,groups,top_k", [("int4-g128", 8, None), ("int4-g128", 8, 200), ("nf4", 8, None)])
def test_generate_graph_equals_eager_inside_the_nucleus(ops, mode, groups, top_k):
    model = _model(mode, groups)
    V = model.config.vocab_size
    prompt = _prompt(V, 9)
    T = prompt.numel()
    _fresh(model)
    ref = _reference(model, prompt, top_k)
    assert ref.numel() == T + NEW
    _fresh(model)
    assert torch.equal(_generate(model, prompt, top_k=top_k, use_graph=False), ref)
    _fresh(model)
    assert not torch.equal(_generate(model, prompt, seed=4321, top_k=top_k), ref)
    # teacher-forced, eager: every sampled token lies in its step's nucleus (the spec's flags on the probabilities the
    # kernel reports for those logits)
    _fresh(model)
    with torch.inference_mode():
        logits = [model(prompt.view(1, -1), torch.arange(T, device=DEV), last_token_only=True)[0, -1].clone()]
        for i in range(NEW - 1):
            tok = ref[T + i:T + i + 1].to(DEV).to(prompt.dtype)
            logits.append(model(tok.view(1, 1), torch.tensor([T + i], device=DEV), last_token_only=True)[0, -1].clone())
    for i, lg in enumerate(logits):
        _, kept, p, flags = _launch(ops, lg.contiguous(), top_k, TOP_P, TEMP, 0.5)
        x = lg.cpu()
        cand = ns.candidates(x, top_k)
        own, _, _ = ns.nucleus_flags(x.float().numpy()[cand], ns.weights(p), TOP_P)
        assert np.array_equal(flags, own)
        assert int(ref[T + i]) in set(cand[own].tolist()), i
    _fresh(model)


def test_generate_on_an_unquantized_model():
    from generate.base import build_model
    from lit_gpt import Config

    cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=8, intermediate_size=2816)
    model = build_model(cfg, quantize=None, device=torch.device(DEV), max_seq_length=48)
    prompt = _prompt(cfg.vocab_size, 9)
    outs = []
    for use_graph in (True, False):
        _fresh(model)
        outs.append(_generate(model, prompt, top_k=None, use_graph=use_graph))
    assert torch.equal(outs[0], outs[1]) and outs[0].numel() == 9 + NEW
    assert len(set(outs[0][9:].tolist())) > NEW // 2


@pytest.mark.parametrize("top_k", [None, 200])
def test_generate_batch_equals_generate_per_seed(top_k):
    from generate.base import generate_batch

    model = _model("int4-g128", 8)
    V = model.config.vocab_size
    prompts = [_prompt(V, 5), _prompt(V, 33)]
    seeds = [1234, 99]
    refs = []
    for p, s in zip(prompts, seeds):
        _fresh(model)
        refs.append(_reference(model, p, top_k, seed=s))
    outs = generate_batch(model, prompts, NEW, temperature=TEMP, top_k=top_k, top_p=TOP_P, seeds=seeds)
    for o, r in zip(outs, refs):
        assert torch.equal(o.cpu(), r), (o.tolist(), r.tolist())
    _fresh(model)


@pytest.mark.parametrize("top_k", [None, 200])
def test_generate_continuous_equals_generate_per_seed(top_k):
    from generate.base import generate_continuous

    model = _model("int4-g128", 4)
    V = model.config.vocab_size
    prompts = [_prompt(V, 5), _prompt(V, 33), _prompt(V, 9)]
    budgets, seeds = [24, 20, 16], [1234, 99, 2**40 + 5]
    _fresh(model)
    free = _generate(model, prompts[0], seeds[0], new=budgets[0], top_k=top_k)
    eos = int(free[5 + 7])  # a decoded token of the first stream: that sequence ends early
    refs = []
    for p, m, s in zip(prompts, budgets, seeds):
        _fresh(model)
        refs.append(_generate(model, p, s, new=m, top_k=top_k, eos_id=eos))
    assert refs[0].numel() < 5 + budgets[0] and int(refs[0][-1]) == eos
    outs = generate_continuous(model, prompts, budgets, batch_size=2, temperature=TEMP, top_k=top_k, top_p=TOP_P,
                               eos_id=eos, seeds=seeds)
    for o, r in zip(outs, refs):
        assert torch.equal(o.cpu(), r), (o.tolist(), r.tolist())
    _fresh(model)


def _spec(model, prompt, drafter, top_k, seed=SEED, **kw):
    from generate.base import SamplerRNG
    from generate.speculative import generate_speculative

    return generate_speculative(model, prompt, prompt.numel() + NEW, drafter, temperature=TEMP, top_k=top_k,
                                top_p=TOP_P, rng=SamplerRNG(torch.device(DEV), seed=seed), **kw).cpu()


@pytest.mark.parametrize("top_k", [None, 200])
@pytest.mark.parametrize("gamma", [1, 7])
def test_scripted_drafter_equals_generate(gamma, top_k):
    from generate.speculative import ScriptedDrafter

    model = _model("int4-g128", 8)
    V = model.config.vocab_size
    prompt = _prompt(V, 33)
    _fresh(model)
    ref = _reference(model, prompt, top_k)
    steps = NEW - 1
    schedules = {"never": lambda rnd, i: False, "always": lambda rnd, i: True, "index0": lambda rnd, i: i == 0}
    for name, wrong in schedules.items():
        stats = {}
        _fresh(model)
        y = _spec(model, prompt, ScriptedDrafter(ref.tolist(), wrong, V), top_k, speculate=gamma, stats=stats)
        assert torch.equal(y, ref), (name, gamma)
        if name == "never":
            assert stats["accepted"] == stats["proposed"] and stats["rounds"] == -(-steps // (gamma + 1))
        if name == "always":
            assert stats["accepted"] == 0 and stats["rounds"] == steps
    _fresh(model)


@pytest.mark.parametrize("top_k", [None, 200])
def test_coupled_model_drafter_equals_generate(top_k):
    from generate.speculative import ModelDrafter

    model = _model("int4-g128", 8)
    dm = _model("int4-g128", 8, copy=1)
    prompt = _prompt(model.config.vocab_size, 33)
    _fresh(model)
    ref = _reference(model, prompt, top_k)
    stats = {}
    _fresh(model)
    _fresh(dm)
    y = _spec(model, prompt, ModelDrafter(dm, coupled=True), top_k, speculate=3, stats=stats)
    assert torch.equal(y, ref)
    # the same logits under the same uniforms at the same top_p: every draft is the target's sample
    assert stats["accepted"] == stats["proposed"] and stats["rounds"] == -(-(NEW - 1) // 4)
    _fresh(model)
    _fresh(dm)


def test_speculative_on_an_fp8_kv_cache():
    from generate.speculative import ScriptedDrafter

    model = _model("int4-g128", 8)
    V = model.config.vocab_size
    fp8 = dict(batch_size=1, device=torch.device(DEV), dtype=torch.float8_e4m3fn)
    prompt = _prompt(V, 9).repeat(4)
    try:
        model.set_kv_cache(**fp8)
        ref = _reference(model, prompt, None, tag="fp8")
        model.set_kv_cache(**fp8)
        y = _spec(model, prompt, ScriptedDrafter(ref.tolist(), lambda rnd, i: i == 1, V), None, speculate=4)
        assert torch.equal(y, ref)
    finally:
        _fresh(model)
