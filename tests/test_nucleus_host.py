"""Nucleus (top-p) sampling without a GPU: the integer specification (tests/nucleus_spec.py) against a float64
restatement and the usual sort-ascending rule, the specification's own properties, and the host plumbing of ``top_p``
(device_sampling / graph_sampling, the command lines, the refusals that come before any device work)."""

import itertools
import types

import numpy as np
import pytest
import torch

import nucleus_spec as ns

NK = [(32000, None), (50304, None), (32000, 200), (32000, 1024), (1000, 1000), (7, 200), (300, None)]
TEMPS = (0.8, 1.7)
TOP_PS = (0.05, 0.5, 0.9, 0.99)
_CACHE = {}


def _logits(n, ties, gen):
    x = torch.randn(n, generator=gen) * 3
    return (x.round() if ties else x).to(torch.bfloat16)


def _cases():
    """(n, k, ties, T) -> (logits, candidates, values, probabilities, weights); drawn once, in a fixed order."""
    if "cases" not in _CACHE:
        gen = torch.Generator().manual_seed(1)
        out = {}
        for (n, k), ties in itertools.product(NK, (False, True)):
            x = _logits(n, ties, gen)
            cand = ns.candidates(x, k)
            for T in TEMPS:
                p = ns.probabilities(x, cand, T)
                out[(n, k, ties, T)] = (x, cand, x.float().numpy()[cand].astype(np.float64), p, ns.weights(p))
        _CACHE["cases"] = out
    return _CACHE["cases"]


def _float64_flags(values, p, top_p):
    """Classes in descending value, each entering whole, until cumulative mass / total >= top_p. Returns the flags
    and the distance of the nearest class boundary's cumulative mass from top_p."""
    p = p.astype(np.float64)
    uniq, inv = np.unique(values, return_inverse=True)
    mass = np.bincount(inv, weights=p, minlength=uniq.size)[::-1] / p.sum()  # descending classes
    cum = np.cumsum(mass)
    before = cum - mass
    keep_desc = before < top_p
    return keep_desc[::-1][inv], float(np.min(np.abs(cum - top_p)))


def test_spec_equals_the_float64_restatement():
    left_out = total = sorted_checked = 0
    for (n, k, ties, T), (x, cand, values, p, w) in _cases().items():
        for top_p in TOP_PS:
            total += 1
            flags, W, target = ns.nucleus_flags(values, w, top_p)
            assert 1 <= target <= W < 2 ** 31
            ref, margin = _float64_flags(values, p, top_p)
            if margin < 1e-4:
                left_out += 1
                continue
            assert np.array_equal(flags, ref), (n, k, ties, T, top_p)
            if np.unique(values).size == values.size:  # tie-free: the usual rule over ascending probabilities
                order = np.argsort(values, kind="stable")
                cum = np.cumsum(p.astype(np.float64)[order] / p.astype(np.float64).sum())
                drop = cum <= 1.0 - top_p
                drop[-1] = False
                usual = np.empty_like(drop)
                usual[order] = ~drop
                assert np.array_equal(flags, usual), (n, k, ties, T, top_p)
                sorted_checked += 1
    assert total == 112 and left_out <= 0.15 * total, (left_out, total)
    assert sorted_checked > 0


def test_spec_properties():
    for (n, k, ties, T), (x, cand, values, p, w) in _cases().items():
        W = int(w.sum())
        assert W < 2 ** 31 and W / 2 ** 30 < 1.0 + 2.0 ** -7
        prev = None
        top = values == values.max()
        for top_p in (0.05, 0.5, 0.9, 0.99, 0.999, 1.0):
            flags, _, _ = ns.nucleus_flags(values, w, top_p)
            assert flags[top].all()  # the top class is always kept
            if prev is not None:
                assert not (prev & ~flags).any()  # monotone in top_p
            prev = flags
            for u in (2.0 ** -24, 0.37, 1.0 - 2.0 ** -24):
                j, tau, Wn = ns.draw(w, flags, u)
                assert 1 <= tau <= Wn and flags[j] and w[j] > 0
    x = _cases()[(32000, 200, False, 0.8)][0]
    for u in (2.0 ** -24, 0.013, 0.5, 0.9999, 1.0 - 2.0 ** -24):
        for top_p in (0.05, 0.9, 1.0):
            cand, p, flags, tok = ns.nucleus_spec(x, 1, top_p, 0.8, u)
            assert tok == int(torch.argmax(x.float())) and cand.tolist() == [tok] and flags.tolist() == [True]
    # probs given: steps 3-5 run on them
    cand, p, flags, tok = ns.nucleus_spec(x, 200, 0.9, 0.8, 0.37)
    again = ns.nucleus_spec(x, 200, 0.9, 0.8, 0.37, probs=p)
    assert np.array_equal(again[2], flags) and again[3] == tok and tok in cand[flags].tolist()


# ------------------------------------------------------------------------------------------------ host plumbing
def test_device_sampling_truth_table():
    from generate.base import device_sampling, graph_sampling

    bf, f32 = torch.bfloat16, torch.float32
    # the rows of today, unchanged
    assert device_sampling(0.8, 200, bf) and device_sampling(0.8, 1, bf) and device_sampling(0.8, 1024, bf, 65536)
    assert not device_sampling(0.8, None, bf) and not device_sampling(0.8, 1025, bf)
    assert not device_sampling(0.0, 200, bf) and not device_sampling(0.8, 200, f32)
    assert not device_sampling(0.8, 200, bf, 65537) and not device_sampling(0.8, 0, bf)
    assert device_sampling(0.8, 200, bf, 0, 1.0) and not device_sampling(0.8, None, bf, 0, 1.0)
    # 0 < top_p < 1
    assert device_sampling(0.8, None, bf, 32000, 0.9) and device_sampling(0.8, 200, bf, 65536, 0.9)
    assert device_sampling(0.8, 1024, bf, top_p=0.5) and device_sampling(0.8, 1, bf, top_p=0.5)
    assert not device_sampling(0.8, 1025, bf, top_p=0.9) and not device_sampling(0.8, 0, bf, top_p=0.9)
    assert not device_sampling(0.0, None, bf, top_p=0.9) and not device_sampling(0.8, None, f32, top_p=0.9)
    assert not device_sampling(0.8, None, bf, 65537, 0.9)

    def model(dtype=bf, vocab=32000):
        wte = types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype))
        return types.SimpleNamespace(config=types.SimpleNamespace(padded_vocab_size=vocab),
                                     transformer=types.SimpleNamespace(wte=wte))

    assert graph_sampling(model(), 0.0, None) and graph_sampling(model(), 0.8, 200)
    assert not graph_sampling(model(), 0.8, None) and not graph_sampling(model(f32), 0.8, 200)
    assert graph_sampling(model(), 0.8, None, top_p=0.9) and graph_sampling(model(), 0.8, 200, 0.9)
    assert not graph_sampling(model(f32), 0.8, None, top_p=0.9)
    assert not graph_sampling(model(vocab=70000), 0.8, None, top_p=0.9)
    assert graph_sampling(model(f32), 0.0, None, top_p=0.9)  # greedy


def test_top_p_flags_reach_main(monkeypatch):
    import chat.base as cb
    import generate.base as gb
    import generate.speculative as gs

    got = {}
    for mod in (gb, cb, gs):
        monkeypatch.setattr(mod, "main", lambda *a, **k: got.update(k))
    gb._cli(["--synthetic", "x", "--top_p", "0.9", "--top_k", "none"])
    assert got["top_p"] == 0.9 and got["top_k"] is None
    got.clear()
    gb._cli(["--synthetic", "x"])
    assert got["top_p"] == 1.0 and got["top_k"] == 200
    got.clear()
    gb._cli(["--synthetic", "x", "--top_k", "50"])
    assert got["top_k"] == 50
    got.clear()
    cb._cli(["--top_p", "0.5", "--top_k", "None"])
    assert got["top_p"] == 0.5 and got["top_k"] is None
    got.clear()
    cb._cli([])
    assert got["top_p"] == 1.0 and got["top_k"] == 200
    got.clear()
    gs._cli(["--draft", "ngram", "--temperature", "0.8", "--top_p", "0.9"])
    assert got["top_p"] == 0.9 and got["top_k"] is None and got["temperature"] == 0.8
    got.clear()
    gs._cli(["--draft", "ngram", "--temperature", "0.8", "--top_p", "0.9", "--top_k", "none"])
    assert got["top_k"] is None
    got.clear()
    gs._cli(["--draft", "ngram", "--temperature", "0.8", "--top_k", "40"])
    assert got["top_p"] == 1.0 and got["top_k"] == 40
    with pytest.raises(SystemExit):  # top_p == 1: greedy only, as before
        gs._cli(["--draft", "ngram", "--temperature", "0.8"])
    with pytest.raises(SystemExit):
        gs._cli(["--draft", "ngram", "--temperature", "0.8", "--top_p", "1.5"])


def _fake_model(max_seq_length=64, dtype=torch.bfloat16, vocab=1000):
    """What the generate functions read before they touch the GPU; any forward is a test failure."""

    def forward(*a, **k):
        raise AssertionError("the fake model must not run")

    wte = types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype))
    return types.SimpleNamespace(max_seq_length=max_seq_length, config=types.SimpleNamespace(padded_vocab_size=vocab),
                                 transformer=types.SimpleNamespace(wte=wte), __call__=forward, forward=forward,
                                 _batch_check=forward)


def _prompt(n):
    return torch.arange(n, dtype=torch.int32)


def test_top_p_refusals_come_before_any_device_work():
    from generate.base import generate, generate_batch, generate_continuous, sample
    from generate.speculative import NgramDrafter, generate_speculative

    m = _fake_model()
    for bad in (0, -0.1, 1.5):
        with pytest.raises(ValueError, match="top_p"):
            generate(m, _prompt(3), 8, temperature=0.8, top_k=50, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            generate_batch(m, [_prompt(3)] * 2, 4, temperature=0.8, top_k=50, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            generate_continuous(m, [_prompt(3)] * 3, 4, batch_size=2, temperature=0.8, top_k=50, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            generate_speculative(m, _prompt(3), 8, NgramDrafter(), temperature=0.8, top_k=50, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            sample(torch.zeros(1, 1, 10, dtype=torch.bfloat16), temperature=0.8, top_k=5, top_p=bad)
    for model, kw in ((_fake_model(dtype=torch.float32), {}), (_fake_model(vocab=70000), {}), (m, {"top_k": 2000})):
        kw = {"top_k": None, **kw}
        with pytest.raises(NotImplementedError, match="device sampler"):
            generate(model, _prompt(3), 8, temperature=0.8, top_p=0.9, **kw)
        with pytest.raises(NotImplementedError, match="device sampler"):
            generate_batch(model, [_prompt(3)] * 2, 4, temperature=0.8, top_p=0.9, **kw)
        with pytest.raises(NotImplementedError, match="device sampler"):
            generate_continuous(model, [_prompt(3)] * 3, 4, batch_size=2, temperature=0.8, top_p=0.9, **kw)
        with pytest.raises(NotImplementedError, match="device sampler"):
            generate_speculative(model, _prompt(3), 8, NgramDrafter(), temperature=0.8, top_p=0.9, **kw)
    with pytest.raises(NotImplementedError, match="device sampler"):  # fp32 logits: no torch fallback for top-p
        sample(torch.zeros(1, 1, 10), temperature=0.8, top_k=5, top_p=0.9)
    # top_p == 1: today's refusals, word for word
    with pytest.raises(NotImplementedError, match="greedy only"):
        generate_speculative(None, _prompt(3), 8, NgramDrafter(), temperature=0.7)
    with pytest.raises(NotImplementedError, match="device sampler"):
        generate_continuous(m, [_prompt(3)] * 3, 4, batch_size=2, temperature=0.8, top_k=None)


def test_ops_signatures_and_runtime_settings():
    from lit_gpt import ops, runtime

    assert len(ops.SIGNATURES["lga_sample_nucleus"]) == len(ops.SIGNATURES["lga_sample_topk"]) + 2
    assert len(ops.SIGNATURES["lga_spec_accept_sample_nucleus"]) == len(ops.SIGNATURES["lga_spec_accept_sample"]) + 1
    ok = runtime._sampling_ok
    assert ok(0.8, 200, 1.0) and not ok(0.8, None, 1.0) and not ok(0.8, 1025, 1.0)
    assert ok(0.8, None, 0.9) and ok(0.8, 200, 0.9) and not ok(0.8, 1025, 0.9) and not ok(0.8, 200, 1.5)
