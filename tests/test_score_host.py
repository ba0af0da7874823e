"""CPU tests of the scoring feature's host logic: the window plan of lit_gpt/score.py against a token-by-token brute
force, the request logic of eval/lm_eval_harness.py against a recording fake of score_tokens and a byte-level stub
tokenizer, the ImportError of the lm_eval glue, and id validation. No kernel runs."""

import sys
import types

import pytest
import torch

import score_spec


# ------------------------------------------------------------------------------------------------ rolling_windows
def _window_cases():
    for max_len in (1, 2, 8):
        for n in sorted({1, 2, max_len - 1, max_len, max_len + 1, 2 * max_len, 2 * max_len + 3}):
            for c in sorted({1, 3, max_len}):
                if n >= 1 and 1 <= c <= max_len:
                    yield n, max_len, c


@pytest.mark.parametrize("n,max_len,min_context", list(_window_cases()))
def test_rolling_windows_match_brute_force(n, max_len, min_context):
    from lit_gpt.score import rolling_windows

    got = list(rolling_windows(n, max_len, -1, min_context))
    assert got == score_spec.rolling_windows_brute(n, max_len, -1, min_context)
    scored = []
    for w, (inp, k) in enumerate(got):
        assert 1 <= k <= len(inp) <= max_len
        last = (scored[-1] if scored else -1) + k  # the window's last scored position
        # row i of the window predicts the token after inp[i]: the input must end right before the last scored token
        want = list(range(last - len(inp), last))
        if w == 0:
            want = [-1] + list(range(last))
            assert len(inp) == last + 1
        assert inp == want
        scored.extend(range(last - k + 1, last + 1))
        # context of the window's first scored token: every input up to and including the one that predicts it
        context = len(inp) - k + 1
        available = (last - k + 1) + 1  # tokens before it, plus the prefix
        assert context >= min(min_context, available)
        if w > 0:
            assert k <= max_len - min_context + 1
    assert scored == list(range(n))  # every token exactly once, in order


def test_rolling_windows_on_a_sequence_and_errors():
    from lit_gpt.score import rolling_windows

    toks = [10, 11, 12, 13, 14, 15, 16]
    assert list(rolling_windows(toks, 3, 99)) == [([99, 10, 11], 3), ([12, 13, 14], 3), ([13, 14, 15], 1)]
    assert list(rolling_windows([], 3, 99)) == []
    with pytest.raises(ValueError, match="min_context"):
        list(rolling_windows(toks, 3, 99, 4))
    with pytest.raises(ValueError, match="max_len"):
        list(rolling_windows(toks, 0, 99))


# ------------------------------------------------------------------------------------------------ harness logic
class ByteTokenizer:
    """One token per byte (ids 0..255); eos 256."""

    eos_id = 256
    vocab_size = 257

    def encode(self, string, device=None, bos=False, eos=False):
        return torch.tensor(list(string.encode()), dtype=torch.int32)

    def decode(self, tensor):
        return bytes(int(t) for t in tensor.tolist() if int(t) < 256).decode(errors="replace")


class FakeModel:
    def __init__(self, max_seq_length):
        self.max_seq_length = max_seq_length


def _harness(monkeypatch, max_len, greedy_of=None):
    """An EvalHarnessBase whose score_tokens is a fake that records (tokens, n_scored) and returns logprob -1 per row
    and, as greedy tokens, ``greedy_of(tokens, n)`` (default: the targets themselves)."""
    import eval.lm_eval_harness as h

    calls = []

    def fake(model, tokens, n_scored):
        tokens = list(tokens)
        calls.append((tokens, n_scored))
        g = tokens[len(tokens) - n_scored:] if greedy_of is None else greedy_of(tokens, n_scored)
        return torch.full((n_scored,), -1.0), torch.tensor(g, dtype=torch.int32)

    monkeypatch.setattr(h.score, "score_tokens", fake)
    return h.EvalHarnessBase(FakeModel(max_len), ByteTokenizer()), calls


def test_harness_surface():
    import eval.lm_eval_harness as h

    lm = h.EvalHarnessBase(FakeModel(77), ByteTokenizer(), batch_size=1)
    assert (lm.eot_token_id, lm.max_length, lm.vocab_size, lm.max_gen_toks, lm.batch_size) == (256, 77, 257, 256, 1)
    assert lm.tok_encode("ab") == [97, 98] and lm.tok_decode([97, 98]) == "ab"
    with pytest.raises(NotImplementedError, match="batch size 1"):
        h.EvalHarnessBase(FakeModel(77), ByteTokenizer(), batch_size=2)


def test_loglikelihood_empty_context_and_rows(monkeypatch):
    lm, calls = _harness(monkeypatch, 32)
    out = lm.loglikelihood([("", "hi"), ("ab", "cde")])
    assert calls[0] == ([256, 104, 105], 2)  # empty context -> [eot]
    assert calls[1] == ([97, 98, 99, 100, 101], 3)  # the rows scored are the continuation's
    assert out == [(-2.0, True), (-3.0, True)]


def test_loglikelihood_left_truncation(monkeypatch):
    lm, calls = _harness(monkeypatch, 4)
    lm.loglikelihood([("abcdefgh", "XY")])
    toks, n = calls[0]
    assert toks == [ord(c) for c in "fghXY"] and n == 2  # the last max_length + 1 tokens: an input of max_length


def test_loglikelihood_is_greedy(monkeypatch):
    def off_by_one_at_last(tokens, n):
        g = tokens[len(tokens) - n:]
        return g[:-1] + [(g[-1] + 1) % 256]

    lm, _ = _harness(monkeypatch, 32, off_by_one_at_last)
    assert lm.loglikelihood([("ab", "cde")]) == [(-3.0, False)]
    lm, _ = _harness(monkeypatch, 32)
    assert lm.loglikelihood([("ab", "cde")]) == [(-3.0, True)]


def test_loglikelihood_rolling_windows(monkeypatch):
    lm, calls = _harness(monkeypatch, 3)
    out = lm.loglikelihood_rolling([("abcdefg",)])
    a = [ord(c) for c in "abcdefg"]
    assert calls == [([256] + a[:3], 3), (a[2:6], 3), (a[3:7], 1)]
    assert out == [-7.0]


def test_greedy_until_context_cut_and_until_split(monkeypatch):
    import eval.lm_eval_harness as h
    import generate.base as gb

    seen = {}

    class Cache:
        resets = 0

        def reset_parameters(self):
            Cache.resets += 1

    class Model(FakeModel):
        def __init__(self, n):
            super().__init__(n)
            blk = types.SimpleNamespace(attn=types.SimpleNamespace(kv_cache=Cache()))
            self.transformer = types.SimpleNamespace(h=[blk, blk],
                                                     wte=types.SimpleNamespace(weight=torch.zeros(1)))

    def fake_generate(model, prompt, max_returned_tokens, *, temperature, eos_id, **kw):
        seen.update(prompt=prompt.tolist(), max_returned=max_returned_tokens, temperature=temperature, eos=eos_id)
        return torch.cat([prompt, torch.tensor(list(b"one. two\nthree"), dtype=prompt.dtype)])

    monkeypatch.setattr(gb, "generate", fake_generate)
    lm = h.EvalHarnessBase(Model(260), ByteTokenizer())
    out = lm.greedy_until([("abcdefgh", {"until": ["\n", "."]})])
    assert seen["prompt"] == [ord(c) for c in "efgh"]  # the last max_length - max_gen_toks = 4 context tokens
    assert seen["max_returned"] == 4 + 256 and seen["temperature"] == 0.0
    assert seen["eos"] == ord("\n")  # the first token of until[0]
    assert out == ["one"]  # cut at the first occurrence of ANY until string
    assert Cache.resets == 2  # the KV caches are reset after the generation
    with pytest.raises(ValueError, match="max_gen_toks"):
        h.EvalHarnessBase(Model(256), ByteTokenizer()).greedy_until([("a", {"until": ["."]})])


def test_run_eval_names_the_missing_package(monkeypatch):
    import eval.lm_eval_harness as h

    monkeypatch.setitem(sys.modules, "lm_eval", None)  # importing it raises ImportError, installed or not
    lm = h.EvalHarnessBase(FakeModel(8), ByteTokenizer())
    with pytest.raises(ImportError, match="lm_eval"):
        lm.run_eval(["piqa"], 0, None, 10, True)
    assert "lm_eval" not in vars(h)  # never imported at module level


# ------------------------------------------------------------------------------------------------ id validation
def _meta_model():
    from lit_gpt import GPT, Config

    cfg = Config.from_name("Llama-2-7b-hf", n_layer=1, n_embd=64, n_head=4, intermediate_size=96, vocab_size=100,
                           padding_multiple=64, block_size=32)
    with torch.device("meta"):
        return GPT(cfg)


@pytest.mark.parametrize("bad", [[1, 2, -1], [1, 128, 3], [5, 10 ** 9]])
def test_score_tokens_rejects_out_of_range_ids_before_any_launch(bad):
    from lit_gpt.score import compare_tokens, score_tokens

    model = _meta_model()  # padded_vocab_size 128; a meta model cannot launch anything
    with pytest.raises(ValueError, match=r"\[0, 128\)"):
        score_tokens(model, bad, 1)
    with pytest.raises(ValueError, match=r"\[0, 128\)"):
        compare_tokens(model, model, bad, 1)


def test_score_tokens_argument_errors():
    from lit_gpt.score import score_tokens

    model = _meta_model()
    with pytest.raises(ValueError, match="n_scored"):
        score_tokens(model, [1, 2, 3], 3)
    with pytest.raises(ValueError, match="max_seq_length"):
        score_tokens(model, list(range(34)), 1)
    with pytest.raises(TypeError, match="integers"):
        score_tokens(model, [0.5, 1.0], 1)


def test_scoring_refuses_tensor_parallelism(monkeypatch):
    from lit_gpt import comm
    from lit_gpt.score import score_tokens

    monkeypatch.setattr(comm, "get_default", lambda: object())
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        score_tokens(_meta_model(), [1, 2, 3], 1)


def test_ops_scoring_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from lit_gpt import ops

    x = torch.zeros(2, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.token_logprobs(x, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="targets"):
        ops.token_logprobs(x, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="shapes differ"):
        ops.logits_kl(x, torch.zeros(2, 9, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="bf16 or fp32"):
        ops.token_logprobs(x.half(), torch.zeros(2, dtype=torch.int32))
