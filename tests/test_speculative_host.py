"""Host-side logic of greedy speculative decoding (no GPU): the n-gram drafter, the round loop on a stub executor,
the command line of generate/speculative.py, and the two new ops refusing CPU tensors."""

import pytest
import torch


def test_ngram_drafter_proposals():
    from generate.speculative import NgramDrafter

    d = NgramDrafter(3)
    # the longest suffix wins: (7, 8, 9) occurred once, followed by 1, 2; the shorter suffix (9,) also precedes 5
    seq = [7, 8, 9, 1, 2, 3, 9, 5, 6, 7, 8, 9]
    assert d.propose(seq, 2) == [1, 2]
    assert d.propose(seq, 1) == [1]
    # the most recent match wins: (4, 5) was followed by 6, later by 7
    assert d.propose([4, 5, 6, 0, 4, 5, 7, 0, 1, 4, 5], 3) == [7, 0, 1]
    # falls back to shorter suffixes, down to one token
    assert d.propose([1, 2, 3, 9, 9, 4, 3], 2) == [9, 9]
    # no match proposes nothing
    assert d.propose([1, 2, 3, 4], 3) == []
    assert d.propose([5], 3) == []
    # a proposal never reads past the sequence: only the tokens that exist after the match
    assert d.propose([1, 2, 3, 1, 2], 7) == [3, 1, 2]
    assert d.propose([6, 6], 5) == [6]
    assert d.propose([1, 2, 1], 0) == []
    assert NgramDrafter(1).propose([1, 2, 3, 1, 2, 9, 2], 2) == [9, 2]
    with pytest.raises(ValueError):
        NgramDrafter(0)


class _StubExecutor:
    """Plays the target model: it knows the true continuation and accepts the matching prefix of the drafts, or a
    scripted count when one is queued."""

    def __init__(self, truth, start, scripted=None):
        self.truth, self.p = truth, start  # truth[p] is the token the model emits after position p - 1
        self.scripted = list(scripted or [])
        self.calls = []

    def step(self, drafts):
        drafts = list(drafts)
        self.calls.append(len(drafts))
        a = 0
        while a < len(drafts) and drafts[a] == self.truth[self.p + a]:
            a += 1
        if self.scripted:
            a = min(a, self.scripted.pop(0))
        new = self.truth[self.p:self.p + a + 1]
        self.p += a + 1
        return a, new


class _Oracle:
    def __init__(self, truth, give=None):
        self.truth, self.give, self.asked = truth, give, []

    def propose(self, tokens, k):
        self.asked.append(k)
        n = k if self.give is None else self.give
        return self.truth[len(tokens):len(tokens) + n]


def test_round_loop_budget_trimming_eos_and_statistics():
    from generate.speculative import speculative_rounds

    truth = list(range(100, 200))
    T = 10  # tokens[:T + 1] = prompt + the prefill's token; the last emitted token sits at position T
    tokens = truth[:T + 1]

    # the budget: 23 steps at gamma 3 -> 6 rounds, the last asks for 23 - 20 - 1 = 2 drafts
    ex, dr, stats = _StubExecutor(truth, T + 1), _Oracle(truth), {}
    out = speculative_rounds(ex, dr, tokens, 23, 1000, 3, None, stats)
    assert out == truth[T + 1:T + 24]
    assert dr.asked == [3, 3, 3, 3, 3, 2] and ex.calls == dr.asked
    assert stats == {"rounds": 6, "proposed": 17, "accepted": 17, "tokens": 23}

    # nothing accepted: one token per round, `steps` rounds; the last round asks for no draft at all
    ex, dr, stats = _StubExecutor(truth, T + 1, scripted=[0] * 23), _Oracle(truth), {}
    assert speculative_rounds(ex, dr, tokens, 23, 1000, 7, None, stats) == truth[T + 1:T + 24]
    assert stats["rounds"] == 23 and stats["accepted"] == 0 and dr.asked[-1] == 1 and ex.calls[-1] == 0

    # the cache end: 14 rows, the last emitted token goes to row 10 -> a window may reach row 13: 3 drafts, though
    # gamma and the budget would allow 5; no later round asks for a draft past the cache
    ex, dr, stats = _StubExecutor(truth, T + 1), _Oracle(truth), {}
    out = speculative_rounds(ex, dr, tokens, 6, 14, 7, None, stats)
    assert out == truth[T + 1:T + 7] and ex.calls == [3, 0, 0] and dr.asked == [3]

    # a drafter that proposes more than asked is cut; one that proposes nothing gives one-row rounds
    ex, dr = _StubExecutor(truth, T + 1), _Oracle(truth, give=9)
    assert speculative_rounds(ex, dr, tokens, 8, 1000, 3) == truth[T + 1:T + 9] and ex.calls == [3, 3]
    ex, dr, stats = _StubExecutor(truth, T + 1), _Oracle(truth, give=0), {}
    assert speculative_rounds(ex, dr, tokens, 5, 1000, 3, None, stats) == truth[T + 1:T + 6]
    assert stats == {"rounds": 5, "proposed": 0, "accepted": 0, "tokens": 5}

    # eos: tokens after the first eos are dropped and the loop stops; the statistics count what was kept
    eos = truth[T + 6]
    ex, dr, stats = _StubExecutor(truth, T + 1), _Oracle(truth), {}
    out = speculative_rounds(ex, dr, tokens, 23, 1000, 3, eos, stats)
    assert out == truth[T + 1:T + 7] and out[-1] == eos
    assert stats["rounds"] == 2 and stats["tokens"] == 6
    # statistics accumulate across calls
    speculative_rounds(_StubExecutor(truth, T + 1), _Oracle(truth), tokens, 4, 1000, 3, None, stats)
    assert stats["rounds"] == 3 and stats["tokens"] == 10


def test_scripted_drafter_corrupts_on_schedule():
    from generate.speculative import ScriptedDrafter

    ref = list(range(50))
    d = ScriptedDrafter(ref, lambda rnd, i: rnd == 1 and i == 2, 50)
    d.begin(None, 0)
    assert d.propose(ref[:10], 4) == [10, 11, 12, 13]
    assert d.propose(ref[:20], 4) == [20, 21, 23, 23]
    assert d.propose(ref[:48], 4) == [48, 49]


def test_command_line_flags(capsys):
    from generate import speculative as sp

    a = sp.parse_args(["--synthetic", "Llama-2-7b-hf", "--quantize", "nf4", "--draft", "ngram", "--speculate", "5",
                       "--max_new_tokens", "33", "--prompt", "hi", "--precision", "bf16-true"])
    assert (a.synthetic, a.quantize, a.draft, a.speculate, a.max_new_tokens, a.prompt, a.precision) == (
        "Llama-2-7b-hf", "nf4", "ngram", 5, 33, "hi", "bf16-true")
    a = sp.parse_args(["--checkpoint_dir", "ckpt/a", "--draft_checkpoint_dir", "ckpt/b", "--draft_quantize", "nf4"])
    assert str(a.checkpoint_dir) == "ckpt/a" and str(a.draft_checkpoint_dir) == "ckpt/b"
    assert a.draft_quantize == "nf4" and a.speculate == sp.DEFAULT_SPECULATE and a.draft is None
    a = sp.parse_args(["--draft_synthetic", "Llama-2-7b-hf"])
    assert a.draft_synthetic == "Llama-2-7b-hf" and a.quantize == "int4-g128"
    assert 1 <= sp.DEFAULT_SPECULATE <= sp.GPT.MAX_WINDOW - 1
    for bad in ([], ["--draft", "ngram", "--draft_synthetic", "x"], ["--draft", "lookup"],
                ["--draft", "ngram", "--speculate", "0"], ["--draft", "ngram", "--speculate", str(sp.GPT.MAX_WINDOW)],
                ["--draft", "ngram", "--temperature", "0.8"]):
        with pytest.raises(SystemExit):
            sp.parse_args(bad)
    capsys.readouterr()


def test_generate_speculative_refuses_before_any_launch():
    from generate.speculative import NgramDrafter, generate_speculative

    prompt = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="greedy only"):
        generate_speculative(None, prompt, 8, NgramDrafter(), temperature=0.7)
    with pytest.raises(ValueError, match="speculate"):
        generate_speculative(None, prompt, 8, NgramDrafter(), speculate=0)


def test_new_ops_refuse_cpu_tensors():
    from lit_gpt import ops

    H, G, hs = 2, 2, 128
    qkv = torch.zeros(2, (H + 2 * G) * hs, dtype=torch.bfloat16)
    kc = torch.zeros(G, 16, hs, dtype=torch.bfloat16)
    cos = torch.zeros(16, hs)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.attention_decode_window(qkv, kc, kc.clone(), torch.zeros(1, dtype=torch.int64), cos, cos, H, G, hs, hs,
                                    0.1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.spec_accept(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32))
    assert "lga_attention_decode_window" in ops.SIGNATURES and "lga_spec_accept" in ops.SIGNATURES
