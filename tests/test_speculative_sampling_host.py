"""Host-side logic of speculative decoding under top-k sampling (no GPU): the command line, the host twin of the
device sampler's uniform, a host model of the algorithm (sequential sampling == speculative rounds, whatever the
drafts), and the draw numbers ``ModelDrafter`` hands its coupled draft model."""

import numpy as np
import pytest
import torch

from oracle import model as om


def test_command_line_accepts_sampling_only_with_top_k(capsys):
    from generate import speculative as sp

    a = sp.parse_args(["--draft", "ngram", "--temperature", "0.8", "--top_k", "200"])
    assert a.temperature == 0.8 and a.top_k == 200
    a = sp.parse_args(["--draft", "ngram"])
    assert a.temperature == 0.0 and a.top_k is None
    for bad in (["--draft", "ngram", "--temperature", "0.8", "--top_k", "0"],
                ["--draft", "ngram", "--temperature", "0.8", "--top_k", "2000"],
                ["--draft", "ngram", "--top_k", "0"], ["--draft", "ngram", "--top_k", "2000"],
                ["--draft", "ngram", "--temperature", "0.8"]):
        with pytest.raises(SystemExit):
            sp.parse_args(bad)
    capsys.readouterr()


def test_generate_speculative_refuses_bad_top_k_before_the_model():
    from generate.speculative import NgramDrafter, generate_speculative

    prompt = torch.zeros(4, dtype=torch.int32)
    for top_k in (None, 0, 2000):
        with pytest.raises(NotImplementedError, match="top_k"):
            generate_speculative(None, prompt, 8, NgramDrafter(), temperature=0.8, top_k=top_k)


# (seed, n) -> mix64(seed ^ n * 0xD1B54A32D192ED03) >> 41, computed once from the formula in uint64 arithmetic
# ((0, 0): splitmix64's first output from state 0, 0xE220A8397B1DCDAF, shifted)
KNOWN = {(0, 0): 7409748, (1234, 0): 6129275, (1234, 1): 4638175, (1234, 41): 2343618, (2**62 - 1, 7): 7680919,
         (99, 2**32 + 5): 3932917, (2**64 - 1, 2**40): 8096748}


def test_sampler_uniform():
    from lit_gpt import ops

    for (seed, n), m in KNOWN.items():
        assert ops.sampler_uniform(seed, n) == (m + 0.5) * 2.0**-23
    rs = np.random.RandomState(0)
    for _ in range(200):
        seed, n = int(rs.randint(0, 2**62, dtype=np.int64)), int(rs.randint(0, 2**40, dtype=np.int64))
        u = ops.sampler_uniform(seed, n)
        assert 0.0 < u < 1.0
        assert float(np.float32(u)) == u  # 24 significant bits: exact in fp32
    assert ops.sampler_uniform(5, 3) != ops.sampler_uniform(5, 4) != ops.sampler_uniform(6, 4)
    assert ops.sampler_uniform(-1, 0) == ops.sampler_uniform(2**64 - 1, 0)  # the seed wraps to 64 bits


V, TOP_K, TEMP, SEED = 64, 8, 0.8, 4242


def _row(prefix):
    """Made-up target logits after ``prefix``: a function of the whole prefix, as a model's are."""
    h = 0
    for t in prefix:
        h = (h * 1000003 + int(t) + 1) % (2**31 - 1)
    g = torch.Generator().manual_seed(h)
    return (torch.randn(V, generator=g) * 3.0).to(torch.bfloat16)


def _draw(prefix, n):
    from lit_gpt import ops

    return om.sample_topk_spec(_row(prefix), TOP_K, TEMP, ops.sampler_uniform(SEED, n))[2]


class _SamplingExecutor:
    """WindowDecodeGraph's contract on the host: row r of the window is sampled with draw number counter + r, draft r
    is accepted iff it equals that sample, the counter advances by the tokens emitted."""

    def __init__(self, seq, counter):
        self.seq, self.counter = list(seq), counter
        self.T = len(self.seq) - counter  # the prompt's length
        self.counters, self.generated = [], []

    def step(self, drafts):
        window = [self.seq[-1]] + list(drafts)
        t = [_draw(self.seq + window[1:r + 1], self.counter + r) for r in range(len(window))]
        a = 0
        while a < len(window) - 1 and window[a + 1] == t[a]:
            a += 1
        new = t[:a + 1]
        self.seq.extend(new)
        self.counter += a + 1
        self.counters.append(self.counter)
        self.generated.append(len(self.seq) - self.T)
        return a, new


class _PatternDrafter:
    """Proposes the true continuation with the drafts ``wrong(round, index)`` marks replaced."""

    def __init__(self, truth, wrong):
        self.truth, self.wrong, self.round = truth, wrong, 0

    def propose(self, tokens, k):
        L = len(tokens)
        out = [(t + 1) % V if self.wrong(self.round, i) else t for i, t in enumerate(self.truth[L:L + k])]
        self.round += 1
        return out


def test_speculative_rounds_emit_the_sequential_samples():
    from generate.speculative import speculative_rounds

    prompt = [3, 1, 4, 1, 5]
    T, steps = len(prompt), 30
    truth = list(prompt)
    for n in range(steps + 1):  # sequential sampling: the n-th generated token is draw n (0: the prefill's)
        truth.append(_draw(truth, n))
    assert len(set(truth[T:])) > 5
    patterns = {"never": lambda rnd, i: False, "always": lambda rnd, i: True, "first": lambda rnd, i: i == 0,
                "third": lambda rnd, i: i == 2, "mixed": lambda rnd, i: (rnd + i) % 3 == 2,
                "late": lambda rnd, i: rnd >= 3}
    for gamma in (1, 3, 7):
        for name, wrong in patterns.items():
            ex = _SamplingExecutor(truth[:T + 1], counter=1)  # the prefill's token spent draw 0
            stats = {}
            out = speculative_rounds(ex, _PatternDrafter(truth, wrong), truth[:T + 1], steps, 1000, gamma, None, stats)
            assert out == truth[T + 1:], (gamma, name)
            # the counter after each round is the number of tokens generated (the prefill's included)
            assert ex.counters == ex.generated and ex.counters[-1] == steps + 1
            if name == "never":
                assert stats["accepted"] == stats["proposed"] and stats["rounds"] == -(-steps // (gamma + 1))
            if name == "always":
                assert stats["accepted"] == 0 and stats["rounds"] == steps


class _StubModel:
    max_seq_length = 64

    def __call__(self, *a, **kw):
        return None


def test_model_drafter_draw_numbers(monkeypatch):
    """Draft i of a round that starts after n generated tokens uses draw n + i — also in the round after a fully
    accepted one, whose catch-up step draws (and advances the counter) before draft 0."""
    import lit_gpt.runtime as rt
    from generate.speculative import ModelDrafter

    log = []

    class _Graph:
        def __init__(self, model, first, pos, *, temperature=0.0, top_k=None, rng=None):
            self.rng, self.setting = rng, (temperature, top_k)
            self.token = torch.zeros(1, 1, dtype=torch.int32)
            self.pos = pos
            self._draw()

        def _draw(self):
            log.append((self.pos, None if self.rng is None else int(self.rng.counter)))
            if self.rng is not None:
                self.rng.counter += 1
            self.pos += 1

        def reset(self, token, pos):
            self.pos = pos

        def step(self):
            self._draw()
            return self.token

    monkeypatch.setattr(rt, "DecodeGraph", _Graph)
    T = 6
    prompt = torch.arange(T, dtype=torch.int32)
    d = ModelDrafter(_StubModel(), coupled=True)
    d.set_sampling(0.8, 200, 77)
    d.begin(prompt, 9)
    assert d.rng.seed == 77 and d.dg is None
    seq = list(range(T)) + [9]  # one token generated (draw 0, the prefill's): the drafts use draws 1, 2, 3
    assert len(d.propose(seq, 3)) == 3
    assert d.dg.setting == (0.8, 200)
    assert log == [(T, 1), (T + 1, 2), (T + 2, 3)]
    # the round was fully accepted: 4 tokens emitted. The catch-up step runs the last draft's position (and draws);
    # the drafts of this round are generated tokens 5, 6, 7
    log.clear()
    seq += [1, 2, 3, 4]
    d.propose(seq, 3)
    assert [p for p, _ in log] == [T + 3, T + 4, T + 5, T + 6]
    assert [c for _, c in log[1:]] == [5, 6, 7]
    # one draft accepted, then the target's token: 2 more generated (7 in all); no catch-up, draws 7, 8
    log.clear()
    seq += [5, 6]
    d.propose(seq, 2)
    assert log == [(T + 6, 7), (T + 7, 8)]
    # uncoupled, or a greedy run: the draft graph is the greedy one and no counter exists
    for drafter, setting in ((ModelDrafter(_StubModel(), coupled=False), (0.8, 200, 77)),
                             (ModelDrafter(_StubModel()), (0.0, None, 0))):
        log.clear()
        drafter.set_sampling(*setting)
        drafter.begin(prompt, 9)
        drafter.propose(list(range(T)) + [9], 2)
        assert drafter.rng is None and drafter.dg.setting == (0.0, None)
        assert log == [(T, None), (T + 1, None)]
