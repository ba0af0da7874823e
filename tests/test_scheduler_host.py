"""CPU tests of continuous batching's host side: ``lit_gpt.scheduler.SlotScheduler`` driven by a scripted fake
executor (every prompt has a scripted token stream; the executor hands out, per launch, what each slot's sequence would
produce next — and junk for idle slots and past a sequence's end), and ``generate_continuous``'s refusals on a fake
model. No kernel runs, no tensor sits on a device."""

import types

import pytest
import torch

EOS = 99


def _stream(i, n=64):
    """Prompt i's scripted decode tokens: distinct per prompt and step, never EOS."""
    return [1000 * (i + 1) + s for s in range(n)]


class FakeExecutor:
    """Slots hold (prompt, next step); a launch returns n rows of B tokens and advances every filled slot by n —
    also past the point where the scheduler stopped collecting (the overshoot it must drop)."""

    def __init__(self, B, streams):
        self.B, self.streams = B, streams
        self.slot = [None] * B  # [prompt index, next step] or None
        self.launches = []

    def fill(self, b, i):
        self.slot[b] = [i, 0]

    def release(self, b):
        self.slot[b] = None

    def run(self, n):
        self.launches.append(n)
        rows = []
        for _ in range(n):
            row = []
            for b in range(self.B):
                if self.slot[b] is None:
                    row.append(-7)  # an idle slot's junk
                else:
                    i, s = self.slot[b]
                    row.append(self.streams[i][s])
                    self.slot[b][1] += 1
            rows.append(row)
        return rows


def _drive(sched, streams, trace=None):
    """The engine's loop (generate.base.generate_continuous) on the fake executor."""
    ex = FakeExecutor(sched.n_slots, streams)
    while not sched.done:
        while (fill := sched.next_fill()) is not None:
            b, i = fill
            if sched.start(b):
                ex.fill(b, i)
        if sched.done:
            break
        n = sched.next_launch()
        if trace is not None:
            trace.append((n, list(sched.slot_prompt), list(sched.collected), list(sched.draws)))
        for b in sched.consume(ex.run(n)):
            ex.release(b)
    return ex


def _expected(stream, budget, eos_id=EOS):
    out = []
    for t in stream[:budget - 1]:
        out.append(t)
        if t == eos_id:
            break
    return out


LENS = [5, 16, 33, 9, 21, 3, 12]
BUDGETS = [30, 40, 3, 25, 1, 28, 34]


def _streams_with_eos():
    streams = [_stream(i) for i in range(len(LENS))]
    streams[1][12] = EOS  # prompt 1 ends at its 13th decode token, inside a chunk
    streams[1][14] = EOS  # (a second eos past the end must not matter)
    streams[3][0] = EOS   # prompt 3 ends at its first decode token
    streams[5][40] = EOS  # past prompt 5's budget: never seen
    return streams


@pytest.mark.parametrize("chunk", [1, 8])
def test_seven_prompts_three_slots(chunk):
    from lit_gpt.scheduler import SlotScheduler

    streams = _streams_with_eos()
    sched = SlotScheduler(LENS, BUDGETS, 3, chunk=chunk, eos_id=EOS)
    trace = []
    ex = _drive(sched, streams, trace)
    res = sched.results()
    assert len(res) == 7
    for i in range(7):  # prompt order; truncation at the first eos inclusive and at the budget; overshoot dropped
        assert res[i] == _expected(streams[i], BUDGETS[i]), i
    assert res[1][-1] == EOS and len(res[1]) == 13
    assert res[3] == [EOS]
    assert res[4] == []  # a budget of one token: the prefill's, no decode step
    assert len(res[5]) == BUDGETS[5] - 1 and EOS not in res[5]
    assert sorted(i for s in sched.served for i in s) == list(range(7))  # every prompt served exactly once
    assert any(len(s) >= 2 for s in sched.served)
    assert all(n in (1, chunk) for n in ex.launches)
    if chunk == 8:
        assert 8 in ex.launches and 1 in ex.launches
        # prompt 1's eos fell inside a chunk: the slot ran on to the chunk's end, and none of that was kept
        assert any(n == 8 and 1 in owners and 12 - 8 < col[owners.index(1)] < 12 for n, owners, col, _ in trace)
    assert ex.slot == [None, None, None]  # everything released at the end


def test_freed_slot_is_refilled_while_others_keep_their_counts():
    from lit_gpt.scheduler import SlotScheduler

    streams = [_stream(i) for i in range(4)]
    sched = SlotScheduler([4, 4, 4, 4], [3, 10, 10, 5], 3, chunk=1)
    ex = FakeExecutor(3, streams)
    for _ in range(3):
        b, i = sched.next_fill()
        assert sched.start(b)
        ex.fill(b, i)
    assert sched.next_fill() is None  # no free slot
    assert sched.slot_prompt == [0, 1, 2]
    assert sched.consume(ex.run(1)) == []
    freed = sched.consume(ex.run(1))  # prompt 0: budget 3 = prefill + 2 decode tokens
    assert freed == [0]
    ex.release(0)
    assert sched.slot_prompt == [None, 1, 2] and sched.collected[1:] == [2, 2] and sched.draws[1:] == [3, 3]
    assert sched.next_fill() == (0, 3)  # the freed slot takes the next prompt of the queue
    assert sched.start(0)
    ex.fill(0, 3)
    assert sched.slot_prompt == [3, 1, 2]
    assert sched.collected == [0, 2, 2] and sched.draws == [1, 3, 3]  # the others keep theirs
    sched.consume(ex.run(1))
    assert sched.collected == [1, 3, 3]
    assert sched.tokens[3] == streams[3][:1] and sched.tokens[1] == streams[1][:3]


def test_release_when_the_queue_is_empty():
    from lit_gpt.scheduler import SlotScheduler

    streams = [_stream(i) for i in range(2)]
    sched = SlotScheduler([3, 3], [2, 6], 2, chunk=1)
    ex = FakeExecutor(2, streams)
    for _ in range(2):
        b, i = sched.next_fill()
        sched.start(b)
        ex.fill(b, i)
    assert sched.consume(ex.run(1)) == [0]
    ex.release(0)
    assert sched.next_fill() is None  # nothing waits: slot 0 stays idle
    assert sched.active == [False, True] and not sched.done
    while not sched.done:
        for b in sched.consume(ex.run(sched.next_launch())):
            ex.release(b)
    assert sched.results() == [streams[0][:1], streams[1][:5]]  # the idle slot's junk never lands anywhere
    assert all(-7 not in r for r in sched.results())


def test_fewer_prompts_than_slots():
    from lit_gpt.scheduler import SlotScheduler

    streams = [_stream(i) for i in range(2)]
    sched = SlotScheduler([7, 2], 5, 4, chunk=8, eos_id=EOS)
    assert sched.n_slots == 2
    _drive(sched, streams)
    assert sched.results() == [streams[0][:4], streams[1][:4]]


@pytest.mark.parametrize("chunk", [1, 8])
def test_uniforms_follow_the_draw_numbers(chunk):
    from lit_gpt import ops
    from lit_gpt.scheduler import SlotScheduler

    seeds = [11, 22, 33, 44, 55]
    budgets = [12, 4, 30, 9, 17]
    streams = [_stream(i) for i in range(5)]
    sched = SlotScheduler([3] * 5, budgets, 2, chunk=chunk, seeds=seeds)
    ex = FakeExecutor(2, streams)
    seen = {i: [] for i in range(5)}  # per prompt: the uniforms handed out for the tokens it kept
    while not sched.done:
        while (fill := sched.next_fill()) is not None:
            b, i = fill
            if sched.start(b):
                ex.fill(b, i)
                assert sched.draws[b] == 1  # draw 0 went to the prefill's token
        if sched.done:
            break
        n = sched.next_launch()
        u = sched.uniforms(n)
        assert len(u) == n and all(len(r) == 2 for r in u)
        owners, before = list(sched.slot_prompt), list(sched.draws)
        for s in range(n):
            for b, i in enumerate(owners):
                if i is None:
                    assert u[s][b] == 0.5
                else:
                    assert u[s][b] == ops.sampler_uniform(seeds[i], before[b] + s)
                    seen[i].append(u[s][b])
        for b in sched.consume(ex.run(n)):
            ex.release(b)
    for i in range(5):  # the kept token k of prompt i (k = 1 .. budget - 1) was drawn with draw number k
        want = [ops.sampler_uniform(seeds[i], k) for k in range(1, budgets[i])]
        assert seen[i][:budgets[i] - 1] == want
    with pytest.raises(RuntimeError, match="seeds"):
        SlotScheduler([3], 4, 1).uniforms(1)


def test_scheduler_refusals():
    from lit_gpt.scheduler import SlotScheduler

    with pytest.raises(ValueError, match="no prompts"):
        SlotScheduler([], 4, 2)
    with pytest.raises(ValueError, match="max_new_tokens for 2 prompts"):
        SlotScheduler([3, 3], [4], 2)
    with pytest.raises(ValueError, match="at least 1"):
        SlotScheduler([3, 3], [4, 0], 2)
    with pytest.raises(ValueError, match="seeds"):
        SlotScheduler([3, 3], 4, 2, seeds=[1])
    with pytest.raises(NotImplementedError, match="max_seq_length 64 needs to be >= 69"):
        SlotScheduler([5, 40], [8, 30], 2, max_seq_length=64)
    SlotScheduler([5, 40], [8, 25], 2, max_seq_length=64)  # 40 + 25 - 1 = 64 fits


def _fake_model(max_seq_length=64, dtype=torch.bfloat16, vocab=1000):
    """What generate_continuous reads before it touches the GPU; any forward is a test failure."""

    def forward(*a, **k):
        raise AssertionError("the fake model must not run")

    def batch_check(B):
        raise NotImplementedError("batch size > 1 with lm_head a Linear: the multi-row decode GEMV streams plain "
                                  "4-bit Linears only")

    wte = types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype))
    return types.SimpleNamespace(max_seq_length=max_seq_length, config=types.SimpleNamespace(padded_vocab_size=vocab),
                                 transformer=types.SimpleNamespace(wte=wte), __call__=forward, forward=forward,
                                 _batch_check=batch_check)


def _prompt(n):
    return torch.arange(n, dtype=torch.int32)


def test_generate_continuous_refusals():
    from generate.base import MAX_BATCH, generate_continuous

    m = _fake_model()
    with pytest.raises(ValueError, match="no prompts"):
        generate_continuous(m, [], 4)
    with pytest.raises(NotImplementedError, match=f"at most {MAX_BATCH}"):
        generate_continuous(m, [_prompt(3)] * 6, 4, batch_size=MAX_BATCH + 1, temperature=0.0)
    with pytest.raises(ValueError, match="batch_size"):
        generate_continuous(m, [_prompt(3)] * 2, 4, batch_size=0, temperature=0.0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        generate_continuous(m, [_prompt(3)] * 2, 0, temperature=0.0)
    with pytest.raises(ValueError, match="max_new_tokens for 3 prompts"):
        generate_continuous(m, [_prompt(3)] * 3, [4, 4], temperature=0.0)
    with pytest.raises(ValueError, match="seeds"):
        generate_continuous(m, [_prompt(3)] * 2, 4, temperature=0.8, top_k=50, seeds=[1])
    with pytest.raises(NotImplementedError, match="max_seq_length 64 needs to be >= 69"):
        generate_continuous(m, [_prompt(5), _prompt(40), _prompt(2)], [4, 30, 4], batch_size=2, temperature=0.0)
    for kw, model in (({"top_k": None}, m), ({"top_k": 2000}, m), ({"top_k": 50}, _fake_model(dtype=torch.float32)),
                      ({"top_k": 50}, _fake_model(vocab=70000))):
        with pytest.raises(NotImplementedError, match="device sampler"):
            generate_continuous(model, [_prompt(3)] * 3, 4, batch_size=2, temperature=0.8, **kw)
    with pytest.raises(NotImplementedError, match="4-bit"):  # whatever _batch_check refuses, before any launch
        generate_continuous(m, [_prompt(3)] * 3, 4, batch_size=2, temperature=0.0)


def test_prompts_file_flag_parses(monkeypatch, tmp_path):
    """--prompts_file reaches main; without it main gets None (nothing changes)."""
    import generate.base as gb

    got = {}
    monkeypatch.setattr(gb, "main", lambda *a, **k: got.update(k))
    f = tmp_path / "p.txt"
    f.write_text("5\n9\n")
    gb._cli(["--synthetic", "x", "--prompts_file", str(f), "--batch_size", "3"])
    assert got["prompts_file"] == f and got["batch_size"] == 3
    gb._cli(["--synthetic", "x"])
    assert got["prompts_file"] is None
