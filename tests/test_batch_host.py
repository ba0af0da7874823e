"""CPU tests of the batched decode's host logic: ``generate_batch`` argument validation on a fake model, the eos
bookkeeping of its step loop on a stub executor that returns scripted token columns, the ``--batch_size`` flag, and the
two rows ops refusing CPU tensors. No kernel runs."""

import types

import pytest
import torch


def _fake_model(max_seq_length=64, dtype=torch.bfloat16, vocab=1000):
    """What generate_batch reads before it touches the GPU; any forward is a test failure."""

    def forward(*a, **k):
        raise AssertionError("the fake model must not run")

    wte = types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype))
    return types.SimpleNamespace(max_seq_length=max_seq_length, config=types.SimpleNamespace(padded_vocab_size=vocab),
                                 transformer=types.SimpleNamespace(wte=wte), __call__=forward, forward=forward)


def _prompt(n):
    return torch.arange(n, dtype=torch.int32)


def test_generate_batch_argument_validation():
    from generate.base import generate_batch

    m = _fake_model()
    with pytest.raises(ValueError, match="no prompts"):
        generate_batch(m, [], 4)
    for n in (5, 9):  # more than MAX_BATCH = 4 (the kernels' 8 rows are not the batch limit)
        with pytest.raises(NotImplementedError, match="at most 4"):
            generate_batch(m, [_prompt(3)] * n, 4, temperature=0.0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        generate_batch(m, [_prompt(3)] * 2, 0, temperature=0.0)
    with pytest.raises(ValueError, match="seeds"):
        generate_batch(m, [_prompt(3)] * 2, 4, temperature=0.8, top_k=50, seeds=[1])
    # the reference's wording (generate/base.py), on the longest prompt: 40 + 30 - 1 = 69 > 64
    with pytest.raises(NotImplementedError, match="max_seq_length 64 needs to be >= 69"):
        generate_batch(m, [_prompt(5), _prompt(40)], 30, temperature=0.0)
    # sampling settings the device sampler does not take: no top_k, top_k > 1024, fp32 logits, a vocabulary > 65536
    for kw, model in (({"top_k": None}, m), ({"top_k": 2000}, m), ({"top_k": 50}, _fake_model(dtype=torch.float32)),
                      ({"top_k": 50}, _fake_model(vocab=70000))):
        with pytest.raises(NotImplementedError, match="device sampler"):
            generate_batch(model, [_prompt(3)] * 2, 4, temperature=0.8, **kw)


class ScriptedSteps:
    """A step executor that replays scripted token columns: ``script`` (n_steps, B); row 0 is already in ``token``."""

    def __init__(self, script, chunk=1):
        self.script = torch.tensor(script, dtype=torch.int64)
        self.B, self.chunk = self.script.shape[1], chunk
        self.token = self.script[0].to(torch.int32)
        self.at, self.launches = 1, 0

    def step(self):
        self.launches += 1
        self.at += 1
        return self.script[self.at - 1].to(torch.int32)

    def steps(self):
        self.launches += 1
        self.at += self.chunk
        return self.script[self.at - self.chunk:self.at]


def _script(n, B, eos_at):
    """Tokens 100 + step everywhere, 7 (the eos) at (step, sequence) of ``eos_at``."""
    s = [[100 + i] * B for i in range(n)]
    for i, b in eos_at:
        s[i][b] = 7
    return s


@pytest.mark.parametrize("chunk", [1, 4])
def test_batch_steps_eos_bookkeeping(chunk):
    from generate.base import _batch_steps

    n = 11
    # no eos id: every sequence collects every step
    dg = ScriptedSteps(_script(n, 3, [(2, 0)]), chunk)
    out, lengths = _batch_steps(dg, n, None)
    assert lengths == [n] * 3 and out.tolist() == dg.script.tolist()
    # sequence 1 meets the eos at step 3 (and again at 6: only the first counts), sequence 0 never, sequence 2 at 9
    dg = ScriptedSteps(_script(n, 3, [(3, 1), (6, 1), (9, 2)]), chunk)
    out, lengths = _batch_steps(dg, n, 7)
    assert lengths == [n, 4, 10]
    assert out[:4, 1].tolist() == [100, 101, 102, 7] and out[:, 0].tolist() == [100 + i for i in range(n)]
    assert dg.at == n  # one sequence still open: the batch stepped to the end
    # all sequences done early: the loop stops after the launch that finished the last one
    dg = ScriptedSteps(_script(n, 2, [(0, 0), (2, 1)]), chunk)
    out, lengths = _batch_steps(dg, n, 7)
    assert lengths == [1, 3]
    assert dg.at == (3 if chunk == 1 else 5) and dg.launches == (2 if chunk == 1 else 1)
    # the first step's tokens (already in ``token``) are tested too
    dg = ScriptedSteps(_script(n, 1, [(0, 0)]), chunk)
    out, lengths = _batch_steps(dg, n, 7)
    assert lengths == [1] and dg.launches == 0


def test_batch_size_flag_reaches_main(monkeypatch):
    from generate import base

    seen = {}
    monkeypatch.setattr(base, "main", lambda prompt, **kw: seen.update(kw, prompt=prompt))
    base._cli(["--batch_size", "4", "--num_samples", "6", "--synthetic", "Llama-2-7b-hf"])
    assert seen["batch_size"] == 4 and seen["num_samples"] == 6
    base._cli([])
    assert seen["batch_size"] == 1  # the default: today's one-sequence run


def test_main_refuses_a_batch_size_out_of_range():
    from generate import base

    for b in (0, 9):
        with pytest.raises(NotImplementedError, match="batch_size"):
            base.main(batch_size=b)  # refused before the device or the checkpoint is looked at


def test_rows_ops_refuse_cpu_tensors():
    from lit_gpt import ops

    N, K = 64, 256
    x = torch.zeros(2, K, dtype=torch.bfloat16)
    qw = torch.zeros(N, K // 2, dtype=torch.uint8)
    sc = torch.zeros(N, K // 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.q4_gemv_rows(x, qw, sc, N, K, 128, ops.FMT_Q4G, out=torch.empty(2, N, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.q4_gemv_swiglu_rows(x, qw, sc, qw, sc, N, K, 128, ops.FMT_Q4G, out=torch.empty(2, N, dtype=torch.bfloat16))
    # shape and range checks come first and need no GPU either
    with pytest.raises(ValueError, match="1..8"):
        ops.q4_gemv_rows(torch.zeros(9, K, dtype=torch.bfloat16), qw, sc, N, K, 128, ops.FMT_Q4G)
    with pytest.raises(ValueError, match="fmt"):
        ops.q4_gemv_swiglu_rows(x, qw, sc, qw, sc, N, K, 128, ops.FMT_BF16)


def test_non_four_bit_linears_refuse_the_rows_route():
    """The rows route of a Linear without the kernel names the supported modes (no launch is attempted)."""
    from lit_gpt import quantize

    for kernels in (quantize.Int8Linear.gemv_rows, quantize._Kernels.gemv_rows):
        holder = types.SimpleNamespace(kind="Int8Linear")
        with pytest.raises(NotImplementedError, match="int4-g128/64/32, nf4, bnb.nf4, bnb.nf4-dq, bnb.fp4, bnb.fp4-dq"):
            kernels(holder, None, None, None, 1e-5)
