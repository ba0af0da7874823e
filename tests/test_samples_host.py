"""CPU tests of the host logic of ``generate_samples`` (n samples of one prompt): its refusals on a fake model, the one
prefill it runs for any number of samples (fake model, scripted step executor), the ``--share_prompt`` flag, and the
new entry point in the header and the built library. No kernel runs."""

import ctypes
import re
import types
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


def _fake_model(max_seq_length=64, dtype=torch.bfloat16, vocab=1000, batch_check=None):
    """What generate_samples reads before it touches the GPU; any forward is a test failure."""

    def forward(*a, **k):
        raise AssertionError("the fake model must not run")

    def _batch_check(B):
        if batch_check is not None:
            raise NotImplementedError(batch_check)

    wte = types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype))
    return types.SimpleNamespace(max_seq_length=max_seq_length, config=types.SimpleNamespace(padded_vocab_size=vocab),
                                 transformer=types.SimpleNamespace(wte=wte), __call__=forward, forward=forward,
                                 _batch_check=_batch_check)


def _prompt(n):
    return torch.arange(n, dtype=torch.int32)


def test_generate_samples_refusals():
    from generate.base import generate_samples

    m = _fake_model()
    for n in (0, -1):
        with pytest.raises(ValueError, match="num_samples"):
            generate_samples(m, _prompt(3), 4, n, temperature=0.0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        generate_samples(m, _prompt(3), 0, 2, temperature=0.0)
    with pytest.raises(ValueError, match="2 seeds for 3 samples"):
        generate_samples(m, _prompt(3), 4, 3, temperature=0.8, top_k=50, seeds=[1, 2])
    with pytest.raises(ValueError, match="share"):
        generate_samples(m, _prompt(3), 4, 3, temperature=0.0, share="yes")
    with pytest.raises(NotImplementedError, match="waves of 5"):
        generate_samples(m, _prompt(3), 4, 6, temperature=0.0, wave=5)
    # the reference's wording (generate/base.py): 40 + 30 - 1 = 69 > 64
    with pytest.raises(NotImplementedError, match="max_seq_length 64 needs to be >= 69"):
        generate_samples(m, _prompt(40), 30, 2, temperature=0.0)
    # sampling settings the device sampler does not take: no top_k, top_k > 1024, fp32 logits, a vocabulary > 65536
    for kw, model in (({"top_k": None}, m), ({"top_k": 2000}, m), ({"top_k": 50}, _fake_model(dtype=torch.float32)),
                      ({"top_k": 50}, _fake_model(vocab=70000))):
        with pytest.raises(NotImplementedError, match="device sampler"):
            generate_samples(model, _prompt(3), 4, 2, temperature=0.8, **kw)
    # a model the batched step does not cover: GPT._batch_check's refusal, before any launch
    with pytest.raises(NotImplementedError, match="plain 4-bit Linears"):
        generate_samples(_fake_model(batch_check="plain 4-bit Linears only"), _prompt(3), 4, 2, temperature=0.0)
    # adapters are out of scope
    lora = _fake_model()
    lora.lora_adapters = object()
    with pytest.raises(NotImplementedError, match="adapter"):
        generate_samples(lora, _prompt(3), 4, 2, temperature=0.0)


class _CountingModel:
    """A model stand-in that counts its prefills (T > 1 forwards); a one-token forward is a test failure."""

    max_seq_length = 64
    config = types.SimpleNamespace(padded_vocab_size=16)
    MAX_BATCH = 4

    def __init__(self, fp8=False):
        self.prefills, self.slots, self.set_calls = 0, [], []
        kv = types.SimpleNamespace(k=torch.zeros(1, 1, 64, 8), v=torch.zeros(1, 1, 64, 8), fp8=fp8, cache_dtype=None)
        attn = types.SimpleNamespace(kv_cache=kv, batch_fusable=lambda dtype: True)
        self.transformer = types.SimpleNamespace(wte=types.SimpleNamespace(weight=torch.zeros(1, dtype=torch.bfloat16)),
                                                 h=[types.SimpleNamespace(attn=attn)])

    def _batch_check(self, B):
        assert B <= self.MAX_BATCH

    def set_kv_cache(self, batch_size, device=None, dtype=None):
        self.set_calls.append(batch_size)
        kv = self.transformer.h[0].attn.kv_cache
        kv.k = torch.zeros(batch_size, 1, 64, 8)
        kv.v = torch.zeros(batch_size, 1, 64, 8)

    def __call__(self, idx, input_pos, **kw):
        assert idx.shape[1] > 1, "decode steps belong to the step executor"
        self.prefills += 1
        self.slots.append(kw.get("kv_slot"))
        return torch.zeros(1, 1, 16)


@pytest.mark.parametrize("share", [True, False])
def test_six_samples_cost_one_prefill(monkeypatch, share):
    from generate import base
    from lit_gpt import runtime

    waves = []

    class Steps:
        chunk = 1

        def __init__(self, model, first_tokens, first_pos, chunk=1, *, shared_prefix=None, rngs=None, **kw):
            self.B = first_tokens.numel()
            self.token = first_tokens.to(torch.int32) + 1
            waves.append((self.B, list(first_pos), None if shared_prefix is None else int(shared_prefix),
                          None if rngs is None else [r.seed for r in rngs]))

        def step(self):
            self.token = self.token + 1
            return self.token

    monkeypatch.setattr(runtime, "BatchDecodeGraph", Steps)
    monkeypatch.setattr(base, "sample", lambda logits, rng=None, **kw: torch.tensor([0 if rng is None else rng.seed]))
    model = _CountingModel()
    seeds = [3, 1, 4, 1, 5, 9]
    outs = base.generate_samples(model, _prompt(7), 5, 6, temperature=0.8, top_k=50, seeds=seeds, share=share)
    assert model.prefills == 1 and model.slots == [0] and model.set_calls == [4]
    assert [w[0] for w in waves] == [4, 2] and all(w[1] == [7] * w[0] for w in waves)
    assert [w[2] for w in waves] == ([7, 7] if share else [None, None])
    assert waves[0][3] == seeds[:4] and waves[1][3] == seeds[4:]  # sample i keeps its own seed in every wave
    assert len(outs) == 6
    for y, s in zip(outs, seeds):  # prompt, the first token drawn with the sample's seed, then the wave's steps
        assert y.tolist() == list(range(7)) + [s, s + 1, s + 2, s + 3, s + 4]
    if not share:  # the copy route put the prompt's rows into the other slots
        assert model.transformer.h[0].attn.kv_cache.k.shape[0] == 4


def test_share_true_refuses_an_fp8_cache_before_any_forward():
    from generate import base

    model = _CountingModel(fp8=True)
    with pytest.raises(NotImplementedError, match="bf16 KV cache"):
        base.generate_samples(model, _prompt(7), 5, 3, temperature=0.0, share=True)
    assert model.prefills == 0


def test_share_prompt_flag(monkeypatch):
    from generate import base

    seen = {}
    monkeypatch.setattr(base, "main", lambda prompt, **kw: seen.update(kw, prompt=prompt))
    base._cli(["--batch_size", "4", "--num_samples", "6", "--share_prompt", "--synthetic", "Llama-2-7b-hf"])
    assert seen["share_prompt"] is True and seen["batch_size"] == 4 and seen["num_samples"] == 6
    base._cli(["--batch_size", "4"])
    assert seen["share_prompt"] is False  # the default: today's run


def test_main_refuses_share_prompt_without_a_batch_or_with_a_prompts_file(tmp_path):
    from generate import base

    with pytest.raises(ValueError, match="--batch_size > 1"):
        base.main(share_prompt=True, batch_size=1)  # refused before the device or the checkpoint is looked at
    f = tmp_path / "prompts.txt"
    f.write_text("4\n5\n")
    with pytest.raises(ValueError, match="--prompts_file"):
        base.main(share_prompt=True, batch_size=2, prompts_file=f)


def test_shared_entry_point_is_declared_and_exported():
    from lit_gpt import ops

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "litgpt_amd.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+lga_attention_decode_shared\s*\(", text)
    assert "lga_attention_decode_shared" in ops.SIGNATURES
    assert ops.LIB_PATH.is_file(), "build the library first (__graft_entry__.build)"
    lib = ctypes.CDLL(str(ops.LIB_PATH))
    assert hasattr(lib, "lga_attention_decode_shared")
    # the argument checks run without a GPU: nothing is launched on a refusal
    lib.lga_last_error_string.restype = ctypes.c_char_p
    f = lib.lga_attention_decode_shared
    f.argtypes = ops.SIGNATURES["lga_attention_decode_shared"]
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    G, S, HS = 2, 16, 128
    assert f(p, p, p, p, None, p, p, S, p, None, None, 2, G * S * HS, None, 4, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"null" in lib.lga_last_error_string()
    for B in (0, 9):
        assert f(p, p, p, p, p, p, p, S, p, None, None, B, G * S * HS, None, 4, G, HS, HS, S, 1, 0.1, None) != 0
        assert b"B must be in [1, 8]" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, p, S, p, None, None, 2, G * S * HS - 1, None, 4, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"slot_stride" in lib.lga_last_error_string()


def test_shared_kernels_use_no_scratch():
    """Rows per workgroup are chosen among the values that compile with no scratch: every instantiation
    of the new kernel in the built library has no private segment and spills no VGPR."""
    from lit_gpt import ops
    from test_native_library import _kernel_scratch

    assert ops.LIB_PATH.is_file(), "build the library first (__graft_entry__.build)"
    shared = {k: v for k, v in _kernel_scratch(ops.LIB_PATH).items() if "attn_shared_kernel" in k}
    assert len(shared) == 5, sorted(shared)
    assert not {k: v for k, v in shared.items() if v[0] or v[1]}
