"""LLaMA-Adapter (v1) without a GPU: the specification (tests/adapter_spec.py) against the reference's own logits (the g7
fixture), ``lit_gpt.adapter.attach``'s key handling, the refusals, generate/adapter.py's argument checks and the
argument validation of the ``lga_adapter_attention`` C entry point (it returns before any launch)."""

import ctypes
import dataclasses
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import adapter_spec as spec

REPO = Path(__file__).resolve().parent.parent
KEYS = ("mha", "gqa")


@pytest.fixture(scope="module")
def g7():
    return np.load(REPO / "tests" / "golden" / "g7_adapter.npz", allow_pickle=False)


def _close(got, want, what):
    """Both sides fp32 evaluations of the same function: within 1e-4 of max |logit| (tests/test_lora_host.py's bound
    for the same kind of comparison)."""
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max error {err / scale:.2e} of the logit scale {scale:.3f}")
    assert err <= 1e-4 * scale, f"{what}: {err / scale:.2e} of the logit scale"


@pytest.mark.parametrize("key", KEYS)
def test_spec_reproduces_the_reference_logits_with_the_adapter(g7, key):
    cfg = spec.adapter_config(key)
    og = spec.AdapterOracle(cfg, spec.fixture_state(key, g7), dtype=torch.float32)
    logits = og.forward(torch.from_numpy(g7[f"{key}/prompt"])).numpy()
    _close(logits, g7[f"{key}/logits_adapter"], f"{key} with the adapter")
    # the condition the generator asserted: the adapter moves the reference's own argmax at 3 or more of the 12 positions
    moved = int((g7[f"{key}/logits_adapter"].argmax(-1) != g7[f"{key}/logits_zero_gating"].argmax(-1)).sum())
    assert g7[f"{key}/prompt"].size == spec.PROMPT == 12 and moved >= spec.MIN_MOVED == 3, moved


@pytest.mark.parametrize("key", KEYS)
def test_spec_with_zero_gating_is_the_plain_oracle_and_the_reference(g7, key):
    from oracle.model import OracleGPT

    cfg = spec.adapter_config(key)
    sd = spec.fixture_state(key, g7)
    zero = {k: (np.zeros_like(v) if "gating_factor" in k else v) for k, v in sd.items()}
    prompt = torch.from_numpy(g7[f"{key}/prompt"])
    got = spec.AdapterOracle(cfg, zero, dtype=torch.float32).forward(prompt)
    plain = OracleGPT(cfg, {k: v for k, v in sd.items() if not spec.is_adapter_key(k)}, dtype=torch.float32)
    assert torch.equal(got, plain.forward(prompt))
    _close(got.numpy(), g7[f"{key}/logits_zero_gating"], f"{key} zero gating")


def test_prefix_attention_spec_helper_agrees_with_a_direct_evaluation():
    """A self-check of the test-side helper ``prefix_attention_spec`` (it exercises no product code): on small bf16
    operands it stays close to a head-by-head float64 evaluation of y + g * softmax(scale * rope(q) ak^T) av without
    any rounding, and it leaves an idle row as it was. The closeness bound, four bf16 steps of the largest element,
    is a sanity margin for the helper's three roundings, not a specification."""
    g = torch.Generator().manual_seed(3)
    H, G, hs, n, aT, T = 4, 2, 16, 8, 5, 3
    bf = spec.bf16_round
    qkv = bf(torch.randn(T, (H + 2 * G) * hs, generator=g, dtype=torch.float64))
    ak, av = (bf(torch.randn(G, aT, hs, generator=g, dtype=torch.float64)) for _ in range(2))
    gating = bf(torch.randn(H, generator=g, dtype=torch.float64))
    y = bf(torch.randn(T, H * hs, generator=g, dtype=torch.float64))
    ang = torch.rand(7, n // 2, generator=g).repeat(1, 2)
    cos, sin = torch.cos(ang), torch.sin(ang)
    pos = torch.tensor([5, 0, 3])
    active = torch.tensor([1, 0, 1], dtype=torch.int32)
    parts = {}
    out = spec.prefix_attention_spec(y, qkv, ak, av, gating, cos, sin, pos, H, G, hs, n, 0.25, active, parts)
    assert torch.equal(out[1], y[1])  # the idle row keeps its bits
    qpk = H // G
    q = qkv.view(T, G, qpk + 2, hs)[:, :, :qpk].reshape(T, H, hs)
    for t in (0, 2):
        for h in range(H):
            x = q[t, h].clone()
            xr = x[:n]
            rot = torch.cat((-xr[n // 2:], xr[:n // 2]))
            x[:n] = xr * cos[pos[t]].double() + rot * sin[pos[t]].double()
            p = torch.softmax(0.25 * (ak[h // qpk] @ x), 0)
            want = y[t, h * hs:(h + 1) * hs] + gating[h] * (p @ av[h // qpk])
            got = out[t, h * hs:(h + 1) * hs]
            assert float((got - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max()) * 4


# ------------------------------------------------------------------------------------------------ attach
def _cpu_model(key):
    from lit_gpt import GPT

    cfg = spec.adapter_config(key)
    return cfg, GPT(cfg).to(torch.bfloat16)


def _tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@pytest.mark.parametrize("layout", ["new", "old"])
@pytest.mark.parametrize("nested", [False, True], ids=["flat", "under-model"])
@pytest.mark.parametrize("key", KEYS)
def test_attach_maps_the_reference_keys(g7, key, nested, layout):
    from lit_gpt import adapter

    cfg, model = _cpu_model(key)
    state = _tensors(spec.fixture_state(key, g7))  # a full checkpoint (base weights too) is accepted
    if layout == "old":  # older checkpoints: (1, n_head, 1, 1)
        state = {k: (v.permute(0, 2, 1, 3).contiguous() if "gating_factor" in k else v) for k, v in state.items()}
        assert state["transformer.h.1.attn.gating_factor"].shape == (1, cfg.n_head, 1, 1)
    out = adapter.attach(model, {"model": state} if nested else state, cfg)
    assert out is model and type(model) is adapter.GPT and model.config is cfg
    for i, blk in enumerate(model.transformer.h):
        assert type(blk) is adapter.Block and type(blk.attn) is adapter.CausalSelfAttention and blk.attn.block_idx == i
        assert blk.attn.adapted == (i >= cfg.adapter_start_layer)
        if i < cfg.adapter_start_layer:
            assert not hasattr(blk.attn, "adapter_wte") and not hasattr(blk.attn, "gating_factor")
            continue
        pre = f"transformer.h.{i}.attn"
        want_w = torch.from_numpy(g7[f"{key}/{pre}.adapter_wte.weight"]).to(torch.bfloat16)
        want_g = torch.from_numpy(g7[f"{key}/{pre}.gating_factor"]).to(torch.bfloat16)
        assert torch.equal(blk.attn.adapter_wte.weight, want_w)
        assert blk.attn.gating_factor.shape == (1, 1, cfg.n_head, 1) and torch.equal(blk.attn.gating_factor, want_g)
        assert blk.attn.adapter_kv_cache is None  # nothing is computed without a device
    names = {n for n, _ in model.named_parameters() if adapter.adapter_filter(n, None)}
    assert names == {k for k in state if spec.is_adapter_key(k)}
    adapter.mark_only_adapter_as_trainable(model)
    assert {n for n, p in model.named_parameters() if p.requires_grad} == names


def test_attach_refuses_missing_and_misshaped_tensors_naming_the_key(g7):
    from lit_gpt import GPT, adapter

    cfg, model = _cpu_model("mha")
    state = {k: v for k, v in _tensors(spec.fixture_state("mha", g7)).items() if spec.is_adapter_key(k)}
    for drop in ("transformer.h.2.attn.adapter_wte.weight", "transformer.h.1.attn.gating_factor"):
        with pytest.raises(ValueError, match=re.escape(drop)):
            adapter.attach(model, {k: v for k, v in state.items() if k != drop}, cfg)
    with pytest.raises(ValueError, match=r"transformer\.h\.1\.attn\.adapter_wte\.weight.*adapter_prompt_length 8"):
        adapter.attach(model, state, dataclasses.replace(cfg, adapter_prompt_length=8))  # a wrong aT
    bad = dict(state)
    bad["transformer.h.2.attn.gating_factor"] = torch.zeros(1, 1, 1, cfg.n_head)
    with pytest.raises(ValueError, match=r"transformer\.h\.2\.attn\.gating_factor"):
        adapter.attach(model, bad, cfg)
    with pytest.raises(ValueError, match="n_head"):
        adapter.attach(model, state, dataclasses.replace(cfg, n_head=2, n_query_groups=2))
    assert type(model) is GPT and not hasattr(model.transformer.h[1].attn, "adapter_wte")  # left as it was


def test_adapter_gpt_loads_both_gating_layouts(g7):
    from lit_gpt import adapter

    cfg = spec.adapter_config("gqa")
    state = _tensors(spec.fixture_state("gqa", g7))
    a = adapter.GPT(cfg)
    a.load_state_dict(state)
    old = {k: (v.permute(0, 2, 1, 3).contiguous() if "gating_factor" in k else v) for k, v in state.items()}
    b = adapter.GPT(cfg)
    b.load_state_dict(old)
    for blk_a, blk_b in zip(a.transformer.h[1:], b.transformer.h[1:]):
        assert torch.equal(blk_a.attn.gating_factor, blk_b.attn.gating_factor)
        assert blk_a.attn.gating_factor.shape == (1, 1, cfg.n_head, 1)
    assert not hasattr(a.transformer.h[0].attn, "adapter_wte")
    assert isinstance(a.transformer.h[0], adapter.Block) and a.transformer.h[2].attn.block_idx == 2


def test_config_carries_the_reference_fields():
    from lit_gpt import Config as Base
    from lit_gpt import adapter

    c = adapter.Config.from_name("Llama-2-7b-hf")
    assert isinstance(c, Base) and (c.adapter_prompt_length, c.adapter_start_layer) == (10, 2)
    assert adapter.adapter_filter("transformer.h.3.attn.adapter_wte.weight", None)
    assert adapter.adapter_filter("transformer.h.3.attn.gating_factor", None)
    assert not adapter.adapter_filter("transformer.h.3.attn.attn.weight", None)


# ------------------------------------------------------------------------------------------------ refusals
def test_check_supported_refusals():
    from lit_gpt import adapter

    cfg = spec.adapter_config("gqa")
    adapter.check_supported(cfg)
    adapter.check_supported(adapter.Config.from_name("pythia-160m"))  # partial rotary, parallel residual
    adapter.check_supported(adapter.Config.from_name("Mixtral-8x7B-v0.1"))  # sparse MoE: only attention is touched
    adapter.check_supported(dataclasses.replace(cfg, adapter_prompt_length=64))
    with pytest.raises(NotImplementedError, match="at most 64"):
        adapter.check_supported(dataclasses.replace(cfg, adapter_prompt_length=65))
    with pytest.raises(NotImplementedError, match="32-true"):
        adapter.check_supported(cfg, precision="32-true")
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        adapter.check_supported(cfg, world_size=2)
    with pytest.raises(ValueError, match="positive"):
        adapter.check_supported(dataclasses.replace(cfg, adapter_prompt_length=0))


def _fake_model(dtype=torch.bfloat16, hooks=False, modules=()):
    """What the refusals read of a model; any forward is a test failure (tests/test_samples_host.py's pattern)."""

    def forward(*a, **k):
        raise AssertionError("the fake model must not run")

    def part():
        return types.SimpleNamespace(_forward_hooks={})

    blocks = [types.SimpleNamespace(_forward_hooks={}, attn=part(), mlp=part()) for _ in range(3)]
    if hooks:
        blocks[1].attn._forward_hooks[0] = lambda *a: None
    wte = types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype))
    return types.SimpleNamespace(transformer=types.SimpleNamespace(wte=wte, h=blocks), forward=forward,
                                 __call__=forward, modules=lambda: iter(modules), config=spec.adapter_config("mha"))


def test_model_refusals_come_before_any_launch(monkeypatch):
    from lit_gpt import adapter, lora, ops

    def boom(*a, **k):
        raise AssertionError("a kernel was launched before the refusal")

    monkeypatch.setattr(ops, "adapter_attention", boom)
    monkeypatch.setattr(ops, "load_library", boom)
    cfg = spec.adapter_config("mha")
    adapter._check_model(_fake_model())
    with pytest.raises(NotImplementedError, match="32-true"):
        adapter.attach(_fake_model(dtype=torch.float32), {}, cfg)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        adapter.attach(_fake_model(hooks=True), {}, cfg)
    with pytest.raises(NotImplementedError, match="at most 64"):
        adapter.attach(_fake_model(), {}, dataclasses.replace(cfg, adapter_prompt_length=65))

    class FakeLora(lora.LoraLinear):
        def __init__(self):
            torch.nn.Module.__init__(self)

    with pytest.raises(NotImplementedError, match="LoRA"):
        adapter.attach(_fake_model(modules=[FakeLora()]), {}, cfg)
    many = _fake_model()
    many.lora_adapters = object()
    with pytest.raises(NotImplementedError, match="LoRA"):
        adapter.attach(many, {}, cfg)
    # an adapter model checks again at every entry: a model that later grows hooks is refused by forward,
    # decode_window and set_kv_cache, before the base class does anything
    model = adapter.GPT(dataclasses.replace(cfg, n_layer=2)).to(torch.bfloat16)
    model.transformer.h[1].attn.register_forward_hook(lambda *a: None)
    idx = torch.zeros(1, 1, dtype=torch.int64)
    for call in (lambda: model(idx), lambda: model.decode_window(idx.view(-1), idx.view(-1)),
                 lambda: model.set_kv_cache(1)):
        with pytest.raises(NotImplementedError, match="tensor parallelism"):
            call()
    with pytest.raises(NotImplementedError, match="32-true"):
        adapter.GPT(dataclasses.replace(cfg, n_layer=2))(idx)  # fp32 parameters


def test_generate_adapter_refuses_bad_arguments_before_building_a_model(monkeypatch, tmp_path):
    import generate.adapter as ga

    def boom(*a, **kw):
        raise AssertionError("the model was built before the refusal")

    monkeypatch.setattr(ga, "build_model", boom)
    kw = dict(synthetic="Llama-2-7b-hf", checkpoint_dir=tmp_path)
    with pytest.raises(NotImplementedError, match="32-true"):
        ga.main(precision="32-true", **kw)
    with pytest.raises(NotImplementedError, match="bf16-true"):
        ga.main(precision="16-true", **kw)
    with pytest.raises(ValueError, match="kv_cache"):
        ga.main(kv_cache="int8", **kw)
    with pytest.raises(ValueError, match="max_new_tokens"):
        ga.main(max_new_tokens=0, **kw)
    with pytest.raises(ValueError, match="top_p"):
        ga.main(top_p=0.0, **kw)
    with pytest.raises(NotImplementedError, match="quantize mode 'gptq.int4' is not supported"):
        ga.main(quantize="gptq.int4", **kw)
    monkeypatch.setattr(ga, "adapter_prompt_length", 65)
    with pytest.raises(NotImplementedError, match="at most 64"):
        ga.main(**kw)
    monkeypatch.setattr(ga, "adapter_prompt_length", 10)
    with pytest.raises((FileNotFoundError, OSError, SystemExit)):  # no checkpoint and no --synthetic
        ga.main(checkpoint_dir=tmp_path)
    # the command line: the reference's options plus --top_p, --kv_cache, --synthetic
    seen = {}
    monkeypatch.setattr(ga, "main", lambda *a: seen.setdefault("args", a))
    ga._cli(["--prompt", "hi", "--adapter_path", "a.pth", "--quantize", "nf4", "--max_new_tokens", "7", "--top_k",
             "none", "--temperature", "0", "--top_p", "0.9", "--kv_cache", "fp8", "--synthetic", "Llama-2-7b-hf"])
    a = seen["args"]
    assert a[0] == "hi" and a[2] == Path("a.pth") and a[4] == "nf4" and a[5] == 7 and a[6] is None and a[7] == 0.0
    assert a[9] == "Llama-2-7b-hf" and a[11] == 0.9 and a[12] == "fp8"
    assert "### Response:" in ga.generate_prompt({"instruction": "x", "input": ""})


# ------------------------------------------------------------------------------------------------ entry point
def test_adapter_kernels_use_no_scratch():
    """Every instantiation of the kernel has an empty private segment and spills nothing (the code object's metadata,
    read as tests/test_native_library.py reads it for the other decode kernels)."""
    from test_native_library import _kernel_scratch

    from lit_gpt import ops

    ours = {k: v for k, v in _kernel_scratch(ops.LIB_PATH).items() if "adapter_attention_kernel" in k}
    assert len(ours) == 3, sorted(ours)  # 64 / 128 / 256 head dims in registers
    assert all(v == (0, 0) for v in ours.values()), ours


def test_header_declares_and_the_library_validates_lga_adapter_attention():
    from lit_gpt import ops

    text = (REPO / "include" / "litgpt_amd.h").read_text()
    assert re.search(r"\bint\s+lga_adapter_attention\s*\(", text)
    assert "lga_adapter_attention" in ops.SIGNATURES
    lib = ops.load_library()
    f = lib.lga_adapter_attention
    p = ctypes.c_void_p(4096)

    def call(T=1, H=4, G=2, hs=128, n=128, aT=10, mode=0, ptr=p):
        return f(ptr, ptr, ptr, ptr, p, p, 64, ptr, mode, None, ptr, T, H, G, hs, n, aT, 0.1, None)

    assert call(ptr=None) != 0 and b"null" in lib.lga_last_error_string()
    assert call(aT=65) != 0 and b"1..64" in lib.lga_last_error_string()
    assert call(aT=0) != 0
    assert call(n=127) != 0 and b"even" in lib.lga_last_error_string()
    assert call(n=130) != 0
    assert call(hs=260, n=64) != 0 and b"at most 256" in lib.lga_last_error_string()
    assert call(hs=100, n=64) != 0  # hs % 8
    assert call(H=4, G=3) != 0 and b"n_head % n_query_groups" in lib.lga_last_error_string()
    assert call(T=0) != 0
    assert call(mode=3) != 0 and b"pos_mode" in lib.lga_last_error_string()
    with pytest.raises(ValueError, match=r"\(T, \(H \+ 2G\) \* hs\)"):
        ops.adapter_attention(torch.zeros(1, 8), torch.zeros(1, 9), torch.zeros(1, 1, 8), torch.zeros(1, 1, 8),
                              torch.zeros(1), torch.zeros(1, dtype=torch.int64), torch.zeros(4, 8), torch.zeros(4, 8), 1,
                              1, 8, 8, 1.0)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path
        ops.adapter_attention(torch.zeros(1, 8, dtype=torch.bfloat16), torch.zeros(1, 24, dtype=torch.bfloat16),
                              torch.zeros(1, 1, 8, dtype=torch.bfloat16), torch.zeros(1, 1, 8, dtype=torch.bfloat16),
                              torch.zeros(1, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int64), torch.zeros(4, 8),
                              torch.zeros(4, 8), 1, 1, 8, 8, 1.0)
