"""LoRA without a GPU: the specification (tests/lora_spec.py) against the reference's own logits (the g6 fixture), the
device layout ``lit_gpt.lora.attach`` builds against what the reference's ``lora_ind`` implies, rank padding, key
mapping, the refusals, and the argument validation of the lga_lora_* C entry points (they return before any launch)."""

import ctypes

import numpy as np
import pytest
import torch

import lora_spec as spec

KEYS = ("mha", "gqa")


@pytest.fixture(scope="module")
def g6():
    from pathlib import Path

    return np.load(Path(__file__).resolve().parent / "golden" / "g6_lora.npz", allow_pickle=False)


def _close(got, want, what):
    """Both sides fp32 evaluations of the same function: within 1e-4 of max |logit| (the reference's own merged and
    unmerged forwards differ by 7e-7 .. 9e-7 of that scale on these models)."""
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max error {err / scale:.2e} of the logit scale {scale:.3f}")
    assert err <= 1e-4 * scale, f"{what}: {err / scale:.2e} of the logit scale"


@pytest.mark.parametrize("key", KEYS)
def test_spec_reproduces_the_reference_unmerged_logits(g6, key):
    cfg = spec.lora_config(key)
    og = spec.LoraOracle(cfg, spec.fixture_state(key, g6), dtype=torch.float32)
    logits = og.forward(torch.from_numpy(g6[f"{key}/prompt"])).numpy()
    _close(logits, g6[f"{key}/logits_unmerged"], f"{key} unmerged")
    # ... and the adapter is not a no-op: the reference's own argmax moves against B = 0
    assert (g6[f"{key}/logits_unmerged"].argmax(-1) != g6[f"{key}/logits_no_adapter"].argmax(-1)).sum() >= 6


@pytest.mark.parametrize("key", KEYS)
def test_spec_over_the_merged_state_reproduces_the_reference_merged_logits(g6, key):
    from oracle.model import OracleGPT

    cfg = spec.lora_config(key)
    og = OracleGPT(cfg, spec.merged_state(cfg, spec.fixture_state(key, g6)), dtype=torch.float32)
    logits = og.forward(torch.from_numpy(g6[f"{key}/prompt"])).numpy()
    _close(logits, g6[f"{key}/logits_merged"], f"{key} merged")


@pytest.mark.parametrize("key", KEYS)
def test_spec_segments_are_the_reference_lora_ind(g6, key):
    cfg = spec.lora_config(key)
    N = (cfg.n_head + 2 * cfg.n_query_groups) * cfg.head_size
    seg = spec.qkv_segments(N, cfg.n_head, cfg.n_query_groups, (cfg.to_query, cfg.to_key, cfg.to_value))
    np.testing.assert_array_equal(torch.cat(seg).numpy(), g6[f"{key}/transformer.h.0.attn.attn.lora_ind"])


def _reference_lora_ind(out_features, n_head, n_query_groups, enable):
    """lora_ind as the fixture's generator read it off the reference, for any enable triple: the fixture pins the
    q + v case of both models; q, k and v rows partition the output, so any triple follows from the full one."""
    return torch.cat(spec.qkv_segments(out_features, n_head, n_query_groups, enable))


@pytest.mark.parametrize("enable", [(True, False, True), (True, True, True), (False, True, False)],
                         ids=["q+v", "q+k+v", "k"])
@pytest.mark.parametrize("heads", [(4, 4), (4, 2), (8, 1)], ids=["mha", "gqa", "mqa"])
def test_build_layout_scatters_rows_as_lora_ind_implies(enable, heads):
    from lit_gpt import lora

    n_head, groups = heads
    hs, K, r = 16, 64, 4
    N = (n_head + 2 * groups) * hs
    ind = _reference_lora_ind(N, n_head, groups, enable)
    n_seg = sum(enable)
    g = torch.Generator().manual_seed(3)
    A0 = torch.randn(r * n_seg, K, generator=g)
    B0 = torch.randn(ind.numel(), r, generator=g)
    A, B, off = lora.build_layout(A0, B0, r, N, (n_head, groups, enable))
    assert A.shape == (8 * n_seg, K) and B.shape == (N, 8) and off.dtype == torch.int32 and off.shape == (N,)
    # reference lora_B row i lands at output row lora_ind[i]; its segment is the one the reference's conv1d pairs it
    # with: rows are ordered q rows, k rows, v rows, and split by the slots' sizes
    sizes = [int(((off == s * 8)).sum()) for s in range(n_seg)]
    seg_of_i = torch.repeat_interleave(torch.arange(n_seg), torch.tensor(sizes))
    torch.testing.assert_close(B[ind, :r], B0, rtol=0, atol=0)
    assert not B[:, r:].any()
    np.testing.assert_array_equal(off[ind].numpy(), (seg_of_i * 8).numpy())
    rest = torch.ones(N, dtype=torch.bool)
    rest[ind] = False
    assert (off[rest] == -1).all() and not B[rest].any()
    for s in range(n_seg):
        torch.testing.assert_close(A[s * 8:s * 8 + r], A0[s * r:(s + 1) * r], rtol=0, atol=0)
        assert not A[s * 8 + r:(s + 1) * 8].any()
    # the same layout as the specification's own scatter
    As, Bs, offs = spec.scatter(A0, B0, r, N, spec.qkv_segments(N, n_head, groups, enable), pad_to=8)
    assert torch.equal(A, As) and torch.equal(B, Bs) and torch.equal(off, offs)


def test_build_layout_plain_linear_and_shape_errors():
    from lit_gpt import lora

    A0, B0 = torch.randn(8, 32), torch.randn(24, 8)
    A, B, off = lora.build_layout(A0, B0, 8, 24)
    assert off is None and torch.equal(A, A0) and torch.equal(B, B0)
    with pytest.raises(ValueError, match="do not match"):
        lora.build_layout(A0, B0, 4, 24)
    with pytest.raises(ValueError, match="do not match"):
        lora.build_layout(torch.randn(8, 64), torch.randn(10, 4), 4, 96, (4, 4, (True, False, True)))


@pytest.mark.parametrize("key", KEYS)
def test_layout_chain_equals_the_reference_forward_and_padding_changes_nothing(g6, key):
    """The device-layout chain over scatter() is the reference-layout forward of LoraOracle._lin, and padding r to a
    multiple of 8 (gqa: 4 -> 8) adds exact zeros only."""
    cfg = spec.lora_config(key)
    sd = spec.fixture_state(key, g6)
    og = spec.LoraOracle(cfg, sd, dtype=torch.float64)
    x = torch.randn(5, cfg.n_embd, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    prefix = "transformer.h.1.attn.attn"
    want = og._lin(prefix, x)
    A0, B0 = og.p[f"{prefix}.lora_A"], og.p[f"{prefix}.lora_B"]
    N = want.shape[1]
    seg = spec.qkv_segments(N, cfg.n_head, cfg.n_query_groups, (cfg.to_query, cfg.to_key, cfg.to_value))
    base = x @ og.p[f"{prefix}.weight"].T
    outs = []
    for pad in (1, 8):
        A, B, off = spec.scatter(A0, B0, cfg.r, N, seg, pad_to=pad)
        outs.append(spec.chain(x, A, B, off, cfg.alpha / cfg.r, base=base))
    torch.testing.assert_close(outs[0], want, rtol=1e-12, atol=1e-12)
    assert torch.equal(outs[0], outs[1])
    assert key != "gqa" or spec.scatter(A0, B0, cfg.r, N, seg, pad_to=8)[1].shape[1] == 8 != cfg.r


class _Recorder(torch.nn.Module):
    """Stands in for LoraLinear on a CPU model: attach's key mapping and layouts without the kernels."""

    def __init__(self, base, A, B, row_off, scaling):
        super().__init__()
        self.base, self.A, self.B, self.row_off, self.scaling = base, A, B, row_off, scaling


def _cpu_model(key):
    from lit_gpt import GPT

    cfg = spec.lora_config(key)
    with torch.device("meta"):
        model = GPT(cfg).to(torch.bfloat16)
    return cfg, model


@pytest.mark.parametrize("nested", [False, True], ids=["flat", "under-model"])
@pytest.mark.parametrize("key", KEYS)
def test_attach_maps_the_reference_keys(g6, key, nested, monkeypatch):
    from lit_gpt import lora

    monkeypatch.setattr(lora, "LoraLinear", _Recorder)
    cfg, model = _cpu_model(key)
    state = {k: torch.from_numpy(v) for k, v in spec.fixture_state(key, g6).items()}  # a full checkpoint is accepted
    lora.attach(model, {"model": state} if nested else state, cfg)
    adapted = {n for n, m in model.named_modules() if isinstance(m, _Recorder)}
    per_block = {"mha": ["attn.attn"], "gqa": ["attn.attn", "attn.proj", "mlp.fc_1", "mlp.fc_2", "mlp.proj"]}[key]
    want = {f"transformer.h.{i}.{n}" for i in range(cfg.n_layer) for n in per_block} | ({"lm_head"} if cfg.to_head else set())
    assert adapted == want
    qkv = model.transformer.h[1].attn.attn
    assert isinstance(qkv.base, torch.nn.Linear) and qkv.scaling == cfg.alpha / cfg.r
    ind = torch.from_numpy(g6[f"{key}/transformer.h.1.attn.attn.lora_ind"])
    torch.testing.assert_close(qkv.B[ind, :cfg.r], state["transformer.h.1.attn.attn.lora_B"], rtol=0, atol=0)
    assert (qkv.row_off[ind] >= 0).all() and int((qkv.row_off >= 0).sum()) == ind.numel()
    assert qkv.A.shape[0] == 2 * 8 and qkv.B.shape[1] == 8
    if cfg.to_head:
        assert model.lm_head.row_off is None and model.lm_head.A.shape[0] == 8


def test_attach_refuses_keys_and_shapes_that_do_not_match_the_config(g6, monkeypatch):
    from lit_gpt import lora

    monkeypatch.setattr(lora, "LoraLinear", _Recorder)
    cfg, model = _cpu_model("mha")
    state = {k: torch.from_numpy(v) for k, v in spec.fixture_state("mha", g6).items() if "lora_" in k}
    missing = dict(state)
    del missing["transformer.h.1.attn.attn.lora_B"]
    with pytest.raises(KeyError, match="missing"):
        lora.attach(model, missing, cfg)
    surplus = dict(state, **{"lm_head.lora_A": torch.zeros(8, 256), "lm_head.lora_B": torch.zeros(1024, 8)})
    with pytest.raises(KeyError, match="not targeted"):
        lora.attach(model, surplus, cfg)
    with pytest.raises(ValueError, match="do not match"):  # a rank-8 adapter under an r = 4 config
        lora.attach(model, state, _with(cfg, r=4))
    assert not any(isinstance(m, _Recorder) for m in model.modules())  # nothing was swapped by the failed calls


def _with(cfg, **kw):
    import dataclasses

    return dataclasses.replace(cfg, **kw)


def test_check_supported_refusals():
    from lit_gpt import lora

    cfg = spec.lora_config("gqa")
    lora.check_supported(cfg)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        lora.check_supported(cfg, world_size=2)
    with pytest.raises(NotImplementedError, match="32-true"):
        lora.check_supported(cfg, precision="32-true")
    moe = lora.Config.from_name("Mixtral-8x7B-v0.1", r=8, to_mlp=True)
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        lora.check_supported(moe)
    lora.check_supported(_with(moe, to_mlp=False, to_query=True))  # attention adapters on a MoE model are fine
    with pytest.raises(NotImplementedError, match="r <= 64"):
        lora.check_supported(_with(cfg, r=65))
    with pytest.raises(ValueError, match="enables no target"):
        lora.check_supported(lora.Config.from_name("Llama-2-7b-hf", r=8))
    with pytest.raises(ValueError, match="positive"):
        lora.check_supported(lora.Config.from_name("Llama-2-7b-hf", to_query=True))


def test_config_carries_the_reference_fields():
    from lit_gpt import Config as Base
    from lit_gpt import lora

    c = lora.Config.from_name("Llama-2-7b-hf", r=8, alpha=16, dropout=0.05, to_query=True, to_value=True)
    assert isinstance(c, Base) and (c.r, c.alpha, c.dropout) == (8, 16, 0.05)
    assert (c.to_query, c.to_key, c.to_value, c.to_projection, c.to_mlp, c.to_head) == (True, False, True, False,
                                                                                       False, False)
    assert lora.Config.from_name("Llama-2-7b-hf").r == 0


def test_merge_refuses_a_quantized_base_before_merging_anything(monkeypatch):
    from lit_gpt import lora, ops

    calls = []
    monkeypatch.setattr(ops, "lora_merge", lambda *a, **k: calls.append(a))

    class Fake(lora.LoraLinear):
        def __init__(self, base):
            torch.nn.Module.__init__(self)
            self.base = base

    class Quantized(torch.nn.Module):
        weight = bias = None

    holder = torch.nn.Module()
    holder.a = Fake(torch.nn.Linear(8, 8, bias=False).to(torch.bfloat16))
    holder.b = Fake(Quantized())
    with pytest.raises(NotImplementedError, match="quantize again"):
        lora.merge_lora_weights(holder)
    assert not calls and isinstance(holder.a, Fake)


def test_ops_signatures_and_argument_validation():
    """The new entry points are bound, and reject bad shapes before any launch (no GPU needed)."""
    from lit_gpt import ops

    for name in ("lga_lora_gemv", "lga_lora_down", "lga_lora_up", "lga_lora_merge"):
        assert name in ops.SIGNATURES
    lib = ops.load_library()
    p = ctypes.c_void_p(4096)
    assert lib.lga_lora_gemv(None, None, 1e-5, None, None, None, 2.0, None, None, None, 8, 8, 8, 8, None) != 0
    assert b"null" in lib.lga_last_error_string()
    assert lib.lga_lora_gemv(p, None, 1e-5, p, p, None, 2.0, None, None, p, 64, 100, 8, 8, None) != 0  # K % 8
    assert b"multiple of 8" in lib.lga_last_error_string()
    assert lib.lga_lora_gemv(p, None, 1e-5, p, p, None, 2.0, None, None, p, 64, 64, 8, 4, None) != 0  # r % 8
    assert b"r % 8" in lib.lga_last_error_string()
    assert lib.lga_lora_gemv(p, None, 1e-5, p, p, None, 2.0, None, None, p, 64, 64, 200, 8, None) != 0  # R > 192
    assert lib.lga_lora_up(p, p, None, 2.0, None, None, p, 4, 64, 72, 72, None) != 0  # r > 64
    assert lib.lga_lora_down(p, p, p, 4, 64, 12, None) != 0  # R % 8
    assert lib.lga_lora_merge(p, p, p, None, 2.0, 16, 60, 8, 8, None) != 0  # K % 8
    with pytest.raises(ValueError, match="outside the kernels' limits"):
        ops._lora_dims(torch.zeros(4, 64), torch.zeros(32, 4), None, "t")
    with pytest.raises(ValueError, match="needs row_off"):
        ops._lora_dims(torch.zeros(16, 64), torch.zeros(32, 8), None, "t")
