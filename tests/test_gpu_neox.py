"""BASELINE config 1 on the MI355X: pythia-160m (GPT-NeoX blocks — LayerNorm with bias, partial rotary 16 of 64
dims, parallel residual, biased Linears, exact-erf GELU MLP; reference lit_gpt/model.py:572-593, 691-702) through
the product's GPT.forward / generate, against

* the reference's own fp32 greedy run (tests/golden/g1_pythia160m_greedy.npz, made by importing /root/reference:
  tokens, step-0 logits, per-step margins), and
* the oracle (CPU restatement of the reference) on the same synthetic weights in bf16 and float64, with the bounds
  of tests/parity.py.

The product has no CPU path, so config 1 runs on the GPU in bf16 (the reference's CPU plumbing run is fp32): the
bound is "as accurate as the reference's own bf16 execution", and the greedy tokens must equal the fp32 reference's
wherever its top-1/top-2 margin clears the bf16 error.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import model as om
from oracle import quant, synth
from parity import check_step, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _pythia(mode="bf16", max_seq=16 + 128):
    """mode: "bf16" (bf16-true), "fp32" (32-true, the reference's config-1 precision) or a 4-bit quantize mode."""
    from lit_gpt import GPT, Config
    from lit_gpt.quantize import QuantizedPrecision

    cfg = Config.from_name("pythia-160m")
    sd = synth.state_dict(cfg, seed=1234)
    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    dt = torch.float32 if mode == "fp32" else torch.bfloat16
    model = model.to(device=DEV, dtype=dt)
    if mode not in ("bf16", "fp32"):
        QuantizedPrecision(mode).convert_module(model, DEV)
    model.max_seq_length = max_seq
    model.set_kv_cache(1, device=DEV, dtype=dt)
    return cfg, sd, model.eval()


def _oracles(cfg, sd, mode):
    def deq(k, v):
        if k.endswith(".weight") and v.ndim == 2 and not k.startswith("transformer.wte"):
            vb = quant.bf16_bits_to_f32(quant.f32_to_bf16_bits(v))
            return vb if mode == "bf16" else quant.dequantize_q4g(*quant.quantize_q4g(vb, 128), 128)
        return quant.bf16_bits_to_f32(quant.f32_to_bf16_bits(v)) if v.dtype == np.float32 else v

    return {dt: om.OracleGPT(cfg, sd, dtype=dt, weight_override=deq) for dt in (torch.bfloat16, torch.float64)}


@pytest.mark.parametrize("mode", ["bf16", "int4-g128"])
@torch.inference_mode()
def test_pythia160m_teacher_forced_on_reference_tokens(golden, mode):
    """Prefill the fixture's 16-token prompt, then decode teacher-forced on the reference's greedy tokens; every
    48th-or-so step (and the first 8) checked against the bf16 / float64 oracles; step 0 also against the fixture."""
    g = golden("g1_pythia160m_greedy.npz")
    cfg, sd, model = _pythia(mode)
    toks = torch.from_numpy(g["tokens"]).long()
    T = 16
    steps = list(range(8)) + list(range(8, 128, 13))
    got = {0: model(toks[:T].view(1, -1).to(DEV), torch.arange(T, device=DEV))[0, -1].float().cpu()}
    for i in range(1, 128):
        lg = model(toks[T + i - 1:T + i].view(1, 1).to(DEV), torch.tensor([T + i - 1], device=DEV))[0, -1]
        if i in steps:
            got[i] = lg.float().cpu()
    refs = {}
    for dt, ref in _oracles(cfg, sd, mode).items():
        ref.set_kv_cache(T + 128)
        out = {0: ref.forward(toks[:T], torch.arange(T))[-1]}
        for i in range(1, 128):
            lg = ref.forward(toks[T + i - 1:T + i], torch.tensor([T + i - 1]))[-1]
            if i in steps:
                out[i] = lg
        refs[dt] = out
    for i in steps:
        check_step(got[i], refs[torch.bfloat16][i], refs[torch.float64][i], f"pythia {mode} step {i}")
    if mode == "bf16":
        # the reference's own fp32 logits at step 0 (fixture): within the bf16 path's distance to exact arithmetic
        mx, rms, _ = rel_err(got[0], g["step0_logits"])
        fmx, frms, _ = rel_err(refs[torch.bfloat16][0], g["step0_logits"])
        assert mx <= 1.25 * fmx + 0.0025 and rms <= 1.25 * frms + 0.0025, (mx, rms, fmx, frms)


@torch.inference_mode()
def test_pythia160m_greedy_generate_follows_reference():
    """generate/base.py's loop (prefill + HIP-graph decode) on config 1: the 128 greedy tokens equal the fp32
    reference's (fixture) at every step whose reference margin exceeds the bf16 error bound — until the first step
    where the reference's own margin is within it (after that the two greedy streams may legitimately fork)."""
    from generate.base import generate

    g = np.load(__import__("pathlib").Path(__file__).parent / "golden" / "g1_pythia160m_greedy.npz")
    cfg, sd, model = _pythia("bf16")
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    y = generate(model, prompt, 16 + 128, temperature=0.0).cpu().numpy()
    ref, margins, absmax = g["tokens"], g["margins"], g["logits_absmax"]
    checked = 0
    for i in range(128):
        if margins[i] <= 0.03 * absmax[i]:
            break
        assert y[16 + i] == ref[16 + i], f"step {i}: {y[16 + i]} vs reference {ref[16 + i]}"
        checked += 1
    assert checked >= 4, checked


FP32_TOL = 2e-5  # relative to max |logit|: fp32 summation-order differences over 12 blocks (measured ~1e-6)


@torch.inference_mode()
def test_pythia160m_fp32_step0_logits_match_reference_fixture(golden):
    """BASELINE config 1 in its own precision (--precision 32-true, csrc/fp32.hip): the prefill's last-row logits
    equal the reference's fp32 logits (fixture g1, generated by importing /root/reference) to fp32 summation-order
    noise — no bf16 rounding anywhere on the path."""
    g = golden("g1_pythia160m_greedy.npz")
    cfg, sd, model = _pythia("fp32")
    prompt = torch.from_numpy(g["prompt"]).long().view(1, -1).to(DEV)
    lg = model(prompt, torch.arange(prompt.shape[1], device=DEV))[0, -1].cpu()
    assert lg.dtype == torch.float32
    ref = torch.from_numpy(g["step0_logits"]).float()
    err = float((lg - ref).abs().max() / ref.abs().max())
    assert err <= FP32_TOL, err


@torch.inference_mode()
def test_pythia160m_fp32_greedy_128_tokens_equal_reference():
    """generate/base.py's loop in fp32 (prefill + HIP-graph decode, fp32 argmax on the device): the 128 greedy
    tokens equal the reference's fp32 run (fixture) at every step up to the first whose reference top-1/top-2 margin
    is within the fp32 noise bound (after which two correct fp32 executions may legitimately fork)."""
    from generate.base import generate

    g = np.load(__import__("pathlib").Path(__file__).parent / "golden" / "g1_pythia160m_greedy.npz")
    cfg, sd, model = _pythia("fp32")
    prompt = torch.from_numpy(g["prompt"]).to(DEV)
    y = generate(model, prompt, 16 + 128, temperature=0.0).cpu().numpy()
    ref, margins, absmax = g["tokens"], g["margins"], g["logits_absmax"]
    checked = 0
    for i in range(128):
        if margins[i] <= 4 * FP32_TOL * absmax[i]:
            break
        assert y[16 + i] == ref[16 + i], f"step {i}: {y[16 + i]} vs reference {ref[16 + i]}"
        checked += 1
    assert checked >= 64, checked
    print(f"fp32: {checked} of 128 greedy tokens checked against the reference's fp32 run")


# ------------------------------------------------------------------ the NeoX block at the geometries pythia-160m is not
def _neox_cfg(kind):
    from lit_gpt import Config

    if kind == "pythia-14m":  # as registered: head_size 32, 8 rotary dims
        return Config.from_name("pythia-14m")
    if kind == "hs256":  # head_size 256, 64 rotary dims, as in pythia-1b
        return Config(n_layer=2, n_embd=512, n_head=2, vocab_size=512, padding_multiple=64, block_size=64)
    if kind == "falcon":  # MQA, one shared bias-free-Linear block norm, tanh GELU, full rotary; head_size 64
        return Config(n_layer=2, n_embd=256, n_head=4, n_query_groups=1, shared_attention_norm=True, bias=False,
                      gelu_approximate="tanh", rotary_percentage=1.0, vocab_size=512, padding_multiple=64,
                      block_size=64)
    raise KeyError(kind)


NEOX_T, NEOX_STEPS = 9, 8  # an odd prompt length, then 8 teacher-forced decode steps


def _neox_model(cfg, sd, dt):
    from lit_gpt import GPT

    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(device=DEV, dtype=dt)
    model.max_seq_length = NEOX_T + NEOX_STEPS
    model.set_kv_cache(1, device=DEV, dtype=dt)
    return model.eval()


def _neox_weights(cfg):
    """oracle.synth's weights; its all-zero biases and all-one norm weights are moved off those values (a kernel
    that dropped a bias or a norm weight would otherwise compute the same logits)."""
    sd = synth.state_dict(cfg, seed=4321)
    for k, v in sd.items():
        if k.endswith(".bias") or (k.endswith(".weight") and v.ndim == 1):
            sd[k] = (v + synth.normal(v.shape, k, 4321, 0.05)).astype(np.float32)
    return sd


def _teacher_forced(step, cfg):
    """step(tokens (T,), positions (T,)) -> last-row logits; the prompt, then one token at a time."""
    toks = torch.from_numpy(synth.token_ids(NEOX_T + NEOX_STEPS, cfg.vocab_size, seed=4321)).long()
    out = [step(toks[:NEOX_T], torch.arange(NEOX_T))]
    for i in range(NEOX_STEPS):
        out.append(step(toks[NEOX_T + i:NEOX_T + i + 1], torch.tensor([NEOX_T + i])))
    return out


def _product_step(model):
    return lambda t, p: model(t.view(1, -1).to(DEV), p.to(DEV))[0, -1].float().cpu()


def _oracle_step(ref):
    ref.set_kv_cache(NEOX_T + NEOX_STEPS)
    return lambda t, p: ref.forward(t, p)[-1]


@pytest.mark.parametrize("kind", ["pythia-14m", "hs256", "falcon"])
@torch.inference_mode()
def test_neox_fp32_geometries_match_float64_oracle(kind):
    """--precision 32-true outside pythia-160m's geometry: head_size 32 with 8 rotary dims, head_size 256 with 64,
    and a falcon-shaped block (MQA, shared attention norm, bias-free Linears, tanh GELU, full rotary). Last-row logits
    of a 9-token prefill and 8 teacher-forced decode steps against the oracle in float64 on the same unrounded fp32
    weights, within FP32_TOL (these models are shallower than the 12 blocks it was measured over). Measured on the
    MI355X: at most 3.0e-7 (2.1e-7 pythia-14m, 3.0e-7 head_size 256, 2.6e-7 falcon-shaped)."""
    cfg = _neox_cfg(kind)
    sd = _neox_weights(cfg)
    got = _teacher_forced(_product_step(_neox_model(cfg, sd, torch.float32)), cfg)
    exp = _teacher_forced(_oracle_step(om.OracleGPT(cfg, sd, dtype=torch.float64)), cfg)
    worst = 0.0
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == torch.float32 and g.shape == e.shape == (cfg.padded_vocab_size,)
        err = float((g.double() - e).abs().max() / e.abs().max())
        worst = max(worst, err)
        assert err <= FP32_TOL, (kind, i, err)
    print(f"{kind} fp32 vs float64 oracle: max relative error {worst:.2e}")


@torch.inference_mode()
def test_neox_falcon_block_bf16_matches_oracles():
    """The falcon-shaped block in bf16 (head_size 64: the bf16 attention kernels take it): the first GQA / MQA run of
    the NeoX block, against the bf16 and float64 oracles with the bounds of tests/parity.py."""
    cfg = _neox_cfg("falcon")
    sd = _neox_weights(cfg)
    got = _teacher_forced(_product_step(_neox_model(cfg, sd, torch.bfloat16)), cfg)
    refs = {dt: _teacher_forced(_oracle_step(o), cfg) for dt, o in _oracles(cfg, sd, "bf16").items()}
    for i, g in enumerate(got):
        check_step(g, refs[torch.bfloat16][i], refs[torch.float64][i], f"falcon-shaped bf16 step {i}")


@pytest.mark.parametrize("kind,hs", [("pythia-14m", 32), ("hs256", 256)])
@torch.inference_mode()
def test_neox_bf16_refuses_head_sizes_without_a_kernel(kind, hs):
    """The bf16 attention kernels exist for head_size 64 and 128 only: at 32 and 256 the product must raise an error
    that names the head size (prefill and decode alike) and return no logits — only --precision 32-true runs these
    geometries."""
    cfg = _neox_cfg(kind)
    assert cfg.head_size == hs
    model = _neox_model(cfg, _neox_weights(cfg), torch.bfloat16)
    toks = torch.from_numpy(synth.token_ids(NEOX_T, cfg.vocab_size, seed=4321)).long().to(DEV)
    for t, p in ((toks, torch.arange(NEOX_T, device=DEV)), (toks[:1], torch.tensor([0], device=DEV))):
        with pytest.raises(RuntimeError, match="head_size must be 64 or 128"):
            model(t.view(1, -1), p)
