"""LLaMA-Adapter (v1) on the MI355X: ``lga_adapter_attention`` against tests/adapter_spec.py, the fixture models end to
end in four weight formats (eager, through the decode graph, over an fp8 cache), every multi-row route bit for bit
against ``generate``, the launch count of a decode step, and generate/adapter.py.

Kernel tolerance, per element: the reference is the float64 evaluation WITH the bf16 rounding points applied
(``prefix_attention_spec``); the kernel may round each of ay, t and y the other way, one bf16 step each:
|y - spec| <= |g| ulp(ay) + ulp(t) + ulp(y). And at most 1 % of the elements may differ from the specification's bits
at all (fp32 against float64 sums straddle a bf16 rounding boundary with probability of order 1e-4 per rounding).
Measured on the MI355X over the 60 shapes: the worst element is 1.2e-6 inside the bound, and at most 0.0056 % of a
shape's elements differ from the specification's bits.
"""

import dataclasses
import json

import numpy as np
import pytest
import torch

import adapter_spec as spec
import int8_spec
import parity
from oracle import quant, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

GEOMETRIES = [(4, 4, 128, 128), (8, 2, 128, 128), (8, 1, 128, 128), (4, 2, 64, 16), (4, 4, 96, 96)]  # H, G, hs, rope
PREFIXES = [1, 10, 33, 64]
ROWS = [1, 3, 70]
ROPE_ROWS = 97


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


@pytest.fixture(scope="module")
def g7():
    from pathlib import Path

    return np.load(Path(__file__).resolve().parent / "golden" / "g7_adapter.npz", allow_pickle=False)


def _bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep float64 (CPU)."""
    return t.to(torch.bfloat16).double()


def _dev(t):
    return t.to(torch.bfloat16).to(DEV).contiguous()


def _ulp(v: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 (8 significant bits) at |v|."""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


_CASES = {}


def _case(H, G, hs, n, aT, T):
    """Seeded operands (bf16 values in float64) and the specification's result, computed once per shape: qkv, ak, av,
    gatings of both signs, a random y, non-zero non-monotone positions, the rope tables."""
    key = (H, G, hs, n, aT, T)
    if key not in _CASES:
        g = torch.Generator().manual_seed(H * 1000 + G * 100 + hs + n + 7 * aT + 13 * T)
        rnd = lambda *s, std=1.0: _bf(torch.randn(*s, generator=g, dtype=torch.float32) * std)  # noqa: E731
        theta = 1.0 / (10000 ** (torch.arange(0, n, 2, dtype=torch.float32) / n))
        ang = torch.outer(torch.arange(ROPE_ROWS, dtype=torch.float32), theta).repeat(1, 2)
        c = dict(qkv=rnd(T, (H + 2 * G) * hs), ak=rnd(G, aT, hs), av=rnd(G, aT, hs), y=rnd(T, H * hs),
                 gating=rnd(H, std=0.5).abs() * (1.0 - 2.0 * (torch.arange(H) % 2)),  # both signs, head by head
                 cos=torch.cos(ang), sin=torch.sin(ang),
                 pos=torch.randperm(ROPE_ROWS - 1, generator=g)[:T] + 1, scale=1.0 / hs ** 0.5)
        assert bool((c["gating"] > 0).any()) and bool((c["gating"] < 0).any()) and bool((c["pos"] > 0).all())
        parts = {}
        c["ref"] = spec.prefix_attention_spec(c["y"], c["qkv"], c["ak"], c["av"], c["gating"], c["cos"], c["sin"],
                                              c["pos"], H, G, hs, n, c["scale"], parts=parts)
        c["tol"] = (c["gating"].abs().view(1, H, 1) * _ulp(parts["ay"]) + _ulp(parts["t"])
                    + _ulp(c["ref"].view(T, H, hs))).view(T, H * hs)
        _CASES[key] = c
    return _CASES[key]


def _run(ops, c, H, G, hs, n, *, pos=None, pos_mode="rows", active=None, rows=None, y=None, gating=None, bits=False):
    """One launch on (a row slice of) the case; returns y on the CPU as float64, or (``bits``) as the int16 bit
    patterns of the bf16 result."""
    sl = slice(None) if rows is None else rows
    yd = _dev(c["y"][sl] if y is None else y)
    p = (c["pos"][sl] if pos is None else pos).to(DEV)
    out = ops.adapter_attention(yd, _dev(c["qkv"][sl]), _dev(c["ak"]), _dev(c["av"]),
                                _dev(c["gating"] if gating is None else gating), p, c["cos"].to(DEV), c["sin"].to(DEV), H,
                                G, hs, n, c["scale"], pos_mode=pos_mode,
                                active=None if active is None else active.to(DEV))
    assert out is yd
    return yd.view(torch.int16).cpu() if bits else yd.double().cpu()


def _bits(t):
    """The bf16 bit patterns (int16) of float64 values that hold bf16 values, NaN payloads as ``_dev`` sends them."""
    return t.to(torch.bfloat16).view(torch.int16)


def _check(got, ref, tol, what):
    err = (got - ref).abs()
    worst = float((err - tol).max())
    share = float((err > 0).double().mean())
    print(f"{what}: max error {float(err.max()):.3e}, worst error - tolerance {worst:.3e}, "
          f"{share:.4%} of the elements off the specification's bits")
    assert worst <= 0, f"{what}: error exceeds one bf16 step per rounding by {worst:.3e}"
    assert share <= 0.01, f"{what}: {share:.3%} of the elements differ from the specification's bits"


@pytest.mark.parametrize("T", ROWS)
@pytest.mark.parametrize("aT", PREFIXES)
@pytest.mark.parametrize("H,G,hs,n", GEOMETRIES)
def test_adapter_attention_matches_the_specification(ops, H, G, hs, n, aT, T):
    c = _case(H, G, hs, n, aT, T)
    got = _run(ops, c, H, G, hs, n)
    _check(got, c["ref"], c["tol"], f"H{H} G{G} hs{hs} rope{n} aT{aT} T{T}")
    assert not torch.equal(got, c["y"])  # the term is not a no-op on these operands


@pytest.mark.parametrize("H,G,hs,n", GEOMETRIES)
def test_adapter_attention_base_plus_index_and_one_position(ops, H, G, hs, n):
    """The verify window's positions (row t at pos[0] + t) and the shared position (every row at pos[0]) meet the
    specification at those positions under the per-element tolerance, and equal the per-row form's bits there."""
    aT, T = 10, 3
    c = _case(H, G, hs, n, aT, T)
    base = torch.tensor([41], dtype=torch.int64)
    for mode, pos in (("window", base + torch.arange(T)), ("one", base.expand(T).contiguous())):
        parts = {}
        ref = spec.prefix_attention_spec(c["y"], c["qkv"], c["ak"], c["av"], c["gating"], c["cos"], c["sin"], pos, H, G,
                                         hs, n, c["scale"], parts=parts)
        tol = (c["gating"].abs().view(1, H, 1) * _ulp(parts["ay"]) + _ulp(parts["t"])
               + _ulp(ref.view(T, H, hs))).view(T, H * hs)
        got = _run(ops, c, H, G, hs, n, pos=base, pos_mode=mode)
        _check(got, ref, tol, f"H{H} G{G} hs{hs} rope{n} positions '{mode}'")
        assert torch.equal(got, _run(ops, c, H, G, hs, n, pos=pos)), mode


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,G,hs,n", [(6, 2, 64, 64), (3, 1, 128, 128), (5, 5, 96, 32)])
def test_adapter_attention_workgroup_tail(ops, H, G, hs, n, T):
    """Head counts that leave the last workgroup partly empty (T * H is no multiple of its 4 waves: 6, 18, 3, 9, 5,
    15): the waves past the end take part in the barriers and write nothing. y is followed by a guard block in the
    same allocation, which must keep its bits."""
    aT = 10
    c = _case(H, G, hs, n, aT, T)
    assert (T * H) % 4 != 0
    _check(_run(ops, c, H, G, hs, n), c["ref"], c["tol"], f"tail H{H} G{G} hs{hs} rope{n} T{T}")
    buf = torch.full((T + 2, H * hs), 7.0, dtype=torch.bfloat16, device=DEV)
    buf[:T] = _dev(c["y"])
    ops.adapter_attention(buf[:T], _dev(c["qkv"]), _dev(c["ak"]), _dev(c["av"]), _dev(c["gating"]), c["pos"].to(DEV),
                          c["cos"].to(DEV), c["sin"].to(DEV), H, G, hs, n, c["scale"])
    assert torch.equal(buf[:T].double().cpu(), _run(ops, c, H, G, hs, n)) and bool((buf[T:] == 7.0).all())


@pytest.mark.parametrize("aT", [10, 64])
@pytest.mark.parametrize("H,G,hs,n", GEOMETRIES)
def test_adapter_attention_row_does_not_depend_on_T(ops, H, G, hs, n, aT):
    """Row r of a T-row call equals the one-row call on that row, bit for bit (T = 70: more than one workgroup per
    head count, rows that share a workgroup with another row's heads)."""
    c = _case(H, G, hs, n, aT, 70)
    whole = _run(ops, c, H, G, hs, n)
    for r in (0, 1, 33, 69):
        one = _run(ops, c, H, G, hs, n, rows=slice(r, r + 1))
        assert torch.equal(one[0], whole[r]), r
    three = _run(ops, c, H, G, hs, n, rows=slice(5, 8))
    assert torch.equal(three, whole[5:8])


@pytest.mark.parametrize("H,G,hs,n", GEOMETRIES)
def test_adapter_attention_idle_rows_and_zero_gating_keep_their_bits(ops, H, G, hs, n):
    """``active``: every idle row — all with positions inside the rope tables, so nothing but the flag can skip them,
    one of them holding NaNs — keeps its input bits (compared as bf16 bit patterns), and the active rows get the bits
    of the call without the flag. Then the same with the idle rows' positions far outside the tables (an idle row's
    position is never used to address anything). A zero gating leaves y bit-identical."""
    aT, T = 33, 70
    c = _case(H, G, hs, n, aT, T)
    whole = _run(ops, c, H, G, hs, n, bits=True)
    active = (torch.arange(T) % 3 != 1).to(torch.int32)
    idle = active == 0
    assert int(idle.sum()) == 23 and bool(((c["pos"] > 0) & (c["pos"] < ROPE_ROWS)).all())
    y = c["y"].clone()
    y[1] = float("nan")  # an idle row
    y_bits = _bits(y)
    without = _run(ops, c, H, G, hs, n, y=y, bits=True)
    assert not any(torch.equal(without[r], y_bits[r]) for r in torch.nonzero(idle).flatten().tolist() if r != 1)
    got = _run(ops, c, H, G, hs, n, active=active, y=y, bits=True)
    assert torch.equal(got[idle], y_bits[idle]), "an idle row's y changed"
    assert torch.equal(got[~idle], whole[~idle]) and not torch.equal(got[~idle], y_bits[~idle])
    far = torch.where(idle, torch.full_like(c["pos"], 10 ** 9), c["pos"])
    assert torch.equal(_run(ops, c, H, G, hs, n, pos=far, active=active, y=y, bits=True), got)
    zero = _run(ops, c, H, G, hs, n, gating=torch.zeros(H, dtype=torch.float64), bits=True)
    assert torch.equal(zero, _bits(c["y"]))


def test_adapter_attention_argument_errors_launch_nothing(ops):
    H, G, hs = 4, 2, 128
    y = torch.zeros(1, H * hs, dtype=torch.bfloat16, device=DEV)
    qkv = torch.zeros(1, (H + 2 * G) * hs, dtype=torch.bfloat16, device=DEV)
    gating = torch.ones(H, dtype=torch.bfloat16, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    table = torch.zeros(4, hs, device=DEV)
    kv = lambda aT, d=hs: torch.ones(G, aT, d, dtype=torch.bfloat16, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="1..64"):
        ops.adapter_attention(y, qkv, kv(65), kv(65), gating, pos, table, table, H, G, hs, hs, 0.1)
    odd = torch.zeros(4, 127, device=DEV)
    with pytest.raises(RuntimeError, match="even"):
        ops.adapter_attention(y, qkv, kv(10), kv(10), gating, pos, odd, odd, H, G, hs, 127, 0.1)
    y260 = torch.zeros(1, H * 260, dtype=torch.bfloat16, device=DEV)
    qkv260 = torch.zeros(1, (H + 2 * G) * 260, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="at most 256"):
        ops.adapter_attention(y260, qkv260, kv(10, 260), kv(10, 260), gating, pos, table, table, H, G, 260, hs, 0.1)
    torch.cuda.synchronize()
    assert float(y.abs().sum()) == 0 and float(y260.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ model
MODES = ["int4-g128", "nf4", "bnb.int8", "bf16"]
T_PROMPT, N_DECODE = 12, 8


def _rounded(sd):
    return {k: int8_spec.bf16_round(v) for k, v in sd.items()}


def _gpu_model(cfg, sd, mode, max_seq, fp8=False):
    """A ``lit_gpt.GPT`` on the device in the weight format ``mode``, with the adapter of ``sd`` attached."""
    from lit_gpt import GPT, adapter
    from lit_gpt.quantize import QuantizedPrecision

    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not spec.is_adapter_key(k)})
    model = model.to(device=DEV, dtype=torch.bfloat16)
    if mode != "bf16":
        QuantizedPrecision(mode).convert_module(model, DEV)
    model.max_seq_length = max_seq
    model.set_kv_cache(1, device=DEV, dtype=torch.float8_e4m3fn if fp8 else None)
    adapter.attach(model, {k: torch.from_numpy(v) for k, v in sd.items() if spec.is_adapter_key(k)}, cfg)
    return model.eval()


class _Oracle(spec.AdapterOracle):
    """AdapterOracle over the base the device model holds: the dequantized 4-bit weight (or the bf16 weight) through
    ``weight_override``; for bnb.int8, whose Linear also quantizes its input, the int8 specification's Linear."""

    def __init__(self, cfg, sd, mode, dtype):
        def deq(k, v):
            if spec.is_adapter_key(k) or not (k.endswith(".weight") and v.ndim == 2) or k.startswith("transformer.wte"):
                return v
            if mode == "int4-g128":
                return quant.dequantize_q4g(*quant.quantize_q4g(v, 128), 128)
            if mode == "nf4":
                return quant.dequantize_fmt(*quant.quantize_fmt(v, 1, 64), 1, 64)
            return v

        super().__init__(cfg, sd, dtype=dtype, weight_override=deq)
        self.mode, self.q8 = mode, {}

    def _lin(self, prefix, x):
        if self.mode != "bnb.int8":
            return super()._lin(prefix, x)
        if prefix not in self.q8:
            self.q8[prefix] = int8_spec.quantize_weight(self.p[f"{prefix}.weight"].float().numpy())
        q, s = self.q8[prefix]
        xn = x.float().numpy()
        if self.dtype == torch.bfloat16:
            return torch.from_numpy(int8_spec.linear(xn, q, s)).to(torch.bfloat16)
        return torch.from_numpy(int8_spec.linear_exact(xn, q, s))


def _teacher_forced(forward, prompt, stream):
    out = list(forward(prompt, torch.arange(T_PROMPT)))  # every prefill row
    for i in range(N_DECODE):
        out.append(forward(stream[i:i + 1], torch.tensor([T_PROMPT + i]))[-1])
    return out


def _oracle_logits(ref, prompt, stream):
    ref.set_kv_cache(T_PROMPT + N_DECODE + 1)
    return _teacher_forced(lambda idx, pos: ref.forward(idx, pos), prompt, stream)


def _gpu_logits(model, prompt, stream):
    return _teacher_forced(lambda idx, pos: model(idx.view(1, -1).to(DEV), pos.to(DEV))[0].float().cpu(), prompt,
                           stream)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_model_teacher_forced_logits_and_graph(g7, key, mode, monkeypatch):
    """The 12 prefill rows + 8 teacher-forced decode steps of the fixture model against the spec oracle in bf16 and
    float64 (tests/parity.py's bounds, nothing new); the adapter moves a clearly pinned argmax; the decode graph equals
    eager bit for bit; zeroed gatings give the un-adapted model's bits."""
    from lit_gpt import GPT
    from lit_gpt import ops as ops_mod
    from lit_gpt.runtime import DecodeGraph

    cfg = spec.adapter_config(key)
    sd = _rounded(spec.fixture_state(key, g7))
    prompt = torch.from_numpy(g7[f"{key}/prompt"])
    stream = torch.from_numpy(synth.token_ids(N_DECODE, cfg.vocab_size, seed=22))
    model = _gpu_model(cfg, sd, mode, T_PROMPT + N_DECODE + 1)
    got = _gpu_logits(model, prompt, stream)
    exp = {dt: _oracle_logits(_Oracle(cfg, sd, mode, dt), prompt, stream) for dt in (torch.bfloat16, torch.float64)}
    assert len(got) == T_PROMPT + N_DECODE
    errs = [parity.check_step(g, exp[torch.bfloat16][i], exp[torch.float64][i], f"adapter {key} {mode} row {i}")
            for i, g in enumerate(got)]
    zero_sd = {k: (np.zeros_like(v) if "gating_factor" in k else v) for k, v in sd.items()}
    plain = _oracle_logits(_Oracle(cfg, zero_sd, mode, torch.float64), prompt, stream)
    # the adapter matters: a product without the term would be an evaluation of the zero-gating model and land within
    # check_step's accuracy bound of THAT oracle. The fixture's adapter shifts the logits by about a fifth of their
    # scale, so at MIN_MOVED rows or more the product is over twice that bound away from it; and wherever the adapter
    # moves an argmax that check_step's margin rule pins, the product follows the adapted oracle
    moved = far = 0
    for i, (a, p) in enumerate(zip(exp[torch.float64], plain)):
        allowed = parity.ACC_FACTOR * parity.rel_err(exp[torch.bfloat16][i], a)[0] + parity.ACC_SLACK
        far += parity.rel_err(got[i], p)[0] > 2 * allowed
        top = torch.topk(a.double(), 2).values
        clear = float(top[0] - top[1]) > 4 * errs[i] * float(a.abs().max())
        if clear and int(a.argmax()) != int(p.argmax()):
            assert int(got[i].argmax()) == int(a.argmax()) != int(p.argmax())
            moved += 1
    print(f"adapter {key} {mode}: {far} of {len(got)} rows far from the zero-gating oracle, {moved} pinned argmax moved")
    assert far >= spec.MIN_MOVED, "the product is an evaluation of the un-adapted model: the test would pass without it"
    # decode graph == eager, bit for bit (tests/test_gpu_lora.py's method)
    handed = []
    for name in ("argmax_embed", "argmax"):
        orig = getattr(ops_mod, name)
        monkeypatch.setattr(ops_mod, name, lambda lg, *a, _o=orig, **k: (handed.append(lg), _o(lg, *a, **k))[1])
    model(prompt.view(1, -1).to(DEV), torch.arange(T_PROMPT, device=DEV))
    dg = DecodeGraph(model, stream[0:1].to(DEV), T_PROMPT)
    buf = dg.logits if getattr(dg, "logits", None) is not None else handed[-1]
    for i in range(1, N_DECODE):
        dg.token.fill_(int(stream[i]))
        dg.x_emb.copy_(model.transformer.wte.weight[int(stream[i])])
        dg.step()
        assert torch.equal(buf.float().cpu().view(-1), got[T_PROMPT + i]), f"{key} {mode}: graph step {i} != eager"
    # zeroed gatings: the un-adapted model's logits, bit for bit (in place: the launch reads the same tensor)
    for blk in model.transformer.h[cfg.adapter_start_layer:]:
        blk.attn.gating_factor.zero_()
    zeroed = _gpu_logits(model, prompt, stream)
    base = GPT(cfg)
    base.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not spec.is_adapter_key(k)})
    base = base.to(device=DEV, dtype=torch.bfloat16)
    if mode != "bf16":
        from lit_gpt.quantize import QuantizedPrecision

        QuantizedPrecision(mode).convert_module(base, DEV)
    base.max_seq_length = T_PROMPT + N_DECODE + 1
    base.set_kv_cache(1, device=DEV)
    for z, b in zip(zeroed, _gpu_logits(base.eval(), prompt, stream)):
        assert torch.equal(z, b)
    assert not all(torch.equal(z, g) for z, g in zip(zeroed, got))


@torch.inference_mode()
def test_neox_block_with_partial_rotary_matches_the_oracles():
    """A GPT-NeoX model (LayerNorm, parallel residual, biased Linears, head_size 64 with 16 rotary dims: the family of
    the reference's default adapter checkpoints) in bf16, one sequence: only attention is touched, so the adapter runs
    there too. 12 prefill rows + 8 decode steps under tests/parity.py's bounds."""
    from lit_gpt.adapter import Config

    cfg = Config(n_layer=3, n_embd=256, n_head=4, vocab_size=512, padding_multiple=64, block_size=64,
                 adapter_start_layer=1)
    assert cfg.parallel_residual and cfg.rope_n_elem == 16 and cfg.head_size == 64 and cfg.bias
    sd = synth.state_dict(cfg, seed=4321)
    for k, v in sd.items():  # synth's zero biases and unit norm weights, moved off those values
        if k.endswith(".bias") or (k.endswith(".weight") and v.ndim == 1):
            sd[k] = (v + synth.normal(v.shape, k, 4321, 0.05)).astype(np.float32)
    sd = _rounded({**sd, **spec.random_adapter(cfg)})
    prompt = torch.from_numpy(synth.token_ids(T_PROMPT, cfg.vocab_size, seed=spec.SEED))
    stream = torch.from_numpy(synth.token_ids(N_DECODE, cfg.vocab_size, seed=22))
    model = _gpu_model(cfg, sd, "bf16", T_PROMPT + N_DECODE + 1)
    got = _gpu_logits(model, prompt, stream)
    exp = {dt: _oracle_logits(_Oracle(cfg, sd, "bf16", dt), prompt, stream) for dt in (torch.bfloat16, torch.float64)}
    for i, g in enumerate(got):
        parity.check_step(g, exp[torch.bfloat16][i], exp[torch.float64][i], f"adapter neox row {i}")
    zero_sd = {k: (np.zeros_like(v) if "gating_factor" in k else v) for k, v in sd.items()}
    plain = _oracle_logits(_Oracle(cfg, zero_sd, "bf16", torch.float64), prompt, stream)
    far = 0
    for i, (a, p) in enumerate(zip(exp[torch.float64], plain)):
        allowed = parity.ACC_FACTOR * parity.rel_err(exp[torch.bfloat16][i], a)[0] + parity.ACC_SLACK
        far += parity.rel_err(got[i], p)[0] > 2 * allowed
    assert far >= spec.MIN_MOVED, far


def test_prefix_kv_follow_the_weights(g7):
    """The cached prefix K / V are dropped when the weights they came from change: a quantization conversion after
    ``attach``, an in-place update of the prefix or of the qkv weight, ``load_state_dict``. Each time the next use
    recomputes them from the layer's own qkv Linear as it then is; untouched weights keep the cached pair."""
    from lit_gpt.model import _lin
    from lit_gpt.quantize import QuantizedPrecision

    key = "gqa"
    cfg = spec.adapter_config(key)
    sd = _rounded(spec.fixture_state(key, g7))
    model = _gpu_model(cfg, sd, "bf16", 32)  # (built outside inference mode: its tensors keep version counters)
    attn = model.transformer.h[1].attn
    G, hs, qpk, aT = cfg.n_query_groups, cfg.head_size, cfg.n_head // cfg.n_query_groups, cfg.adapter_prompt_length

    def fresh():
        with torch.no_grad():
            a = _lin(attn.attn, attn.adapter_wte.weight.view(1, aT, -1)).view(aT, G, qpk + 2, hs)
        return a[:, :, qpk].transpose(0, 1), a[:, :, qpk + 1].transpose(0, 1)

    def current():
        with torch.no_grad():
            return attn.adapter_kv()

    ak0, av0 = current()
    assert attn.adapter_kv_cache is not None and torch.equal(ak0, fresh()[0]) and torch.equal(av0, fresh()[1])
    assert current()[0] is ak0  # nothing changed: the cached pair
    with torch.no_grad():
        attn.adapter_wte.weight.mul_(2.0)  # in place: same storage
    ak1, av1 = current()
    assert ak1 is not ak0 and not torch.equal(ak1, ak0) and torch.equal(ak1, fresh()[0]) and torch.equal(av1, fresh()[1])
    with torch.no_grad():
        attn.attn.weight.mul_(0.5)
    ak2, _ = current()
    assert ak2 is not ak1 and torch.equal(ak2, fresh()[0]) and not torch.equal(ak2, ak1)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(state)
    assert all(b.attn.adapter_kv_cache is None for b in model.transformer.h[cfg.adapter_start_layer:])
    assert torch.equal(current()[0], ak2)
    ak2 = attn.adapter_kv_cache[0]
    QuantizedPrecision("int4-g128").convert_module(model, DEV)  # after attach: another module in attn.attn's place
    assert type(attn.attn).__name__ == "QuantLinear"
    model.set_kv_cache(1, device=DEV)
    ak3, av3 = attn.adapter_kv_cache[:2]
    assert ak3 is not ak2 and torch.equal(ak3, fresh()[0]) and torch.equal(av3, fresh()[1])
    assert not torch.equal(ak3, ak2)  # the 4-bit weight's keys, not the bf16 weight's


def _wide(key, mode="int4-g128", fp8=False, max_seq=64):
    """The fixture model widened to head_size 128, base weights from oracle.synth, a random adapter."""
    cfg = spec.wide_config(key)
    sd = _rounded({**synth.state_dict(cfg, seed=spec.SEED), **spec.random_adapter(cfg)})
    return cfg, sd, _gpu_model(cfg, sd, mode, max_seq, fp8=fp8)


@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_model_over_the_fp8_cache_follows_the_fp8_specification(key):
    """int4-g128 over the fp8 KV cache, teacher-forced, against AdapterOracle + the fp8 cache specification: the bound of
    tests/test_gpu_kv8.py test_model_logits_follow_the_fp8_specification (2 R, R the bf16 specification's own largest
    distance to the float64 one over the run)."""
    import kv8_spec
    from parity import rel_err

    cfg, sd, model = _wide(key, fp8=True, max_seq=T_PROMPT + N_DECODE + 1)
    assert model.transformer.h[0].attn.kv_cache.fp8
    prompt = torch.from_numpy(synth.token_ids(T_PROMPT, cfg.vocab_size, seed=spec.SEED))
    stream = torch.from_numpy(synth.token_ids(N_DECODE, cfg.vocab_size, seed=22))
    got = _gpu_logits(model, prompt, stream)
    refs = {}
    for dt in (torch.float64, torch.bfloat16):
        og = _Oracle(cfg, sd, "int4-g128", dt)
        og.set_kv_cache(T_PROMPT + N_DECODE + 1)
        og.cache = kv8_spec.Kv8Cache(k=og.cache.k, v=og.cache.v)
        refs[dt] = [r.double() for r in _teacher_forced(lambda idx, pos: og.forward(idx, pos), prompt, stream)]
    exact, bf = refs[torch.float64], refs[torch.bfloat16]
    R = max(rel_err(b, e)[0] for b, e in zip(bf, exact))
    worst = [0.0] * 4
    for i, (g, b, e) in enumerate(zip(got, bf, exact)):
        e_max, e_rms, _ = rel_err(g, e)
        b_max, b_rms, _ = rel_err(g, b)
        worst = [max(w, x) for w, x in zip(worst, (e_max, e_rms, b_max, b_rms))]
        assert e_max <= 2 * R and e_rms <= 2 * R, (i, e_max, e_rms, R)
        assert b_max <= 2 * R and b_rms <= 2 * R, (i, b_max, b_rms, R)
    print(f"\nadapter {key} fp8: R = {R:.3%}; product vs float64 max {worst[0] / R:.2f} R rms {worst[1] / R:.2f} R; vs "
          f"bf16 oracle max {worst[2] / R:.2f} R rms {worst[3] / R:.2f} R")


# ------------------------------------------------------------------------------------------------ multi-row routes
NEW = 10
_MODELS = {}


def _shared_wide(key):
    if key not in _MODELS:
        _MODELS[key] = _wide(key)
    return _MODELS[key]


def _cache(model, B):
    model.set_kv_cache(batch_size=B, device=DEV)


def _prompts(vocab, lens):
    return [torch.from_numpy(synth.token_ids(n, vocab, seed=40 + n)).to(DEV) for n in lens]


def _singles(model, prompts, budgets, seeds=None, **kw):
    from generate.base import SamplerRNG, generate

    out = []
    for i, (p, m) in enumerate(zip(prompts, budgets)):
        _cache(model, 1)
        rng = None if seeds is None else SamplerRNG(DEV, seed=seeds[i])
        out.append(generate(model, p, p.numel() + m, rng=rng, **kw).cpu())
    return out


SAMPLING = [dict(temperature=0.0), dict(temperature=0.8, top_k=200)]


@pytest.mark.parametrize("kw", SAMPLING, ids=["greedy", "sampled"])
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_generate_batch_equals_generate(key, kw):
    from generate.base import generate_batch

    cfg, _, model = _shared_wide(key)
    prompts = _prompts(cfg.vocab_size, (5, 12, 9))
    seeds = [11, 12, 13] if kw["temperature"] > 0 else None
    single = _singles(model, prompts, (NEW,) * 3, seeds, **kw)
    outs = generate_batch(model, prompts, NEW, seeds=seeds, **kw)
    for b in range(3):
        assert torch.equal(outs[b].cpu(), single[b]), (b, outs[b].tolist(), single[b].tolist())
    assert len({tuple(s[-NEW:].tolist()) for s in single}) == 3
    _cache(model, 1)


@pytest.mark.parametrize("kw", SAMPLING, ids=["greedy", "sampled"])
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_generate_continuous_equals_generate(key, kw):
    """5 prompts through 2 slots: slots go idle and are refilled, the idle rows pass ``active`` to the adapter launch."""
    from generate.base import generate_continuous

    cfg, _, model = _shared_wide(key)
    prompts = _prompts(cfg.vocab_size, (5, 12, 9, 7, 10))
    budgets = (4, 10, 7, 3, 9)
    seeds = [21, 22, 23, 24, 25] if kw["temperature"] > 0 else None
    single = _singles(model, prompts, budgets, seeds, **kw)
    outs = generate_continuous(model, prompts, list(budgets), batch_size=2, seeds=seeds, **kw)
    for i in range(5):
        assert torch.equal(outs[i].cpu(), single[i]), (i, outs[i].tolist(), single[i].tolist())
    _cache(model, 1)


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("kw", SAMPLING, ids=["greedy", "sampled"])
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_generate_samples_equals_generate(key, kw, share):
    from generate.base import generate_samples

    cfg, _, model = _shared_wide(key)
    prompt = _prompts(cfg.vocab_size, (12,))[0]
    seeds = [31, 32, 33] if kw["temperature"] > 0 else None
    single = _singles(model, [prompt] * 3, (NEW,) * 3, seeds, **kw)
    _cache(model, 1)
    outs = generate_samples(model, prompt, NEW, 3, seeds=seeds, share=share, **kw)
    for i in range(3):
        assert torch.equal(outs[i].cpu(), single[i]), (i, outs[i].tolist(), single[i].tolist())
    _cache(model, 1)


@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_generate_speculative_equals_generate(key):
    from generate.speculative import NgramDrafter, generate_speculative

    cfg, _, model = _shared_wide(key)
    # a repetitive prompt, so that the n-gram drafter proposes and windows of several rows are verified
    base = synth.token_ids(6, cfg.vocab_size, seed=50)
    prompt = torch.from_numpy(np.concatenate([base, base, base[:4]])).to(DEV)
    single = _singles(model, [prompt], (24,), temperature=0.0)[0]
    _cache(model, 1)
    stats = {}
    out = generate_speculative(model, prompt, prompt.numel() + 24, NgramDrafter(), speculate=4, stats=stats)
    assert torch.equal(out.cpu(), single), (out.tolist(), single.tolist())
    print(f"speculative {key}: {stats}")
    _cache(model, 1)


# ------------------------------------------------------------------------------------------------ launches
class Recorder:
    """Stands in for ``ops._lib`` (as tests/test_gpu_dispatch.py): logs the name of every ``lga_*`` call."""

    def __init__(self, ops):
        self.lib, self.calls = ops.load_library(), []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("lga_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_one_adapter_launch_per_adapted_block_per_step_and_no_torch_matmul(g7, key, mode, monkeypatch):
    from torch.utils._python_dispatch import TorchDispatchMode

    from lit_gpt import ops

    cfg = spec.adapter_config(key)
    model = _gpu_model(cfg, _rounded(spec.fixture_state(key, g7)), mode, 32)
    rec = Recorder(ops)
    monkeypatch.setattr(ops, "_lib", rec)
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func.__name__)
            return func(*args, **(kwargs or {}))

    idx = torch.from_numpy(g7[f"{key}/prompt"]).to(DEV)
    with Watch():
        model(idx[:8].view(1, -1), torch.arange(8, device=DEV))
        prefill, rec.calls = rec.calls, []
        model(idx[8:9].view(1, 1), torch.tensor([8], device=DEV))
        decode, rec.calls = rec.calls, []
        model(idx[:8].view(1, -1))  # the no-cache forward
        nocache = rec.calls
    bad = [f for f in seen if any(s in f for s in ("mm", "matmul", "linear", "einsum", "dot", "scaled_dot", "softmax"))]
    assert not bad, bad
    n = cfg.n_layer - cfg.adapter_start_layer
    assert n == 2
    for calls in (prefill, decode, nocache):
        assert calls.count("lga_adapter_attention") == n, calls
    # the launch follows the block's attention launch directly and precedes the out-projection
    for i, name in enumerate(decode):
        if name == "lga_adapter_attention":
            assert "attention" in decode[i - 1] and decode[i - 1] != name, decode[max(0, i - 2):i + 2]


# ------------------------------------------------------------------------------------------------ entry point
@pytest.mark.parametrize("quantize", [None, "int4-g128"], ids=["bf16", "int4-g128"])
@torch.inference_mode()
def test_generate_adapter_entry_point_follows_the_oracle(g7, tmp_path, monkeypatch, capsys, quantize):
    """generate/adapter.py --synthetic on a checkpoint + adapter written here: its greedy tokens equal the float64
    oracle's argmax wherever ``parity.check_step``'s margin rule pins them — the margin exceeds 4 x the largest error
    that function allows the product at that step (ACC_FACTOR x the bf16 oracle's own error + ACC_SLACK)."""
    import generate.adapter as ga

    key = "gqa"
    cfg = spec.adapter_config(key)
    sd = _rounded(spec.fixture_state(key, g7))
    base_fields = {f.name for f in dataclasses.fields(cfg)} - {"adapter_prompt_length", "adapter_start_layer"}
    (tmp_path / "lit_config.json").write_text(json.dumps({k: getattr(cfg, k) for k in sorted(base_fields)}))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items() if not spec.is_adapter_key(k)}, tmp_path / "lit_model.pth")
    torch.save({"model": {k: torch.from_numpy(v) for k, v in sd.items() if spec.is_adapter_key(k)}},
               tmp_path / "adapter.pth")
    monkeypatch.setattr(ga, "adapter_start_layer", cfg.adapter_start_layer)
    monkeypatch.setattr(ga, "adapter_prompt_length", cfg.adapter_prompt_length)
    new = 8
    y = ga.main(adapter_path=tmp_path / "adapter.pth", checkpoint_dir=tmp_path, quantize=quantize, max_new_tokens=new,
                temperature=0.0, top_k=None, synthetic="Llama-2-7b-hf", prompt_len=T_PROMPT)
    io = capsys.readouterr()
    assert str(y) in io.out and "Time for inference" in io.err and "tokens/sec" in io.err
    y = torch.tensor(y)
    mode = quantize or "bf16"
    logits = {}
    for dt in (torch.bfloat16, torch.float64):
        ref = _Oracle(cfg, sd, mode, dt)
        ref.set_kv_cache(T_PROMPT + new)
        lg = [ref.forward(y[:T_PROMPT], torch.arange(T_PROMPT))[-1].double()]
        for i in range(new - 1):
            lg.append(ref.forward(y[T_PROMPT + i:T_PROMPT + i + 1], torch.tensor([T_PROMPT + i]))[-1].double())
        logits[dt] = lg
    checked = 0
    for i, (e, b) in enumerate(zip(logits[torch.float64], logits[torch.bfloat16])):
        allowed = (parity.ACC_FACTOR * parity.rel_err(b, e)[0] + parity.ACC_SLACK) * float(e.abs().max())
        top = torch.topk(e, 2).values
        if float(top[0] - top[1]) > 4 * allowed:
            assert int(y[T_PROMPT + i]) == int(e.argmax()), f"token {i} differs from the oracle"
            checked += 1
    assert checked >= 1, "no token had a clear oracle margin"
