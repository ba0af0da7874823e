"""LoRA on the MI355X: the lga_lora_* kernels against tests/lora_spec.py, the LoraLinear dispatch, the fixture models
end to end (eager and through the decode graph, merged and at run time) and generate/lora.py.

Kernel tolerance (per element, built as test_gpu_kernels.py test_gemv_fused_norm_residual_bias builds its own): the
reference is the float64 evaluation of the chain WITH the bf16 rounding points applied; the kernel may round each of
them the other way, so 2^-7 of every quantity that is rounded to bf16 on the way — |y|, |bf16(p + l)|, |l| (its two
roundings, u and u * scaling), and scaling * sum_j |B_nj| |t_j| for the rounding of t — plus that test's 2e-3 floor.
"""

import dataclasses
import json

import numpy as np
import pytest
import torch

import int8_spec
import lora_spec as spec
import parity
from oracle import quant, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SHAPES = [(77, 1376), (1000, 256), (12288, 4096), (4096, 11008)]  # (N, K)
RANKS = [(8, 1), (8, 2), (8, 3), (16, 1), (16, 2), (16, 3), (64, 1), (64, 2), (64, 3)]  # (r, R / r)


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


@pytest.fixture(scope="module")
def g6():
    from pathlib import Path

    return np.load(Path(__file__).resolve().parent / "golden" / "g6_lora.npz", allow_pickle=False)


def _bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep float64 (CPU)."""
    return t.to(torch.bfloat16).double()


def _dev(t):
    return None if t is None else t.to(torch.bfloat16).to(DEV).contiguous()


_CASES = {}


def _case(N, K, r, segs, M=1):
    """Seeded operands (bf16 values in float64): x (M, K), norm weight, A (R, K), B (N, r), row_off (segs > 1: the rows
    dealt to the segments in blocks of 5, every 7th block without adapter; segs == 1: None), base, residual."""
    key = (N, K, r, segs, M)
    if key not in _CASES:
        _CASES.clear()  # one case at a time: the largest is 300 x 12288 doubles several times over
        g = torch.Generator().manual_seed(N * 31 + K * 7 + r * 3 + segs + 1000 * M)
        rnd = lambda *s, std=1.0: _bf(torch.randn(*s, generator=g, dtype=torch.float32) * std)  # noqa: E731
        block = torch.arange(N) // 5
        off = None if segs == 1 else torch.where(block % 7 == 6, -1, (block % segs) * r).to(torch.int32)
        _CASES[key] = dict(x=rnd(M, K), nw=_bf(1.0 + torch.randn(K, generator=g) * 0.2), A=rnd(r * segs, K, std=K ** -0.5),
                           B=rnd(N, r, std=0.05), off=off, base=rnd(M, N), res=rnd(M, N), scaling=16.0 / r)
    return _CASES[key]


def _reference(c, x, base, res, with_parts=False):
    parts = {}
    y = spec.chain(x, c["A"], c["B"], c["off"], c["scaling"], base=base, residual=res, rnd=_bf, parts=parts)
    tol = 2.0 ** -7 * (y.abs() + parts["pre_residual"].abs() + parts["l"].abs() + c["scaling"] * parts["mag"]) + 2e-3
    return (y, tol, parts) if with_parts else (y, tol)


def _ulp(v: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 (8 significant bits) at |v|."""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


def _rows_dot(B, vec, off):
    """(N,): sum_j B[n, j] * vec[off_n + j] (0 on rows without adapter)."""
    r = B.shape[1]
    o = torch.zeros(B.shape[0], dtype=torch.int64) if off is None else off.long()
    idx = o.clamp(min=0)[:, None] + torch.arange(r)[None, :]
    return torch.where(o >= 0, (B * vec[idx]).sum(-1), torch.zeros(B.shape[0], dtype=B.dtype))


def _check(got, ref, tol, what):
    err = (got.double().cpu() - ref).abs()
    worst = float((err - tol).max())
    print(f"{what}: max error {float(err.max()):.3e}, worst error - tolerance {worst:.3e}")
    assert worst <= 0, f"{what}: error exceeds the tolerance by {worst:.3e}"


# ------------------------------------------------------------------------------------------------ lga_lora_gemv
@pytest.mark.parametrize("r,segs", RANKS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_lora_gemv_matches_the_chain(ops, N, K, r, segs):
    c = _case(N, K, r, segs)
    A, B, off = _dev(c["A"]), _dev(c["B"]), None if c["off"] is None else c["off"].to(DEV)
    x, nw, base, res = _dev(c["x"]), _dev(c["nw"]), _dev(c["base"][0]), _dev(c["res"][0])
    xn = spec.rms_norm(c["x"], c["nw"], 1e-5, rnd=_bf)
    kw = dict(norm_weight=nw, eps=1e-5)
    # norm + base + residual, into a fresh y; the same with y aliasing base: bit-identical
    ref, tol = _reference(c, xn, c["base"], c["res"])
    y = ops.lora_gemv(x, A, B, off, c["scaling"], base=base, residual=res, **kw)
    _check(y, ref[0], tol[0], "norm+base+res")
    alias = base.clone()
    assert ops.lora_gemv(x, A, B, off, c["scaling"], base=alias, residual=res, out=alias, **kw) is alias
    assert torch.equal(alias, y)
    # no norm, no base, no residual: y = l
    ref, tol = _reference(c, c["x"], None, None)
    l = ops.lora_gemv(x, A, B, off, c["scaling"])
    _check(l, ref[0], tol[0], "plain")
    # base alone, residual alone (no norm)
    yb = ops.lora_gemv(x, A, B, off, c["scaling"], base=base)
    ref, tol = _reference(c, c["x"], c["base"], None)
    _check(yb, ref[0], tol[0], "base")
    ref, tol = _reference(c, xn, None, c["res"])
    _check(ops.lora_gemv(x, A, B, off, c["scaling"], residual=res, **kw), ref[0], tol[0], "norm+res")
    # bit-exact: base = NULL followed by lga_add is the base form
    assert torch.equal(ops.add(base, l), yb)
    if c["off"] is not None:
        has = (c["off"] >= 0).to(DEV)
        # rows with offset -1 return base (+ residual) unchanged, and l = 0 there
        assert torch.equal(yb[~has], base[~has]) and not l[~has].any()
        assert torch.equal(y[~has], ops.add(base, res)[~has])
    # B = 0 returns base
    assert torch.equal(ops.lora_gemv(x, A, torch.zeros_like(B), off, c["scaling"], base=base, **kw), base)


def test_lora_gemv_does_not_depend_on_the_grid(ops):
    """Every workgroup computes t itself, in an order independent of the rows it owns: rows of the same segment give
    the same bits wherever they sit in the output."""
    N, K, r = 4096, 4096, 8
    c = _case(N, K, r, 1)
    x, A = _dev(c["x"]), _dev(c["A"])
    B = _dev(c["B"][:16].repeat(N // 16, 1))  # the same 16 rows of B in every workgroup
    y = ops.lora_gemv(x, A, B, None, c["scaling"])
    assert torch.equal(y.view(-1, 16), y[:16].expand(N // 16, 16))


# ------------------------------------------------------------------------------------------------ prefill pair
@pytest.mark.parametrize("r,segs", RANKS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_lora_down_up_match_the_chain_and_the_gemv_rows(ops, N, K, r, segs):
    A = B = off = None
    for M in (2, 65, 300):
        c = _case(N, K, r, segs, M)
        A, B, off = _dev(c["A"]), _dev(c["B"]), None if c["off"] is None else c["off"].to(DEV)
        x, base, res = _dev(c["x"]), _dev(c["base"]), _dev(c["res"])
        t = ops.lora_down(x, A)
        assert t.shape == (M, r * segs)
        y = ops.lora_up(t, B, off, c["scaling"], base=base, residual=res)
        ref, tol = _reference(c, c["x"], c["base"], c["res"])
        _check(y, ref, tol, f"M={M} base+res")
        alias = base.clone()
        ops.lora_up(t, B, off, c["scaling"], base=alias, residual=res, out=alias)
        assert torch.equal(alias, y)
        ref, tol = _reference(c, c["x"], None, None)
        _check(ops.lora_up(t, B, off, c["scaling"]), ref, tol, f"M={M} plain")
        # t against the reference's: one bf16 ulp (it may round the other way) plus what fp32 accumulation in another
        # order can move the sum before it is rounded — worst case (chain length) x 2^-24 x sum_k |x_k| |A_jk|, the
        # chain being K / 16 MFMA steps and the 16 products inside one; without this term a t_j that cancels to almost
        # nothing would be held to an ulp of its own tiny value
        ref, tol, parts = _reference(c, c["x"], c["base"], c["res"], with_parts=True)
        t_step = _ulp(parts["t"]) + (K / 16 + 16) * 2.0 ** -24 * (c["x"].abs() @ c["A"].abs().T)
        dt = (t.double().cpu() - parts["t"]).abs()
        assert bool((dt <= t_step).all()), f"M={M}: t is {float((dt / t_step).max()):.2f} x its bound off"
        # row m of the M-row result against lga_lora_gemv on row m alone: each kernel's t_j is within that step of the
        # reference's (both sum in fp32, in different orders), so the two are up to two steps apart, and u, l and the two sums after it may then round one step the
        # other way: one bf16 ulp at each rounding point — ulp(y) + ulp(p + l) + 2 ulp(l) + scaling * sum_j |B_nj|
        # step(t_j), magnitudes taken from the reference chain
        for m in sorted({0, M // 2, M - 1}):
            ym = ops.lora_gemv(x[m], A, B, off, c["scaling"], base=base[m], residual=res[m]).double().cpu()
            tmag = _rows_dot(c["B"].abs(), 2 * t_step[m], c["off"])
            bound = (_ulp(ref[m]) + _ulp(parts["pre_residual"][m]) + 2 * _ulp(parts["l"][m]) + c["scaling"] * tmag)
            d = (y[m].double().cpu() - ym).abs()
            assert bool((d <= bound).all()), f"M={M} row {m}: {float((d - bound).max()):.3e} past the one-ulp bound"


# ------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("r,segs", [(8, 1), (8, 2), (16, 3), (64, 3)])
@pytest.mark.parametrize("N,K", SHAPES)
def test_lora_merge_matches_the_merged_product(ops, N, K, r, segs):
    """lga_bf16_gemv over the merged weight against the float64 product x (W + scaling * B A)^T, with the existing bf16
    GEMV test's tolerance (test_gpu_kernels.py test_bf16_gemv_matches_reference) plus what the merge's own three bf16
    roundings (B A, its scaling, the sum) can add: element (n, k) of the merged weight is off by at most
    e_nk = 2^-9 (2 |delta_nk| + |W_nk + delta_nk|); the roundings of different elements are independent, so their sum
    sum_k x_k err_nk stays within 6 sqrt(sum_k (x_k e_nk)^2) (Hoeffding: 2 exp(-18) per output row).
    The merged weight itself: within one bf16 ulp at each of its three roundings of the specification's, bit-equal on all but 2e-3 of the
    elements (fp32 against float64 sums of r <= 64 products straddle a bf16 rounding boundary with probability about
    sqrt(r) 2^-24 / 2^-9 per rounding), and bit-identical to the input on rows without adapter."""
    c = _case(N, K, r, segs)
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    Wd = W.to(DEV)
    assert ops.lora_merge(Wd, _dev(c["A"]), _dev(c["B"]), None if c["off"] is None else c["off"].to(DEV),
                          c["scaling"]) is Wd
    Wk = Wd.cpu()
    off = torch.zeros(N, dtype=torch.int64) if c["off"] is None else c["off"].long()
    assert torch.equal(Wk[off < 0], W[off < 0])
    x, s = c["x"][0], c["scaling"]
    y = ops.bf16_gemv(_dev(x), Wd).double().cpu()
    ref, spread = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    differing = 0
    for n0 in range(0, N, 2048):
        rows = torch.arange(n0, min(n0 + 2048, N))
        delta = torch.zeros(rows.numel(), K, dtype=torch.float64)
        for o in torch.unique(off[rows][off[rows] >= 0]).tolist():
            sel = off[rows] == o
            delta[sel] = c["B"][rows[sel]] @ c["A"][o:o + r]
        w = W[rows].double()
        merged = torch.where((off[rows] >= 0)[:, None], _bf(w + _bf(_bf(delta) * s)), w)  # the specification
        d = (Wk[rows].double() - merged).abs()
        ulp = s * _ulp(delta) + _ulp(s * delta) + _ulp(merged)  # one step at each of the three roundings
        assert bool((d <= ulp).all()), f"rows {n0}..: merged weight {float((d - ulp).max()):.3e} past one bf16 ulp"
        differing += int((d > 0).sum())
        exact = w + s * delta
        ref[rows] = exact @ x
        e = 2.0 ** -9 * (2 * (s * delta).abs() + exact.abs())
        spread[rows] = ((e * x[None, :]) ** 2).sum(-1).sqrt()
    assert differing <= 2e-3 * N * K, f"{differing} of {N * K} merged elements differ from the specification"
    tol = ref.abs() * 2 ** -7 + 1e-3 * np.sqrt(K / 4096) * 0.02 * float(x.abs().mean()) * 4 + 6 * spread
    err = (y - ref).abs()
    print(f"merge {N}x{K} r={r} segs={segs}: max error {float(err.max()):.3e}, {differing} elements off the spec bits")
    assert bool((err <= tol).all()), float((err - tol).max())


# ------------------------------------------------------------------------------------------------ dispatch
MODES = ["int4-g128", "nf4", "bnb.int8", "bf16"]


def _state(key, g6):
    """The fixture model's state (base + adapter), rounded to bf16 as the device model holds it."""
    return {k: int8_spec.bf16_round(v) for k, v in spec.fixture_state(key, g6).items()}


def build_gpu_model(cfg, sd, mode, max_seq):
    from lit_gpt import GPT
    from lit_gpt.quantize import QuantizedPrecision

    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if "lora_" not in k})
    model = model.to(device=DEV, dtype=torch.bfloat16)
    if mode != "bf16":
        QuantizedPrecision(mode).convert_module(model, DEV)
    model.max_seq_length = max_seq
    model.set_kv_cache(1, device=DEV)
    return model.eval()


def _adapter(sd, zero_b=False):
    return {k: torch.from_numpy(np.zeros_like(v) if zero_b and k.endswith("lora_B") else v) for k, v in sd.items()
            if "lora_" in k}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_lora_linear_with_zero_b_equals_its_base(g6, key, mode):
    from lit_gpt import lora
    from lit_gpt.model import _lin

    cfg = spec.lora_config(key)
    sd = _state(key, g6)
    model = build_gpu_model(cfg, sd, mode, 32)
    lora.attach(model, _adapter(sd, zero_b=True), cfg)
    adapted = [m for m in model.modules() if isinstance(m, lora.LoraLinear)]
    assert len(adapted) == cfg.n_layer * (1 if key == "mha" else 5) + int(cfg.to_head)
    g = torch.Generator().manual_seed(5)
    for m in adapted[:5] + adapted[-1:]:
        nw = (1.0 + 0.2 * torch.randn(m.in_features, generator=g)).to(torch.bfloat16).to(DEV)
        for M in (1, 5):
            x = torch.randn(1, M, m.in_features, generator=g).to(torch.bfloat16).to(DEV)
            res = torch.randn(1, M, m.out_features, generator=g).to(torch.bfloat16).to(DEV)
            for kw in (dict(), dict(residual=res), dict(norm_weight=nw, norm_eps=1e-5),
                       dict(residual=res, norm_weight=nw, norm_eps=1e-5)):
                assert torch.equal(m(x, **kw), _lin(m.base, x, **kw)), (type(m.base).__name__, M, sorted(kw))


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
def test_one_lora_gemv_per_adapted_linear_per_decode_step_and_no_torch_matmul(g6, key, mode, monkeypatch):
    from torch.utils._python_dispatch import TorchDispatchMode

    from lit_gpt import lora, ops

    cfg = spec.lora_config(key)
    sd = _state(key, g6)
    model = build_gpu_model(cfg, sd, mode, 32)
    lora.attach(model, _adapter(sd), cfg)
    n_adapted = sum(isinstance(m, lora.LoraLinear) for m in model.modules())
    rec = Recorder(ops)
    monkeypatch.setattr(ops, "_lib", rec)
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func.__name__)
            return func(*args, **(kwargs or {}))

    idx = torch.from_numpy(g6[f"{key}/prompt"]).to(DEV)
    with Watch():
        model(idx[:8].view(1, -1), torch.arange(8, device=DEV))
        prefill, rec.calls = rec.calls, []
        model(idx[8:9].view(1, 1), torch.tensor([8], device=DEV))
    matmuls = [f for f in seen if any(s in f for s in ("mm", "matmul", "linear", "einsum", "dot"))]
    assert not matmuls, matmuls
    decode = rec.calls
    assert decode.count("lga_lora_gemv") == n_adapted and "lga_lora_down" not in decode and "lga_lora_up" not in decode
    assert prefill.count("lga_lora_down") == prefill.count("lga_lora_up") == n_adapted and "lga_lora_gemv" not in prefill
    # two launches per adapted Linear in a decode step: the base's GEMV, then the adapter's
    gemv = {"int4-g128": "lga_q4_gemv", "nf4": "lga_q4_gemv", "bnb.int8": "lga_int8_gemv", "bf16": "lga_bf16_gemv"}[mode]
    for i, name in enumerate(decode):
        if name == "lga_lora_gemv":
            assert decode[i - 1] == gemv, decode[max(0, i - 2):i + 1]
    if key == "gqa":  # an adapted fc_1 / fc_2 pair: two Linears + lga_swiglu, no dual launch; an adapted head: no
        assert not any("swiglu" in n and n != "lga_swiglu" for n in decode)  # fused argmax head either
        assert decode.count("lga_swiglu") == cfg.n_layer and "lga_q4_gemv_argmax_embed" not in decode


# ------------------------------------------------------------------------------------------------ model
class _Oracle(spec.LoraOracle):
    """LoraOracle over the base the device model holds: the dequantized 4-bit weight (or the bf16 weight) through
    ``weight_override``; for bnb.int8, whose Linear also quantizes its input, the int8 specification's Linear."""

    def __init__(self, lcfg, sd, mode, dtype):
        def deq(k, v):
            if "lora_" in k or not (k.endswith(".weight") and v.ndim == 2) or k.startswith("transformer.wte"):
                return v
            if mode == "int4-g128":
                return quant.dequantize_q4g(*quant.quantize_q4g(v, 128), 128)
            if mode == "nf4":
                return quant.dequantize_fmt(*quant.quantize_fmt(v, 1, 64), 1, 64)
            return v

        super().__init__(lcfg, sd, dtype=dtype, weight_override=deq)
        self.mode, self.q8 = mode, {}

    def _base_lin(self, prefix, x):
        if self.mode != "bnb.int8":
            return super()._base_lin(prefix, x)
        if prefix not in self.q8:
            self.q8[prefix] = int8_spec.quantize_weight(self.p[f"{prefix}.weight"].float().numpy())
        q, s = self.q8[prefix]
        xn = x.float().numpy()
        if self.dtype == torch.bfloat16:
            return torch.from_numpy(int8_spec.linear(xn, q, s)).to(torch.bfloat16)
        return torch.from_numpy(int8_spec.linear_exact(xn, q, s))


T_PROMPT, N_DECODE = 12, 8


def _teacher_forced(forward, prompt, stream):
    out = [forward(prompt, torch.arange(T_PROMPT))]
    for i in range(N_DECODE):
        out.append(forward(stream[i:i + 1], torch.tensor([T_PROMPT + i])))
    return out


def _oracle_logits(ref, prompt, stream):
    ref.set_kv_cache(T_PROMPT + N_DECODE + 1)
    return _teacher_forced(lambda idx, pos: ref.forward(idx, pos)[-1], prompt, stream)


def _gpu_logits(model, prompt, stream):
    for b in model.transformer.h:
        b.attn.kv_cache.reset_parameters()
    return _teacher_forced(lambda idx, pos: model(idx.view(1, -1).to(DEV), pos.to(DEV))[0, -1].float().cpu(), prompt,
                           stream)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_model_teacher_forced_logits_eager_graph_and_merged(g6, key, mode, monkeypatch):
    """12-token prefill + 8 teacher-forced decode steps against the spec oracle in bf16 and float64 (tests/parity.py);
    the decode graph bit for bit equal to eager; for the bf16 base the merged model under the same bounds, with plain
    nn.Linears again; and the adapter moves the argmax of at least one step by more than check_step's margin rule."""
    from lit_gpt import lora
    from lit_gpt import ops as ops_mod
    from lit_gpt.runtime import DecodeGraph

    cfg = spec.lora_config(key)
    sd = _state(key, g6)
    prompt = torch.from_numpy(g6[f"{key}/prompt"])
    stream = torch.from_numpy(synth.token_ids(N_DECODE, cfg.vocab_size, seed=22))
    model = build_gpu_model(cfg, sd, mode, T_PROMPT + N_DECODE + 1)
    lora.attach(model, _adapter(sd), cfg)
    got = _gpu_logits(model, prompt, stream)
    exp = {dt: _oracle_logits(_Oracle(cfg, sd, mode, dt), prompt, stream) for dt in (torch.bfloat16, torch.float64)}
    errs = [parity.check_step(g, exp[torch.bfloat16][i], exp[torch.float64][i], f"lora {key} {mode} step {i}")
            for i, g in enumerate(got)]
    # the adapter matters: against the float64 oracle WITHOUT the adapter, some step's argmax differs, and at that
    # step the adapted oracle's top-1 margin exceeds 4 x the product's error (check_step then pinned the token)
    base_sd = {k: v for k, v in sd.items() if "lora_" not in k}
    plain = _oracle_logits(_Oracle(cfg, base_sd, mode, torch.float64), prompt, stream)
    moved = 0
    for i, (a, p) in enumerate(zip(exp[torch.float64], plain)):
        top = torch.topk(a.double(), 2).values
        clear = float(top[0] - top[1]) > 4 * errs[i] * float(a.abs().max())
        if clear and int(a.argmax()) != int(p.argmax()):
            assert int(got[i].argmax()) == int(a.argmax()) != int(p.argmax())
            moved += 1
    assert moved >= 1, "the adapter never moved a clear argmax: the test would pass without it"
    # decode graph == eager, bit for bit: the 8 forced decode steps again through DecodeGraph (step 0 eager, the rest
    # replays); the logits are the tensor handed to the step's argmax launch (the fused 4-bit head keeps dg.logits)
    handed = []
    for name in ("argmax_embed", "argmax"):
        orig = getattr(ops_mod, name)
        monkeypatch.setattr(ops_mod, name, lambda lg, *a, _o=orig, **k: (handed.append(lg), _o(lg, *a, **k))[1])
    for b in model.transformer.h:
        b.attn.kv_cache.reset_parameters()
    model(prompt.view(1, -1).to(DEV), torch.arange(T_PROMPT, device=DEV))
    dg = DecodeGraph(model, stream[0:1].to(DEV), T_PROMPT)
    buf = dg.logits if getattr(dg, "logits", None) is not None else handed[-1]  # the captured step's logits buffer
    for i in range(1, N_DECODE):
        dg.token.fill_(int(stream[i]))
        dg.x_emb.copy_(model.transformer.wte.weight[int(stream[i])])
        dg.step()
        assert int(dg.pos) == T_PROMPT + i + 1
        assert torch.equal(buf.float().cpu().view(-1), got[1 + i]), f"{key} {mode}: graph step {i} differs from eager"
    if mode == "bf16":
        lora.merge_lora_weights(model)
        assert not any(isinstance(m, lora.LoraLinear) for m in model.modules())
        assert type(model.transformer.h[0].attn.attn) is torch.nn.Linear and type(model.lm_head) is torch.nn.Linear
        for i, g in enumerate(_gpu_logits(model, prompt, stream)):
            parity.check_step(g, exp[torch.bfloat16][i], exp[torch.float64][i], f"lora {key} merged step {i}")


@pytest.mark.parametrize("mode", ["int4-g128", "bf16"])
@pytest.mark.parametrize("key", ["mha", "gqa"])
@torch.inference_mode()
def test_generate_graph_equals_eager(g6, key, mode):
    from generate.base import generate
    from lit_gpt import lora

    cfg = spec.lora_config(key)
    sd = _state(key, g6)
    model = build_gpu_model(cfg, sd, mode, T_PROMPT + 12)
    lora.attach(model, _adapter(sd), cfg)
    prompt = torch.from_numpy(g6[f"{key}/prompt"]).to(DEV)

    def run(use_graph):
        for b in model.transformer.h:
            b.attn.kv_cache.reset_parameters()
        return generate(model, prompt, T_PROMPT + 12, temperature=0.0, use_graph=use_graph).cpu()

    assert torch.equal(run(True), run(False))


def test_merge_refuses_a_quantized_base(g6):
    from lit_gpt import lora

    cfg = spec.lora_config("mha")
    sd = _state("mha", g6)
    model = build_gpu_model(cfg, sd, "int4-g128", 16)
    lora.attach(model, _adapter(sd), cfg)
    with pytest.raises(NotImplementedError, match="quantize again"):
        lora.merge_lora_weights(model)
    assert isinstance(model.transformer.h[0].attn.attn, lora.LoraLinear)


# ------------------------------------------------------------------------------------------------ entry point
@pytest.mark.parametrize("quantize,merge", [(None, None), ("int4-g128", None), (None, False)],
                         ids=["bf16-merged", "int4-run-time", "bf16-run-time"])
@torch.inference_mode()
def test_generate_lora_entry_point_follows_the_oracle(g6, tmp_path, monkeypatch, capsys, quantize, merge):
    """generate/lora.py --synthetic on a checkpoint + adapter written here: greedy tokens equal to the spec oracle's
    greedy loop wherever the oracle's margin is clear (tests/test_gpu_model.py's rule: 3 % of the logit scale)."""
    import generate.lora as gl

    key = "mha"
    cfg = spec.lora_config(key)
    sd = _state(key, g6)
    base_fields = {f.name for f in dataclasses.fields(cfg)} - set(spec.MODELS[key]["lora"]) - {"dropout"}
    (tmp_path / "lit_config.json").write_text(json.dumps({k: getattr(cfg, k) for k in sorted(base_fields)}))
    torch.save({k: torch.from_numpy(v) for k, v in sd.items() if "lora_" not in k}, tmp_path / "lit_model.pth")
    torch.save({"model": _adapter(sd)}, tmp_path / "adapter.pth")
    for name, v in dict(lora_r=cfg.r, lora_alpha=cfg.alpha, lora_query=True, lora_key=False, lora_value=True,
                        lora_projection=False, lora_mlp=False, lora_head=False).items():
        monkeypatch.setattr(gl, name, v)
    new = 8
    y = gl.main(lora_path=tmp_path / "adapter.pth", checkpoint_dir=tmp_path, quantize=quantize, max_new_tokens=new,
                temperature=0.0, top_k=None, merge=merge, synthetic="Llama-2-7b-hf", prompt_len=T_PROMPT)
    assert str(y) in capsys.readouterr().out
    y = torch.tensor(y)
    mode = quantize or "bf16"
    ref = _Oracle(cfg, sd, mode, torch.bfloat16)
    ref.set_kv_cache(T_PROMPT + new)
    logits = [ref.forward(y[:T_PROMPT], torch.arange(T_PROMPT))[-1].float()]
    for i in range(new - 1):
        logits.append(ref.forward(y[T_PROMPT + i:T_PROMPT + i + 1], torch.tensor([T_PROMPT + i]))[-1].float())
    checked = 0
    for i, lg in enumerate(logits):
        top = torch.topk(lg, 2).values
        if float(top[0] - top[1]) > 0.03 * float(lg.abs().max()):
            assert int(y[T_PROMPT + i]) == int(lg.argmax()), f"token {i} differs from the oracle"
            checked += 1
    assert checked >= new // 2, f"only {checked} of {new} tokens had a clear oracle margin"


def test_generate_lora_refuses_before_building_the_model(monkeypatch, tmp_path):
    import generate.lora as gl

    def boom(*a, **kw):
        raise AssertionError("the model was built before the refusal")

    monkeypatch.setattr(gl, "build_model", boom)
    with pytest.raises(NotImplementedError, match="32-true"):
        gl.main(synthetic="Llama-2-7b-hf", precision="32-true", checkpoint_dir=tmp_path)
    with pytest.raises(NotImplementedError, match="--merge"):
        gl.main(synthetic="Llama-2-7b-hf", quantize="nf4", merge=True, checkpoint_dir=tmp_path)
    monkeypatch.setattr(gl, "lora_mlp", True)
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        gl.main(synthetic="Mixtral-8x7B-v0.1", checkpoint_dir=tmp_path)
