"""CPU-side checks of the fp8 (e4m3) KV cache: the format's specification (tests/kv8_spec.py), the ``KVCache`` fp8
form, every refusal, the ``--kv_cache`` flags and the argument validation of the four C entry points."""

import ctypes
import functools
import re
from pathlib import Path

import pytest
import torch

import kv8_spec as spec

REPO = Path(__file__).resolve().parent.parent
FP8 = torch.float8_e4m3fn
NEW_SYMBOLS = ["lga_attention_decode_fused_kv8", "lga_attention_decode_window_kv8", "lga_kv8_rope_append",
               "lga_kv8_dequantize"]


# ------------------------------------------------------------------------------------------------ the specification
def _rows(n=4096, seed=0):
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(torch.empty(n, 1).uniform_(-13.8, 13.8, generator=g))  # 1e-6 .. 1e6
    return (torch.randn(n, 128, generator=g) * mag).to(torch.bfloat16).float()


def test_scale_is_a_power_of_two_and_rows_fill_the_top_binade():
    x = _rows()
    codes, s, deq = spec.kv8_round(x)
    m, _ = torch.frexp(s)
    assert torch.all(m == 0.5)
    r = x.abs().amax(-1) / s
    assert torch.all((r > 224) & (r <= 448)), (float(r.min()), float(r.max()))
    assert not torch.isnan(deq).any() and int((codes & 0x7F).max()) <= 0x7E  # no NaN code, nothing past 448
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)  # exact in bf16
    rel = ((deq - x).pow(2).sum(-1) / x.pow(2).sum(-1)).sqrt()
    assert 0.02 < float(rel.mean()) < 0.035  # Gaussian rows: 2.7 % rms


@pytest.mark.parametrize("k", [-20, -1, 0, 5, 40])
def test_scale_boundaries(k):
    """m = 0.875 exactly takes the smaller scale (amax / s = 448); one bf16 ulp above takes the next."""
    at = torch.tensor(0.875 * 2.0 ** k)
    above = torch.tensor((0.875 + 2.0 ** -8) * 2.0 ** k)  # bf16: 8 significant bits, m in [0.5, 1) steps by 2^-8
    assert above.to(torch.bfloat16).float() == above
    assert float(spec.kv8_scale(at)) == 2.0 ** (k - 9) and float(at / spec.kv8_scale(at)) == 448.0
    assert float(spec.kv8_scale(above)) == 2.0 ** (k - 8)
    assert float(spec.kv8_scale(torch.tensor(0.5 * 2.0 ** k))) == 2.0 ** (k - 9)
    row = torch.zeros(128)
    row[7] = -at
    codes, s, deq = spec.kv8_round(row)
    assert int(codes[7]) == 0xFE and float(deq[7]) == -float(at)


def test_zero_row_and_idempotence():
    codes, s, deq = spec.kv8_round(torch.zeros(3, 128))
    assert torch.all(codes == 0) and torch.all(s == 1) and torch.all(deq == 0)
    x = _rows(512, seed=1)
    c1, s1, d1 = spec.kv8_round(x)
    c2, s2, d2 = spec.kv8_round(d1)
    # Re-quantizing what the cache gives back returns the same VALUES for every row. Codes and scale repeat too,
    # with the one exception the scale rule itself creates: a row whose largest element lay in (224 s, 232 s] rounds
    # down to 224 s = 0.875 * 2^k exactly, where the rule takes the next smaller scale (224 s / (s / 2) = 448) — the
    # same values, one exponent step up in every code.
    assert torch.equal(d1, d2)
    top = d1.abs().amax(-1) / s1
    moved = top == 224
    assert torch.all(top >= 224) and 0 < int(moved.sum()) < moved.numel() // 8
    assert torch.equal(c1[~moved], c2[~moved]) and torch.equal(s1[~moved], s2[~moved])
    assert torch.equal(s2[moved], s1[moved] / 2)
    assert torch.equal(spec.kv8_dequantize(c1, s1), d1) and torch.equal(spec.kv8_dequantize(c2, s2), d1)


# ------------------------------------------------------------------------------------------------ KVCache
def _cfg(**kw):
    from lit_gpt import Config

    base = dict(n_layer=2, n_embd=1024, n_head=8, n_query_groups=2, intermediate_size=256, vocab_size=512,
                padding_multiple=64, block_size=64)
    base.update(kw)
    return Config.from_name("Llama-2-7b-hf", **base)


def test_fp8_kv_cache_shapes_dtypes_and_bytes():
    from lit_gpt import GPT
    from lit_gpt.model import KVCache

    model = GPT(_cfg()).to(torch.bfloat16)
    model.max_seq_length = 48
    model.set_kv_cache(3, dtype=FP8)
    kv = model.transformer.h[1].attn.kv_cache
    assert isinstance(kv, KVCache) and kv.cache_dtype == FP8 and kv.fp8
    assert kv.k.shape == kv.v.shape == (3, 2, 48, 128) and kv.k.dtype == kv.v.dtype == torch.uint8
    assert kv.k_scale.shape == kv.v_scale.shape == (3, 2, 48) and kv.k_scale.dtype == torch.float32
    assert torch.all(kv.k == 0) and torch.all(kv.k_scale == 1) and torch.all(kv.v_scale == 1)
    nbytes = sum(b.numel() * b.element_size() for b in kv.buffers())
    assert nbytes == 3 * 2 * 48 * 2 * 132  # 132 B per K row and per V row
    assert set(kv.state_dict()) == set()  # non-persistent, as the bf16 cache
    # the scratch pair of the cached prefill: one for the whole model
    assert model.transformer.h[0].attn.kv_cache.scratch[0] is kv.scratch[0] and kv.scratch[0].shape == (2, 48, 128)
    kv.k.fill_(0x38)  # 1.0
    kv.v.fill_(0xC0)  # -2.0
    kv.k_scale.fill_(0.25)
    k, v = kv.dequantized(slot=2)
    assert k.dtype == torch.bfloat16 and k.shape == (2, 48, 128)
    assert torch.all(k == 0.25) and torch.all(v == -2.0)
    kv.reset_parameters()
    assert torch.all(kv.k == 0) and torch.all(kv.v == 0) and torch.all(kv.k_scale == 1)
    with pytest.raises(NotImplementedError, match="quantizing kernels"):
        kv(torch.tensor([0]), torch.zeros(3, 2, 1, 128), torch.zeros(3, 2, 1, 128))
    # the bf16 cache is what it was, plus the attribute callers read instead of k.dtype
    model.set_kv_cache(1)
    kv = model.transformer.h[0].attn.kv_cache
    assert kv.cache_dtype == torch.bfloat16 and not kv.fp8 and kv.k.dtype == torch.bfloat16
    assert [n for n, _ in kv.named_buffers()] == ["k", "v"]


def test_fp8_kv_cache_refusals(monkeypatch):
    from lit_gpt import GPT, comm

    with pytest.raises(NotImplementedError, match="head_size"):  # 64-dim heads
        GPT(_cfg(n_embd=512)).to(torch.bfloat16).set_kv_cache(1, dtype=FP8)
    with pytest.raises(NotImplementedError, match="heads per query group"):  # 3 heads per group
        GPT(_cfg(n_embd=768, n_head=6, n_query_groups=2)).to(torch.bfloat16).set_kv_cache(1, dtype=FP8)
    with pytest.raises(NotImplementedError, match="heads per query group"):  # partial rotary
        GPT(_cfg(rotary_percentage=0.25)).to(torch.bfloat16).set_kv_cache(1, dtype=FP8)
    model = GPT(_cfg())
    with pytest.raises(NotImplementedError, match="32-true"):  # fp32 model
        model.set_kv_cache(1, dtype=FP8)
    assert model.transformer.h[0].attn.kv_cache is None  # refused before anything was built
    model = model.to(torch.bfloat16)
    monkeypatch.setattr(comm, "get_default", lambda: object())
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        model.set_kv_cache(1, dtype=FP8)
    monkeypatch.undo()
    model.transformer.h[1].attn.register_forward_hook(
        functools.partial(comm.all_reduce_output, 2))  # generate/tp.py's hook
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        model.set_kv_cache(1, dtype=FP8)


def test_build_model_kv_cache_argument():
    from generate.base import KV_CACHE_DTYPES, build_model

    assert KV_CACHE_DTYPES == {"bf16": None, "fp8": FP8}
    dev = torch.device("cpu")  # every refusal comes before a weight is materialised
    with pytest.raises(ValueError, match="kv_cache"):
        build_model(_cfg(), quantize=None, device=dev, kv_cache="int8")
    with pytest.raises(NotImplementedError, match="kv_cache fp8"):
        build_model(_cfg(), quantize=None, device=dev, dtype=torch.float32, kv_cache="fp8")

    class Fabric:
        world_size, global_rank = 2, 0

    with pytest.raises(NotImplementedError, match="kv_cache fp8"):
        build_model(_cfg(), quantize="int4-g128", device=dev, fabric=Fabric(), kv_cache="fp8")


@pytest.mark.parametrize("module,extra", [("generate.base", ["--batch_size", "2"]), ("chat.base", []),
                                           ("generate.speculative", ["--draft", "ngram"]),
                                           ("eval.perplexity", ["--synthetic", "Llama-2-7b-hf"])])
def test_cli_kv_cache_flag(monkeypatch, module, extra):
    import importlib

    mod = importlib.import_module(module)
    seen = {}
    monkeypatch.setattr(mod, "main", lambda *a, **kw: seen.update(kw))
    mod._cli(extra + ["--kv_cache", "fp8"])
    assert seen["kv_cache"] == "fp8"
    mod._cli(extra)
    assert seen["kv_cache"] == "bf16"
    with pytest.raises(SystemExit):
        mod._cli(extra + ["--kv_cache", "int4"])


@pytest.mark.parametrize("module", ["generate.tp", "generate.sequentially"])
def test_tp_and_sequential_entry_points_have_no_kv_cache_flag(module):
    text = (REPO / "lit-gpt_amd" / (module.replace(".", "/") + ".py")).read_text()
    assert "--kv_cache" not in text


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_and_bindings():
    from lit_gpt import ops

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "litgpt_amd.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(lga_[a-z0-9_]+)\s*\(", text))
    lib = ops.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared and name in ops.SIGNATURES and hasattr(lib, name), name


def test_kv8_argument_validation_without_gpu():
    """Null, shape and range errors come back through lga_last_error_string before any launch."""
    from lit_gpt import ops

    lib = ops.load_library()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused first

    def fused(n_head=8, G=2, hs=128, ne=128, S=64, splits=1, ws=None, rope_rows=64, qkv=p):
        return lib.lga_attention_decode_fused_kv8(qkv, p, p, p, p, p, p, p, p, rope_rows, p, ws, ws, n_head, G, hs, ne,
                                                  S, splits, 0.1, None)

    def window(M=2, n_head=8, G=2, hs=128, ne=128, S=64, splits=1, ws=None, scales=p):
        return lib.lga_attention_decode_window_kv8(p, p, p, scales, scales, p, p, p, 64, p, ws, ws, M, n_head, G, hs,
                                                   ne, S, splits, 0.1, None)

    def err():
        return lib.lga_last_error_string()

    assert fused(qkv=None) != 0 and b"null" in err()
    assert lib.lga_attention_decode_fused_kv8(p, p, p, None, p, p, p, p, p, 64, p, None, None, 8, 2, 128, 128, 64, 1,
                                              0.1, None) != 0 and b"null" in err()  # a missing scale array
    assert fused(G=3) != 0 and b"geometry" in err()
    assert fused(hs=64, ne=64) != 0 and b"128" in err()
    assert fused(ne=32) != 0 and b"128" in err()
    assert fused(n_head=6) != 0 and b"q_per_kv" in err()
    assert fused(S=0) != 0 and b"empty" in err()
    assert fused(rope_rows=0) != 0 and b"empty" in err()
    assert fused(splits=0) != 0 and b"n_splits" in err()
    assert fused(splits=257, ws=p) != 0 and b"n_splits" in err()
    assert fused(splits=4) != 0 and b"workspace" in err()

    assert window(scales=None) != 0 and b"null" in err()
    for M in (0, 9):
        assert window(M=M) != 0 and b"[1, 8]" in err()
    assert window(hs=64) != 0 and b"128" in err()
    assert window(n_head=32, G=2) != 0 and b"q_per_kv" in err()
    assert window(splits=8) != 0 and b"workspace" in err()

    def append(T=4, n_head=8, G=2, hs=128, ne=128, S=64, q_out=p):
        return lib.lga_kv8_rope_append(p, q_out, p, p, p, p, p, p, p, p, 64, T, n_head, G, hs, ne, S, None)

    assert append(q_out=None) != 0 and b"null" in err()
    assert append(T=0) != 0 and b"geometry" in err()
    assert append(n_head=7) != 0 and b"geometry" in err()
    assert append(hs=64, ne=64) != 0 and b"128" in err()
    assert append(ne=64) != 0 and b"128" in err()
    assert append(S=0) != 0 and b"empty" in err()

    def deq(G=2, n=8, hs=128, S=64, out=p):
        return lib.lga_kv8_dequantize(p, p, p, p, out, p, G, n, hs, S, None)

    assert deq(out=None) != 0 and b"null" in err()
    assert deq(hs=64) != 0 and b"128" in err()
    assert deq(n=0) != 0 and b"max_seq" in err()
    assert deq(n=65) != 0 and b"max_seq" in err()
    assert deq(G=0) != 0 and b"max_seq" in err()


_DECODE_SYMBOLS = [f"lga_attention_decode_{form}{kv8}" for form in ("fused", "window", "batch") for kv8 in ("", "_kv8")]
# (word in lga_last_error_string(), argument overrides, the symbols the case applies to: a substring of the name)
_DECODE_REFUSALS = [
    ("null", dict(qkv=None), ""),
    ("null", dict(y=None), ""),
    ("null", dict(k_scale=None), "_kv8"),
    ("geometry", dict(G=3), ""),                    # G does not divide n_head = 8
    ("128", dict(hs=64, ne=64), ""),
    ("head_size", dict(hs=64, ne=64), ""),
    ("128", dict(ne=32), ""),
    ("q_per_kv", dict(n_head=6), ""),               # 3 heads per group
    ("empty", dict(S=0), ""),
    ("empty", dict(rope_rows=0), ""),
    ("n_splits", dict(splits=0), ""),
    ("n_splits", dict(splits=257, ws=True), ""),
    ("workspace", dict(splits=4), ""),
    ("[1, 8]", dict(rows=0), "window"),
    ("[1, 8]", dict(rows=9), "window"),
    ("[1, 8]", dict(rows=0), "batch"),
    ("[1, 8]", dict(rows=9), "batch"),
    ("slot_stride", dict(slot_stride=2 * 64 * 128 - 1), "batch"),
    ("scale_slot_stride", dict(scale_slot_stride=2 * 64 - 1), "batch_kv8"),
]


@pytest.mark.parametrize("symbol,word,over", [(s, w, o) for s in _DECODE_SYMBOLS for w, o, only in _DECODE_REFUSALS
                                              if only in s])
def test_decode_attention_entry_points_refuse_before_any_launch(symbol, word, over):
    """Every lga_attention_decode_* entry point makes the same argument checks, names itself in the message and returns
    before anything is dereferenced or launched (the pointers are never valid)."""
    from lit_gpt import ops

    lib = ops.load_library()
    p = ctypes.c_void_p(256)
    a = dict(qkv=p, k_scale=p, y=p, ws=False, rows=2, slot_stride=2 * 64 * 128, scale_slot_stride=2 * 64, n_head=8,
             G=2, hs=128, ne=128, S=64, rope_rows=64, splits=1)
    assert set(over) <= set(a)
    a.update(over)
    ws = p if a["ws"] else None
    args = [a["qkv"], p, p] + ([a["k_scale"], p] if symbol.endswith("_kv8") else []) + [p]  # qkv, caches, position(s)
    if "window" not in symbol:
        args.append(p)  # rope_pos
    args += [p, p, a["rope_rows"], a["y"], ws, ws]
    if "fused" not in symbol:
        args.append(a["rows"])
    if "batch" in symbol:
        args += [a["slot_stride"]] + ([a["scale_slot_stride"]] if symbol.endswith("_kv8") else []) + [None]  # active
    args += [a["n_head"], a["G"], a["hs"], a["ne"], a["S"], a["splits"], 0.1, None]
    assert len(args) == len(ops.SIGNATURES[symbol])
    lib.lga_set_error(b"")
    assert getattr(lib, symbol)(*args) != 0
    err = lib.lga_last_error_string()
    assert err.startswith(symbol.encode() + b": ") and word.encode() in err, err


def test_ops_wrappers_check_the_cache_layout():
    from lit_gpt import ops

    cache = (torch.zeros(2, 8, 128, dtype=torch.uint8), torch.zeros(2, 8, 128, dtype=torch.uint8),
             torch.ones(2, 8), torch.ones(2, 8))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.kv8_dequantize(cache)
    bad = (cache[0], cache[1], torch.ones(2, 9), torch.ones(2, 9))
    with pytest.raises(ValueError, match="fp8 cache"):
        ops.kv8_dequantize(bad)
    with pytest.raises(ValueError, match="exactly one token"):
        ops.attention_decode_fused_kv8(torch.zeros(2, 1536, dtype=torch.bfloat16), cache, None, None, None, None, 8, 2,
                                       128, 128, 0.1)
    with pytest.raises(ValueError, match="1 <= M <= 8"):
        ops.attention_decode_window_kv8(torch.zeros(9, 1536, dtype=torch.bfloat16), cache, None, None, None, 8, 2, 128,
                                        128, 0.1)
