"""The fp8 (e4m3) KV cache on the MI355X: the quantizing appends bit for bit against the specification
(tests/kv8_spec.py), decode / window / cached-prefill attention over fp8 caches against an fp64 softmax of what the cache
holds, and the model with ``set_kv_cache(dtype=torch.float8_e4m3fn)`` against the whole-model specification
(``OracleGPT`` + ``Kv8Cache``).

One rule makes every comparison exact where it should be: attention reads K and V as the cache holds them, the call's
own rows included. The dequantized values are exact in bf16 and the scales are powers of two, so the existing decode
and prefill bounds carry over unchanged.
"""

import math

import pytest
import torch

import kv8_spec as spec
from oracle import model as om
from oracle import synth
from parity import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
HS, S = 128, 1024
GEOMS = [(32, 32), (16, 8), (32, 8), (8, 1)]  # 1 / 2 / 4 / 8 heads per query group
SCALE = 1.0 / math.sqrt(HS)
ZERO_ROW, EDGE_ROW = 5, 9  # an all-zero row; a row whose amax is exactly 0.875 * 2^k
# K / V rows are N(0, BASE^2) times the per-row factor 2^((j mod 13) - 6): the largest rows sit at unit scale, where
# the existing decode and prefill bounds were set. (Those bounds are relative to |ref| plus a small absolute term, and
# the prefill kernel's bf16 P costs 2^-9 sum p_i |v_i| whatever the cache format: rows of magnitude 64 would put that
# above the absolute term wherever an output element cancels.)
BASE = 2.0 ** -6
NAN_CODE = 0x7F

_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def _bf16(shape, name, std=1.0):
    key = ("t", shape, name, std)
    if key not in _CACHE:
        _CACHE[key] = torch.from_numpy(synth.normal(shape, name, 5, std)).to(torch.bfloat16)
    return _CACHE[key]


def _rope():
    if "rope" not in _CACHE:
        cos, sin = om.build_rope_cache(S, HS, 10000)
        _CACHE["rope"] = (cos.to(DEV), sin.to(DEV))
    return _CACHE["rope"]


def _rows(G, name):
    """(G, S, HS) bf16 rows on the CPU with a different magnitude per row — row j times 2^((j mod 13) - 6), so a kernel
    that ignores or misindexes a scale is off by a power of two — plus the all-zero row and the 0.875 * 2^k row."""
    key = ("rows", G, name)
    if key not in _CACHE:
        x = _bf16((G, S, HS), f"{name}{G}").float() * BASE
        x = x * torch.exp2((torch.arange(S) % 13 - 6).float()).view(1, S, 1)
        x[:, ZERO_ROW] = 0
        x[:, EDGE_ROW] = x[:, EDGE_ROW].clamp(-0.04, 0.04)
        x[:, EDGE_ROW, 17] = -0.875 * 2.0 ** -4
        _CACHE[key] = x.to(torch.bfloat16)
    return _CACHE[key]


def _filled(G):
    """The test cache of a geometry: CPU (codes, scales, dequantized) of K and V by the specification, computed once."""
    key = ("filled", G)
    if key not in _CACHE:
        _CACHE[key] = (spec.kv8_round(_rows(G, "k")), spec.kv8_round(_rows(G, "v")))
    return _CACHE[key]


def _device_cache(G, valid=S):
    """A fresh device cache holding rows [0, valid) of the test cache; the rows past them are NaN codes and NaN scales."""
    (kc, ks, _), (vc, vs, _) = _filled(G)
    cache = [t.clone() for t in (kc, vc, ks, vs)]
    for c in cache[:2]:
        c[:, valid:] = NAN_CODE
    for s in cache[2:]:
        s[:, valid:] = float("nan")
    return tuple(t.to(DEV) for t in cache)


def _qkv(H, G, rows=8):
    """(rows, (H + 2G) * HS) bf16 on the device; row t's k and v scaled by 2^((t mod 13) - 6), row 2's k and v zero,
    row 4's v with an amax of exactly 0.875 * 2^-8."""
    key = ("qkv", H, G, rows)
    if key not in _CACHE:
        qpk = H // G
        x = _bf16((rows, G, qpk + 2, HS), f"qkv{H}x{G}").float().clone()
        x[:, :, qpk:] *= BASE * torch.exp2((torch.arange(rows) % 13 - 6).float()).view(rows, 1, 1, 1)
        x[2, :, qpk:] = 0
        x[4, :, qpk + 1] = x[4, :, qpk + 1].clamp(-0.003, 0.003)
        x[4, :, qpk + 1, 100] = 0.875 * 2.0 ** -8
        _CACHE[key] = x.reshape(rows, -1).to(torch.bfloat16).to(DEV)
    return _CACHE[key]


def _bf16_append(ops, qkv, pos, H, G):
    """What ``ops.rope_kv_append`` writes for these rows: (q (T, H, HS), k rows (G, T, HS), v rows), all on the CPU."""
    cos, sin = _rope()
    kc = torch.zeros(G, S, HS, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    q = ops.rope_kv_append(qkv, kc, vc, pos, pos, cos, sin, H, G, HS, HS)
    return q.cpu(), kc[:, pos].cpu(), vc[:, pos].cpu()


def _fp64_attention(q, kd, vd, positions, H, G):
    """softmax(q . K[0..p] * scale) . V[0..p] in fp64; q (T, H, HS), kd / vd (G, S, HS) dequantized cache contents."""
    qpk = H // G
    out = torch.empty(len(positions), H, HS, dtype=torch.float64)
    for t, p in enumerate(positions):
        qd = q[t].double().view(G, qpk, HS)
        s = torch.einsum("gqd,gkd->gqk", qd, kd[:, : p + 1].double()) * SCALE
        out[t] = torch.einsum("gqk,gkd->gqd", torch.softmax(s, -1), vd[:, : p + 1].double()).reshape(H, HS)
    return out


def _deq(cache):
    kc, vc, ks, vs = (t.cpu() for t in cache)
    return spec.kv8_dequantize(kc, ks), spec.kv8_dequantize(vc, vs)


# ------------------------------------------------------------------------------------------------ append
@pytest.mark.parametrize("H,G", GEOMS)
def test_kv8_rope_append_bit_exact(ops, H, G):
    """T = 7 rows at scattered positions (S - 1 among them): codes and scales == kv8_round of the rows
    ``ops.rope_kv_append`` writes to a bf16 cache from the same qkv; q == the bf16 path's q; other rows untouched."""
    T = 7
    qkv = _qkv(H, G)[:T].contiguous()
    pos = torch.tensor([3, 0, 500, S - 1, 64, 65, 700], device=DEV)
    cos, sin = _rope()
    cache = (torch.full((G, S, HS), 0xAB, dtype=torch.uint8, device=DEV),
             torch.full((G, S, HS), 0xCD, dtype=torch.uint8, device=DEV),
             torch.full((G, S), 3.0, device=DEV), torch.full((G, S), 5.0, device=DEV))
    q = ops.kv8_rope_append(qkv, cache, pos, pos, cos, sin, H, G, HS, HS)
    q_ref, k_ref, v_ref = _bf16_append(ops, qkv, pos, H, G)
    assert torch.equal(q.cpu(), q_ref)
    kc, vc, ks, vs = (t.cpu() for t in cache)
    p = pos.cpu()
    for codes, scales, ref, name in ((kc, ks, k_ref, "k"), (vc, vs, v_ref, "v")):
        c_ref, s_ref, _ = spec.kv8_round(ref)
        assert torch.equal(scales[:, p], s_ref), name
        assert torch.equal(codes[:, p], c_ref), (name, int((codes[:, p] != c_ref).sum()))
    # the zero row: scale 1, every code a zero (RoPE of zeros leaves some -0)
    assert torch.all(ks[:, p[2]] == 1) and torch.all(kc[:, p[2]] & 0x7F == 0)
    assert torch.all(vs[:, p[2]] == 1) and torch.all(vc[:, p[2]] == 0)
    assert torch.all(vs[:, p[4]] == 2.0 ** -17) and int(vc[0, p[4], 100]) == 0x7E  # 0.875 * 2^-8 = 448 * 2^-17
    rest = torch.ones(S, dtype=torch.bool)
    rest[p] = False
    assert torch.all(kc[:, rest] == 0xAB) and torch.all(vc[:, rest] == 0xCD)
    assert torch.all(ks[:, rest] == 3.0) and torch.all(vs[:, rest] == 5.0)


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("p", [0, 1, 37, 1022, 1023])
@pytest.mark.parametrize("splits", [1, 7, 36])
def test_decode_fused_kv8(ops, H, G, p, splits):
    """One decode row at p over a cache whose rows past p are NaN codes and NaN scales. The appended row's codes and
    scales == kv8_round of the bf16 path's row, nothing else changes, and y is within the decode bound of an fp64
    softmax over the dequantized cache (the new row as stored). p = 37 with 36 splits leaves most splits empty;
    p = 1023 with 1 split runs 4 pipelined steps."""
    r = (3 * p + 2) % 8  # p = 0: the zero k / v row; p = 1022: the 0.875 * 2^k row
    qkv = _qkv(H, G)[r:r + 1].contiguous()
    cache = _device_cache(G, valid=p)
    before = [t.clone() for t in cache]
    pos = torch.tensor([p], device=DEV)
    cos, sin = _rope()
    y = ops.attention_decode_fused_kv8(qkv, cache, pos, pos, cos, sin, H, G, HS, HS, SCALE, n_splits=splits)
    y = y.double().cpu().view(H, HS)
    assert torch.all(torch.isfinite(y))
    q_ref, k_ref, v_ref = _bf16_append(ops, qkv, pos, H, G)
    for i, ref in ((0, k_ref), (1, v_ref)):
        c_ref, s_ref, _ = spec.kv8_round(ref)
        assert torch.equal(cache[i + 2][:, p].cpu(), s_ref[:, 0]), i
        assert torch.equal(cache[i][:, p].cpu(), c_ref[:, 0]), i
    keep = torch.ones(S, dtype=torch.bool)
    keep[p] = False
    for now, was in zip(cache, before):
        assert torch.equal(now[:, keep].view(torch.uint8), was[:, keep].view(torch.uint8))  # (bytes: NaN != NaN)
    kd, vd = _deq(cache)
    ref = _fp64_attention(q_ref, kd, vd, [p], H, G)[0]
    err = float(torch.max((y - ref).abs() - ref.abs() * 2 ** -7))
    print(f"H {H} G {G} p {p} splits {splits}: max(|y - ref| - |ref| 2^-7) = {err:.3e}")
    assert err <= 1e-4


def test_decode_fused_kv8_row_past_the_cache_stores_nothing(ops):
    H, G = 16, 8
    cache = _device_cache(G)
    before = [t.clone() for t in cache]
    pos = torch.tensor([S], device=DEV)
    rope_pos = torch.tensor([S - 1], device=DEV)
    cos, sin = _rope()
    y = ops.attention_decode_fused_kv8(_qkv(H, G)[:1].contiguous(), cache, pos, rope_pos, cos, sin, H, G, HS, HS,
                                       SCALE, n_splits=7)
    assert torch.all(torch.isfinite(y.float()))
    for now, was in zip(cache, before):
        assert torch.equal(now, was)


@pytest.mark.parametrize("splits", [16, 8])
def test_decode_fused_kv8_counters_rearm(ops, splits):
    """Two (and more) successive split launches on one workspace agree, and the counters end at zero."""
    H, G = 32, 32
    cache = _device_cache(G)
    ws = ops.AttentionWorkspace(1, H, G, HS, splits, DEV)
    qkv = _qkv(H, G)[1:2].contiguous()
    cos, sin = _rope()
    outs = []
    for p in (5, 1000, 5, 1000, 1000):  # (a launch rewrites its own row with the same bits)
        pos = torch.tensor([p], device=DEV)
        outs.append(ops.attention_decode_fused_kv8(qkv, cache, pos, pos, cos, sin, H, G, HS, HS, SCALE, splits,
                                                   workspace=ws).clone())
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]) and torch.equal(outs[1], outs[4])
    assert not torch.equal(outs[0], outs[1])
    assert int(ws.counters.abs().sum()) == 0


def test_decode_fused_kv8_graph_replay_equals_eager(ops):
    """A captured decode step replayed over 4 advancing positions: y, codes and scales equal the eager launches'."""
    H, G = 32, 8
    splits = ops.decode_splits(G, H // G, HS, S)
    rows = _qkv(H, G)
    cos, sin = _rope()
    eager = _device_cache(G, valid=600)
    ys = []
    for i in range(4):
        pos = torch.tensor([600 + i], device=DEV)
        ys.append(ops.attention_decode_fused_kv8(rows[i:i + 1].contiguous(), eager, pos, pos, cos, sin, H, G, HS, HS,
                                                 SCALE, splits).clone())
    cache = _device_cache(G, valid=600)
    ws = ops.AttentionWorkspace(1, H, G, HS, splits, DEV)
    qkv = rows[:1].clone()
    pos = torch.tensor([600], device=DEV)
    y = torch.empty(1, H * HS, dtype=torch.bfloat16, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attention_decode_fused_kv8(qkv, cache, pos, pos, cos, sin, H, G, HS, HS, SCALE, splits, workspace=ws, out=y)
    for i in range(4):
        qkv.copy_(rows[i:i + 1])
        pos.fill_(600 + i)
        g.replay()
        assert torch.equal(y, ys[i]), i
    for a, b in zip(cache, eager):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert int(ws.counters.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ window
def _window_case(ops, H, G, M, p0, splits):
    cos, sin = _rope()
    qkv = _qkv(H, G)[:M].contiguous()
    seq = _device_cache(G, valid=p0)
    ws1 = ops.AttentionWorkspace(1, H, G, HS, splits, DEV) if splits > 1 else None
    ys = []
    for r in range(M):
        pos = torch.tensor([p0 + r], device=DEV)
        ys.append(ops.attention_decode_fused_kv8(qkv[r:r + 1], seq, pos, pos, cos, sin, H, G, HS, HS, SCALE, splits,
                                                 workspace=ws1).clone())
    win = _device_cache(G, valid=p0)
    ws = ops.AttentionWorkspace(M, H, G, HS, splits, DEV) if splits > 1 else None
    y = ops.attention_decode_window_kv8(qkv, win, torch.tensor([p0], device=DEV), cos, sin, H, G, HS, HS, SCALE,
                                        splits, workspace=ws)
    for r in range(M):
        assert torch.equal(y[r], ys[r][0]), (p0, r, int((y[r] != ys[r][0]).sum()))
    for a, b in zip(win, seq):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    if ws is not None:
        assert int(ws.counters.abs().sum()) == 0


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("M", [1, 3, 8])
def test_window_kv8_bit_identical_to_one_row_launches(ops, H, G, M):
    """y, codes and scales of a window == M successive one-row launches with the same split count (the production
    count of the geometry), at the start, in the middle and at the end of the cache."""
    for p0 in (0, 100, S - 8):
        _window_case(ops, H, G, M, p0, ops.decode_splits(G, H // G, HS, S))


@pytest.mark.parametrize("splits", [1, 7, 36])
def test_window_kv8_other_split_counts(ops, splits):
    for p0 in (0, 100, S - 8):
        _window_case(ops, 32, 8, 8, p0, splits)


# ------------------------------------------------------------------------------------------------ prefill, dequantize
@pytest.mark.parametrize("H,G", [(16, 8), (8, 1)])
@pytest.mark.parametrize("T,start", [(16, 0), (100, 0), (40, 110)])
def test_prefill_through_the_fp8_cache(ops, H, G, T, start):
    """The cached prefill's three launches — quantizing append, dequantize into a bf16 pair, the MFMA flash attention
    over that pair — against fp64 over the dequantized cache, the existing prefill bound. T = 40 from 110 attends rows
    written earlier."""
    cos, sin = _rope()
    (kc, ks, _), (vc, vs, _) = _filled(G)
    cache = [t.clone() for t in (kc, vc, ks, vs)]
    for c in cache[:2]:
        c[:, start:] = 0
    for s in cache[2:]:
        s[:, start:] = 1
    cache = tuple(t.to(DEV) for t in cache)
    rows = _qkv(H, G, rows=128)[:T].contiguous()
    pos = torch.arange(start, start + T, device=DEV)
    q = ops.kv8_rope_append(rows, cache, pos, pos, cos, sin, H, G, HS, HS)
    kd, vd = ops.kv8_dequantize(cache)
    y = ops.attention(q, kd, vd, pos, H, G, HS, SCALE, 1).double().cpu().view(T, H, HS)
    ck, cv = _deq(cache)
    assert torch.equal(kd.float().cpu(), ck) and torch.equal(vd.float().cpu(), cv)
    q_ref, k_ref, v_ref = _bf16_append(ops, rows, pos, H, G)
    assert torch.equal(ck[:, start:start + T], spec.kv8_round(k_ref)[2])
    ref = _fp64_attention(q_ref, ck, cv, list(range(start, start + T)), H, G)
    err = float(torch.max((y - ref).abs() - ref.abs() * 2 ** -6))
    print(f"H {H} G {G} T {T} start {start}: max(|y - ref| - |ref| 2^-6) = {err:.3e}")
    assert err <= 5e-3


@pytest.mark.parametrize("G,n", [(8, S), (8, 37), (1, 1), (32, 1000)])
def test_kv8_dequantize_bit_exact(ops, G, n):
    """lga_kv8_dequantize == codes.view(float8_e4m3fn).float() * scale, bit for bit (every code byte occurs)."""
    (kc, ks, _), (vc, vs, _) = _filled(G)
    kc = kc.clone()
    every = torch.arange(256, dtype=torch.uint8)
    kc[0, 0, :] = every[:128]
    kc[0, 1 % S, :] = every[128:]
    kc[kc == 0x7F] = 0x7E  # NaN bit patterns are not compared
    kc[kc == 0xFF] = 0xFE
    cache = tuple(t.to(DEV) for t in (kc, vc, ks, vs))
    kd, vd = ops.kv8_dequantize(cache, n)
    assert kd.shape == vd.shape == (G, n, HS) and kd.dtype == torch.bfloat16
    for got, codes, scales in ((kd, kc, ks), (vd, vc, vs)):
        ref = spec.kv8_dequantize(codes[:, :n], scales[:, :n]).to(torch.bfloat16)
        assert torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))


# ------------------------------------------------------------------------------------------------ model
S_MAX = 96
T_PROMPT, N_DECODE = 33, 16
MODELS = [("int4-g128", 8), ("int4-g128", 2), ("bf16", 8)]  # (weights, query groups of 8 heads)
ROWS_MODELS = MODELS[:2]  # the multi-row decode steps stream 4-bit weights


def _model(mode, groups):
    from generate.base import build_model
    from lit_gpt import Config

    key = ("model", mode, groups)
    if key not in _CACHE:
        cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=groups,
                               intermediate_size=2816)
        _CACHE[key] = build_model(cfg, quantize=None if mode == "bf16" else mode, device=torch.device(DEV),
                                  max_seq_length=S_MAX)
    return _CACHE[key]


def _set_cache(model, fp8, B=1):
    model.set_kv_cache(batch_size=B, device=torch.device(DEV), dtype=FP8 if fp8 else None)


def _prompt(vocab, T):
    return torch.from_numpy(synth.token_ids(T, vocab, seed=20 + T)).to(DEV)


def _run(model, prompt, n, tokens=None):
    """Prefill + n one-token steps (eager); greedy, or teacher-forced on ``tokens``. Returns (logits per step, tokens)."""
    T = prompt.numel()
    logits, toks = [], []
    with torch.inference_mode():
        lg = model(prompt.view(1, -1), torch.arange(T, device=DEV), last_token_only=True).view(-1)
        for i in range(n + 1):
            logits.append(lg.float().cpu())
            toks.append(int(tokens[i]) if tokens is not None else int(torch.argmax(lg.float())))
            if i < n:
                lg = model(torch.tensor([[toks[-1]]], device=DEV), torch.tensor([T + i], device=DEV)).view(-1)
    return logits, toks


def _bf16_run(mode, groups):
    """The bf16-cache run every model test starts from, once per model: logits, tokens and layer 0's cache."""
    key = ("bf16run", mode, groups)
    if key not in _CACHE:
        model = _model(mode, groups)
        _set_cache(model, False)
        logits, toks = _run(model, _prompt(model.config.vocab_size, T_PROMPT), N_DECODE)
        kv = model.transformer.h[0].attn.kv_cache
        _CACHE[key] = (logits, toks, kv.k[0].cpu(), kv.v[0].cpu())
    return _CACHE[key]


@pytest.mark.parametrize("mode,groups", MODELS)
def test_model_layer0_cache_bit_exact_and_switch(mode, groups):
    """Prefill (33 tokens) + 16 decode steps with a bf16 cache, and again with an fp8 cache fed the same tokens: layer
    0's K / V do not depend on the cache, so its codes and scales == kv8_round of layer 0's bf16 rows (the prefill
    append and the fused decode append end to end). The fp8 logits differ from the bf16-cache ones, the cache holds
    0.516 x the bytes, and a bf16-cache run afterwards repeats the first one bit for bit."""
    model = _model(mode, groups)
    prompt = _prompt(model.config.vocab_size, T_PROMPT)
    logits, toks, k0, v0 = _bf16_run(mode, groups)
    bytes_bf16 = sum(b.numel() * b.element_size() for blk in model.transformer.h for b in blk.attn.kv_cache.buffers())
    _set_cache(model, True)
    kv = model.transformer.h[0].attn.kv_cache
    assert kv.cache_dtype == FP8 and kv.k.dtype == torch.uint8
    bytes_fp8 = sum(b.numel() * b.element_size() for blk in model.transformer.h for b in blk.attn.kv_cache.buffers())
    assert bytes_fp8 * 256 == bytes_bf16 * 132
    got, _ = _run(model, prompt, N_DECODE, tokens=toks)
    n = T_PROMPT + N_DECODE
    for codes, scales, ref, name in ((kv.k, kv.k_scale, k0, "k"), (kv.v, kv.v_scale, v0, "v")):
        c_ref, s_ref, _ = spec.kv8_round(ref[:, :n])
        assert torch.equal(scales[0, :, :n].cpu(), s_ref), name
        assert torch.equal(codes[0, :, :n].cpu(), c_ref), (name, int((codes[0, :, :n].cpu() != c_ref).sum()))
        assert torch.all(codes[0, :, n:] == 0) and torch.all(scales[0, :, n:] == 1)
    kd, vd = kv.dequantized()
    assert torch.equal(kd[:, :n].float().cpu(), spec.kv8_round(k0[:, :n])[2])
    assert torch.equal(got[0], logits[0]) is False and not any(torch.equal(a, b) for a, b in zip(got, logits))
    _set_cache(model, False)
    again, toks2 = _run(model, prompt, N_DECODE)
    assert toks2 == toks and all(torch.equal(a, b) for a, b in zip(again, logits))


@pytest.mark.parametrize("mode,groups", MODELS)
def test_model_logits_follow_the_fp8_specification(mode, groups):
    """Teacher-forced logits of the fp8-cache model against ``OracleGPT`` + ``Kv8Cache`` on the dequantized weights, in
    float64 and in bf16. Quantization is discontinuous: two correct bf16 evaluations round some K / V elements to
    different codes, so the bound is relative to R, the bf16 specification's own largest max-relative distance to the
    float64 one over the run (a second bf16 evaluation with K / V moved by one bf16 ulp lands up to 1.41 R from the
    float64 oracle and 1.20 R from the bf16 one; the factor 2 is that plus a margin of about 1.4)."""
    from test_gpu_geometry import oracle_state_from_model

    model = _model(mode, groups)
    prompt = _prompt(model.config.vocab_size, T_PROMPT)
    _set_cache(model, True)
    got, toks = _run(model, prompt, N_DECODE)
    _set_cache(model, False)
    sd = oracle_state_from_model(model)
    refs = {}
    for dt in (torch.float64, torch.bfloat16):
        og = om.OracleGPT(model.config, sd, dtype=dt, rope_pos_dtype=torch.bfloat16)
        og.set_kv_cache(S_MAX)
        og.cache = spec.Kv8Cache(k=og.cache.k, v=og.cache.v)
        out = [og.forward(prompt.cpu(), torch.arange(T_PROMPT), last_only=True)[-1].double()]
        for i in range(N_DECODE):
            out.append(og.forward(torch.tensor([toks[i]]), torch.tensor([T_PROMPT + i]))[-1].double())
        refs[dt] = out
    exact, bf = refs[torch.float64], refs[torch.bfloat16]
    R = max(rel_err(b, e)[0] for b, e in zip(bf, exact))
    R_rms = max(rel_err(b, e)[1] for b, e in zip(bf, exact))
    worst = [0.0, 0.0, 0.0, 0.0]
    checked = 0
    for i, (g, b, e) in enumerate(zip(got, bf, exact)):
        e_max, e_rms, e_abs = rel_err(g, e)
        b_max, b_rms, _ = rel_err(g, b)
        worst = [max(w, x) for w, x in zip(worst, (e_max, e_rms, b_max, b_rms))]
        assert e_max <= 2 * R and e_rms <= 2 * R, (i, e_max, e_rms, R)
        assert b_max <= 2 * R and b_rms <= 2 * R, (i, b_max, b_rms, R)
        top2 = torch.topk(e, 2).values
        if float(top2[0] - top2[1]) > 4 * e_abs:
            assert toks[i] == int(torch.argmax(e)), i
            checked += 1
    print(f"\n{mode} G={groups}: R = {R:.3%} (rms {R_rms:.3%}); product vs float64 max {worst[0] / R:.2f} R, rms "
          f"{worst[1] / R:.2f} R ({worst[1] / R_rms:.2f} R_rms); vs bf16 oracle max {worst[2] / R:.2f} R, rms "
          f"{worst[3] / R:.2f} R; {checked} of {len(got)} greedy tokens checked")
    assert checked >= 1


def test_model_fp8_graph_equals_eager():
    from generate.base import generate

    model = _model("int4-g128", 2)
    prompt = _prompt(model.config.vocab_size, 16)
    outs = []
    for use_graph in (True, False):
        _set_cache(model, True)
        outs.append(generate(model, prompt, 16 + 24, temperature=0.0, use_graph=use_graph).cpu())
    assert torch.equal(outs[0], outs[1])
    _set_cache(model, False)


@pytest.mark.parametrize("mode,groups", ROWS_MODELS)
def test_generate_batch_fp8_equals_generate_fp8(ops, mode, groups):
    """Batched decode is unchanged in kind: three prompts batched over an fp8 cache get, token for token, what
    ``generate`` gives each alone over an fp8 cache; one batched step's logits equal the single-sequence logits bit
    for bit."""
    from generate.base import generate, generate_batch

    model = _model(mode, groups)
    prompts = [_prompt(model.config.vocab_size, T) for T in (5, 16, 33)]
    new = 24
    single, steps = [], []
    for p in prompts:
        _set_cache(model, True)
        single.append(generate(model, p, p.numel() + new, temperature=0.0).cpu())
    with torch.inference_mode():
        for p in prompts:
            _set_cache(model, True)
            T = p.numel()
            pre = model(p.view(1, -1), torch.arange(T, device=DEV), last_token_only=True)
            tok = ops.argmax(pre.view(-1).contiguous()).to(torch.int32)
            steps.append((tok, model(tok.view(1, 1), torch.tensor([T], device=DEV)).clone()))
        _set_cache(model, True, B=3)
        for b, p in enumerate(prompts):
            model(p.view(1, -1), torch.arange(p.numel(), device=DEV), last_token_only=True, kv_slot=b)
        logits = model(torch.cat([s[0] for s in steps]).view(-1, 1),
                       torch.tensor([p.numel() for p in prompts], device=DEV))
        for b in range(3):
            assert torch.equal(logits[b], steps[b][1][0]), b
    _set_cache(model, True)
    outs = generate_batch(model, prompts, new, temperature=0.0)
    assert model.transformer.h[0].attn.kv_cache.cache_dtype == FP8  # the batch cache keeps the format
    assert model.transformer.h[0].attn.kv_cache.k.size(0) == 3
    for b in range(3):
        assert torch.equal(outs[b].cpu(), single[b]), b
    _set_cache(model, False)


@pytest.mark.parametrize("mode,groups", ROWS_MODELS)
def test_generate_speculative_fp8_equals_generate_fp8(mode, groups):
    """Speculative decoding is unchanged in kind: the n-gram drafter at gamma = 4 on an fp8 target cache gives the
    tokens of ``generate`` with an fp8 cache."""
    from generate.base import generate
    from generate.speculative import NgramDrafter, generate_speculative

    model = _model(mode, groups)
    prompt = _prompt(model.config.vocab_size, 9).repeat(4)
    _set_cache(model, True)
    ref = generate(model, prompt, prompt.numel() + 24, temperature=0.0).cpu()
    _set_cache(model, True)
    stats = {}
    y = generate_speculative(model, prompt, prompt.numel() + 24, NgramDrafter(3), speculate=4, stats=stats)
    assert torch.equal(y.cpu(), ref)
    assert stats["proposed"] > 0
    _set_cache(model, False)


def test_build_model_kv_cache_fp8(ops):
    from generate.base import build_model, generate
    from lit_gpt import Config

    cfg = Config.from_name("Llama-2-7b-hf", n_layer=1, n_embd=256, n_head=2, n_query_groups=1, intermediate_size=512,
                           vocab_size=1000, padding_multiple=64, block_size=64)
    model = build_model(cfg, quantize="bnb.int8", device=torch.device(DEV), max_seq_length=32, kv_cache="fp8")
    kv = model.transformer.h[0].attn.kv_cache
    assert kv.cache_dtype == FP8 and kv.k.dtype == torch.uint8 and kv.k_scale.shape == (1, 1, 32)
    y = generate(model, _prompt(cfg.vocab_size, 8), 20, temperature=0.0)
    assert y.numel() == 20 and torch.any(kv.k[0, :, :19] != 0) and torch.all(kv.k[0, :, 19:] == 0)
    with pytest.raises(NotImplementedError, match="head_size"):
        build_model(Config.from_name("Llama-2-7b-hf", n_layer=1, n_embd=128, n_head=2, intermediate_size=256,
                                     vocab_size=1000, padding_multiple=64, block_size=64),
                    quantize=None, device=torch.device(DEV), max_seq_length=32, kv_cache="fp8")


def test_perplexity_kv_cache_flag(monkeypatch):
    """eval/perplexity.py: ``--kv_cache bf16`` prints what no flag prints, bit for bit; ``--kv_cache fp8`` scores each
    window as a prefill through an fp8 cache — finite, and different."""
    from eval import perplexity
    from lit_gpt import Config

    small = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=2,
                             intermediate_size=2816)

    class Registry:
        from_name = staticmethod(lambda name: small)

    monkeypatch.setattr(perplexity, "Config", Registry)
    kw = dict(synthetic="Llama-2-7b-hf", n_tokens=200, max_seq_length=64, quantize="int4-g128", min_context=8)
    plain = perplexity.main(**kw)
    bf16 = perplexity.main(kv_cache="bf16", **kw)
    fp8 = perplexity.main(kv_cache="fp8", **kw)
    for key in ("tokens", "nll", "ppl", "windows"):
        assert plain[key] == bf16[key], key
    assert fp8["tokens"] == plain["tokens"] == 200 and fp8["windows"] == plain["windows"] > 1
    assert math.isfinite(fp8["nll"]) and math.isfinite(fp8["ppl"]) and fp8["nll"] != plain["nll"]
    assert abs(fp8["nll"] - plain["nll"]) < 0.05 * plain["nll"]  # the same model: a perturbation, not another answer
    print(f"nll {plain['nll']:.4f} (no cache) vs {fp8['nll']:.4f} (fp8 cache)")
