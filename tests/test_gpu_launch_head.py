"""The launch heads of the decode kernels. The one-row GEMV entry points take their leading arguments as scalars
(preloaded into SGPRs on gfx950: x, norm weight, both weight / scale pairs, N, and K and the group packed in one word)
with the rest of ``GemvArgs`` as a trailing struct; the routed-expert launches moved to a by-value kernel of their own.
Nothing arithmetic changed, so these cases aim at what an argument re-plumbing can get wrong — a swapped or dropped
pointer, a wrong N / K / group / codebook row, a position frozen at capture — at the smallest shapes that still run the
clamped tail rows and every epilogue combination. The decode-attention cases (every form, RoPE row != cache row, a graph
replayed over a moving position) guard the same kind of change to the attention head, which was measured and is not in
the product. The references and the bounds are those of tests/test_gpu_kernels.py (and
tests/test_gpu_kv8.py for the fp8 cache) for the same entry points.
"""

import itertools
import math

import numpy as np
import pytest
import torch

import kv8_spec as spec
from oracle import model as om
from oracle import quant, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, K = 40, 512  # 40 rows: not a multiple of the 8 / 16 rows of a workgroup, so clamped tail rows run
FORMATS = [(0, 128), (1, 64), (3, 64)]  # int4-g128, nf4, fp4 (codebook row cb = 1)
HS, S = 128, 96
SCALE = 1.0 / math.sqrt(HS)
GEOMS = [(4, 4), (8, 2)]
POSITIONS = [0, 1, 63, 95]

_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def bf16_np(x):
    return quant.bf16_bits_to_f32(quant.f32_to_bf16_bits(np.ascontiguousarray(x, dtype=np.float32)))


def to_dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(torch.bfloat16)


def _weight(name, fmt, group, n=N, k=K):
    """(fp32 weight, its oracle dequantization, device (qweight, scales)), computed once per (name, format)."""
    key = (name, fmt, group, n, k)
    if key not in _CACHE:
        w = synth.normal((n, k), f"lh_{name}", 5, 0.02)
        deq = quant.dequantize_fmt(*quant.quantize_fmt(w, fmt, group), fmt, group)
        from lit_gpt import ops as _ops

        _CACHE[key] = (w, deq, _ops.quantize(torch.from_numpy(w).to(DEV), fmt, group))
    return _CACHE[key]


def _ref_linear(x, wdeq):
    return x.astype(np.float64) @ wdeq.astype(np.float64).T


def _normed(x, nw):
    return om.rms_norm(torch.from_numpy(x).bfloat16(), torch.from_numpy(nw).bfloat16(), 1e-5).float().numpy()


# ------------------------------------------------------------------------------------------------ GEMV
@pytest.mark.parametrize("fmt,group", FORMATS)
@pytest.mark.parametrize("variant", [-1, 4])  # one-shot and streaming entry points
@pytest.mark.parametrize("norm,res,bias", list(itertools.product([False, True], repeat=3)))
def test_gemv_every_epilogue_combination(ops, fmt, group, variant, norm, res, bias):
    """bf16(x' W^T + bias) + residual with x' = RMSNorm(x) or x, each of the three present or absent (the bound of
    test_gemv_fused_norm_residual_bias; distinct O(1) vectors, so a swapped or missing pointer is far outside it)."""
    _, deq, (qw, sc) = _weight("w", fmt, group)
    x = bf16_np(synth.normal((K,), "lh_x", 5, 2.0))
    nw = bf16_np(1.0 + synth.normal((K,), "lh_nw", 5, 0.2))
    rv = bf16_np(synth.normal((N,), "lh_res", 5, 1.0))
    bv = bf16_np(3.0 + synth.normal((N,), "lh_bias", 5, 0.1))
    y = ops.q4_gemv(to_dev_bf16(x), qw, sc, N, K, group, fmt, bias=to_dev_bf16(bv) if bias else None,
                    residual=to_dev_bf16(rv) if res else None, norm_weight=to_dev_bf16(nw) if norm else None,
                    eps=1e-5, variant=variant).float().cpu().numpy()
    h = _ref_linear(_normed(x, nw) if norm else x, deq) + (bv if bias else 0.0)
    h = bf16_np(h.astype(np.float32))
    ref = h + (rv if res else 0.0)
    err = float(np.max(np.abs(y - ref) - np.abs(ref) * 2 ** -7 - np.abs(h) * 2 ** -7))
    print(f"fmt {fmt} variant {variant} norm {norm} res {res} bias {bias}: {err:.3e}")
    assert err <= 2e-3


@pytest.mark.parametrize("fmt,group", FORMATS)
@pytest.mark.parametrize("variant", [0, 4])  # one-shot, streaming
@pytest.mark.parametrize("norm", [False, True])
def test_gemv_swiglu_both_forms(ops, fmt, group, variant, norm):
    """silu(x' W1^T) * (x' W2^T) with two different matrices (the bound of test_gemv_swiglu)."""
    _, d1, (q1, s1) = _weight("s1", fmt, group)
    _, d2, (q2, s2) = _weight("s2", fmt, group)
    x = bf16_np(synth.normal((K,), "lh_xs", 5, 1.0))
    nw = bf16_np(1.0 + synth.normal((K,), "lh_nws", 5, 0.2))
    y = ops.q4_gemv_swiglu(to_dev_bf16(x), q1, s1, q2, s2, N, K, group, fmt,
                           norm_weight=to_dev_bf16(nw) if norm else None, variant=variant).float().cpu().numpy()
    xn = _normed(x, nw) if norm else x
    a, b = _ref_linear(xn, d1), _ref_linear(xn, d2)
    ref = (a / (1 + np.exp(-a))) * b
    err = float(np.max(np.abs(y - ref) - np.abs(ref) * 2 ** -6))
    print(f"fmt {fmt} variant {variant} norm {norm}: {err:.3e}")
    assert err <= 1e-3


@pytest.mark.parametrize("mode", ["int4-g128", "nf4", "bnb.fp4"])
def test_fused_head_small_vocabulary(ops, mode):
    """lga_q4_gemv_argmax_embed at V = 96 == lga_q4_gemv(norm) then lga_argmax_embed, bit for bit (the criterion of
    test_fused_greedy_head_bit_identical): logits, token, index, position and embedding row."""
    from lit_gpt.quantize import QuantLinear

    V = 96
    g = torch.Generator().manual_seed(V + K)
    lin = QuantLinear.from_float(torch.randn(V, K, generator=g) * 0.02, None, mode, torch.device(DEV))
    nw = (1.0 + torch.randn(K, generator=g) * 0.1).bfloat16().to(DEV)
    table = torch.randn(V, 64, generator=g).bfloat16().to(DEV)
    work = ops.HeadWorkspace(V, K, DEV)
    for it in range(3):
        x = (torch.randn(K, generator=g) * 2).bfloat16().to(DEV)
        la = ops.q4_gemv(x, lin.qweight, lin.scales, V, K, lin.group, lin.fmt, norm_weight=nw)
        ia, ta, pa = (torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                      torch.tensor([40 + it], device=DEV))
        ea = torch.empty(64, dtype=torch.bfloat16, device=DEV)
        ops.argmax_embed(la, table, ea, out_idx=ia, token_out=ta, pos_inout=pa)
        ib, tb, pb = torch.zeros_like(ia), torch.zeros_like(ta), torch.tensor([40 + it], device=DEV)
        eb = torch.empty_like(ea)
        lb = ops.q4_gemv_argmax_embed(x, lin, work, norm_weight=nw, table=table, emb_out=eb, out_idx=ib,
                                      token_out=tb, pos_inout=pb)
        assert torch.equal(la, lb) and int(ia) == int(ib) and int(ta) == int(tb) and int(pa) == int(pb) == 41 + it
        assert torch.equal(ea, eb)
    assert int(work.buf[-(9 * 256) // 8:].abs().sum()) == 0  # counters re-armed


@pytest.mark.parametrize("fmt,group", FORMATS)
def test_routed_experts_two_slots_of_four(ops, fmt, group):
    """The routed launches (their own by-value kernel now): slot s == the plain GEMV on expert ids[s]'s weights, bit
    for bit (test_routed_expert_gemvs_equal_per_expert_gemvs), for the SwiGLU pair with a norm and the plain form with
    one activation row per slot."""
    E = 4
    qs = [_weight(f"e{e}", fmt, group)[2] for e in range(E)]
    qs2 = [_weight(f"f{e}", fmt, group)[2] for e in range(E)]
    ids = torch.tensor([3, 1], dtype=torch.int32, device=DEV)
    x = to_dev_bf16(synth.normal((K,), "lh_xe", 5, 1.0))
    nw = to_dev_bf16(1.0 + 0.1 * synth.normal((K,), "lh_nwe", 5, 1.0))
    act = ops.q4_gemv_swiglu_experts(x, torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs]),
                                     torch.stack([q for q, _ in qs2]), torch.stack([s for _, s in qs2]), ids, N, K,
                                     group, fmt, norm_weight=nw)
    for s, e in enumerate((3, 1)):
        ref = ops.q4_gemv_swiglu(x, qs[e][0], qs[e][1], qs2[e][0], qs2[e][1], N, K, group, fmt, norm_weight=nw)
        assert torch.equal(act[s], ref)
    xs = to_dev_bf16(synth.normal((2, K), "lh_xe2", 5, 1.0))
    out = ops.q4_gemv_experts(xs, torch.stack([q for q, _ in qs]), torch.stack([s for _, s in qs]), ids, N, K, group,
                              fmt)
    for s, e in enumerate((3, 1)):
        assert torch.equal(out[s], ops.q4_gemv(xs[s].contiguous(), qs[e][0], qs[e][1], N, K, group, fmt))


# ------------------------------------------------------------------------------------------------ attention
def _rope():
    if "rope" not in _CACHE:
        cos, sin = om.build_rope_cache(S, HS, 10000)
        _CACHE["rope"] = (cos.to(DEV), sin.to(DEV))
    return _CACHE["rope"]


def _rope_pos(p):
    """A RoPE row different from the cache row p (and from every other case's), inside the 96-row table."""
    return (7 * p + 5) % S


def _qkv(H, G, rows=3):
    key = ("qkv", H, G, rows)
    if key not in _CACHE:
        _CACHE[key] = to_dev_bf16(synth.normal((rows, (H + 2 * G) * HS), f"lh_q{H}x{G}", 7, 1.0))
    return _CACHE[key]


def _kv(G, name="kv"):
    key = (name, G)
    if key not in _CACHE:
        _CACHE[key] = (to_dev_bf16(synth.normal((G, S, HS), f"lh_k{name}{G}", 7, 1.0)),
                       to_dev_bf16(synth.normal((G, S, HS), f"lh_v{name}{G}", 7, 1.0)))
    return _CACHE[key]


def _fp64_attention(q, kd, vd, p, H, G):
    """softmax(q . K[0..p] * scale) . V[0..p] in fp64; q (H, HS), kd / vd (G, S, HS)."""
    qpk = H // G
    ref = torch.empty(H, HS, dtype=torch.float64)
    for h in range(H):
        s = kd[h // qpk, : p + 1].double() @ q[h].double() * SCALE
        ref[h] = torch.softmax(s, 0) @ vd[h // qpk, : p + 1].double()
    return ref


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("splits", [1, 8])
def test_attention_fused_rope_row_differs_from_cache_row(ops, H, G, p, splits):
    """The fused launch at cache row p with RoPE row rp != p == lga_rope_kv_append then lga_attention: caches bit-exact,
    y within fp32 reordering, and within the decode bound of an fp64 softmax (the criteria of
    test_attention_decode_fused_matches_two_launch_path). Swapped position pointers would rope with row p and append
    at row rp."""
    qkv = _qkv(H, G)[:1].contiguous()
    k0, v0 = _kv(G)
    cos, sin = _rope()
    pos, rpos = torch.tensor([p], device=DEV), torch.tensor([_rope_pos(p)], device=DEV)
    ka, va = k0.clone(), v0.clone()
    q = ops.rope_kv_append(qkv, ka, va, pos, rpos, cos, sin, H, G, HS, HS)
    ya = ops.attention(q, ka, va, pos, H, G, HS, SCALE, n_splits=splits).float()
    kb, vb = k0.clone(), v0.clone()
    yb = ops.attention_decode_fused(qkv, kb, vb, pos, rpos, cos, sin, H, G, HS, HS, SCALE, n_splits=splits).float()
    assert torch.equal(ka, kb) and torch.equal(va, vb)
    assert not torch.equal(kb[:, p], k0[:, p])  # the row was appended at p
    assert torch.all((ya - yb).abs() <= ya.abs() * 2 ** -7 + 2e-3)
    ref = _fp64_attention(q.cpu()[0], ka.cpu(), va.cpu(), p, H, G)
    err = float(torch.max((yb.double().cpu().view(H, HS) - ref).abs() - ref.abs() * 2 ** -7))
    print(f"H {H} G {G} p {p} splits {splits}: {err:.3e}")
    assert err <= 1e-4


def _kv8_cache(G, valid):
    """Device fp8 cache (k codes, v codes, k scales, v scales) holding rows [0, valid); NaN codes and scales past them."""
    key = ("kv8", G)
    if key not in _CACHE:
        k0, v0 = _kv(G, "kv8")
        _CACHE[key] = (spec.kv8_round(k0.cpu() * 2.0 ** -3), spec.kv8_round(v0.cpu() * 2.0 ** -3))
    (kc, ks, _), (vc, vs, _) = _CACHE[key]
    cache = [t.clone() for t in (kc, vc, ks, vs)]
    for c in cache[:2]:
        c[:, valid:] = 0x7F
    for s in cache[2:]:
        s[:, valid:] = float("nan")
    return tuple(t.to(DEV) for t in cache)


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("splits", [1, 8])
def test_attention_fused_kv8_rope_row_differs_from_cache_row(ops, H, G, p, splits):
    """The fp8-cache form of the same cases (the criteria of test_decode_fused_kv8): the appended row's codes and
    scales == kv8_round of the row the bf16 path writes with RoPE row rp, nothing else changes, y within the decode
    bound of an fp64 softmax over the dequantized cache."""
    qkv = _qkv(H, G)[:1].contiguous()
    cos, sin = _rope()
    pos, rpos = torch.tensor([p], device=DEV), torch.tensor([_rope_pos(p)], device=DEV)
    cache = _kv8_cache(G, valid=p)
    before = [t.clone() for t in cache]
    y = ops.attention_decode_fused_kv8(qkv, cache, pos, rpos, cos, sin, H, G, HS, HS, SCALE, n_splits=splits)
    y = y.double().cpu().view(H, HS)
    assert torch.all(torch.isfinite(y))
    kc = torch.zeros(G, S, HS, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    q_ref = ops.rope_kv_append(qkv, kc, vc, pos, rpos, cos, sin, H, G, HS, HS).cpu()
    for i, row in ((0, kc[:, pos].cpu()), (1, vc[:, pos].cpu())):
        c_ref, s_ref, _ = spec.kv8_round(row)
        assert torch.equal(cache[i + 2][:, p].cpu(), s_ref[:, 0]), i
        assert torch.equal(cache[i][:, p].cpu(), c_ref[:, 0]), i
    keep = torch.ones(S, dtype=torch.bool)
    keep[p] = False
    for now, was in zip(cache, before):
        assert torch.equal(now[:, keep].view(torch.uint8), was[:, keep].view(torch.uint8))  # (bytes: NaN != NaN)
    kcd, vcd, ksd, vsd = (t.cpu() for t in cache)
    ref = _fp64_attention(q_ref[0], spec.kv8_dequantize(kcd, ksd), spec.kv8_dequantize(vcd, vsd), p, H, G)
    err = float(torch.max((y - ref).abs() - ref.abs() * 2 ** -7))
    print(f"H {H} G {G} p {p} splits {splits}: {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("splits", [1, 8])
def test_attention_window_of_three_rows(ops, H, G, p, splits):
    """A window of M = 3 rows == 3 successive one-row launches, y and caches bit for bit (the window's contract); the
    window starts at p, or ends on the last cache row."""
    M = 3
    p0 = min(p, S - M)
    qkv = _qkv(H, G)
    k0, v0 = _kv(G)
    cos, sin = _rope()
    ks, vs = k0.clone(), v0.clone()
    ws1 = ops.AttentionWorkspace(1, H, G, HS, splits, DEV) if splits > 1 else None
    ys = []
    for r in range(M):
        pos = torch.tensor([p0 + r], device=DEV)
        ys.append(ops.attention_decode_fused(qkv[r:r + 1].contiguous(), ks, vs, pos, pos, cos, sin, H, G, HS, HS, SCALE,
                                             splits, workspace=ws1).clone())
    kw, vw = k0.clone(), v0.clone()
    ws = ops.AttentionWorkspace(M, H, G, HS, splits, DEV) if splits > 1 else None
    y = ops.attention_decode_window(qkv, kw, vw, torch.tensor([p0], device=DEV), cos, sin, H, G, HS, HS, SCALE, splits,
                                    workspace=ws)
    for r in range(M):
        assert torch.equal(y[r], ys[r][0]), (p0, r)
    assert torch.equal(kw, ks) and torch.equal(vw, vs)
    assert not torch.equal(ys[0], ys[1])


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("splits", [1, 8])
def test_attention_batch_of_two_with_an_idle_row(ops, H, G, p, splits):
    """B = 2 rows in one launch, one of them idle: the live row's y and slot == the one-row launch on that row and
    slot, bit for bit; the idle row's y is zero and its slot untouched."""
    B, live = 2, p % 2
    qkv = _qkv(H, G)[:B].contiguous()
    k0, v0 = _kv(G)
    k1, v1 = _kv(G, "slot1")
    kc, vc = torch.stack([k0, k1]), torch.stack([v0, v1])
    cos, sin = _rope()
    posv = [17, 17]
    posv[live] = p
    pos = torch.tensor(posv, device=DEV)
    active = torch.tensor([int(b == live) for b in range(B)], dtype=torch.int32, device=DEV)
    ws = ops.AttentionWorkspace(B, H, G, HS, splits, DEV) if splits > 1 else None
    y = ops.attention_decode_batch(qkv, kc, vc, pos, cos, sin, H, G, HS, HS, SCALE, splits, workspace=ws,
                                   active=active)
    ke, ve = [k0, k1][live].clone(), [v0, v1][live].clone()
    one = torch.tensor([p], device=DEV)
    ws1 = ops.AttentionWorkspace(1, H, G, HS, splits, DEV) if splits > 1 else None
    ye = ops.attention_decode_fused(qkv[live:live + 1].contiguous(), ke, ve, one, one, cos, sin, H, G, HS, HS, SCALE,
                                    splits, workspace=ws1)
    assert torch.equal(y[live], ye[0])
    assert torch.equal(kc[live], ke) and torch.equal(vc[live], ve)
    idle = 1 - live
    assert int(y[idle].float().abs().sum()) == 0
    assert torch.equal(kc[idle], [k0, k1][idle]) and torch.equal(vc[idle], [v0, v1][idle])


def test_graph_replay_reads_the_moving_position(ops):
    """One fused attention launch and a device-side pos += 1, captured once and replayed 4 times: every replay equals
    the eager launch at that position (y and caches), so the positions are read from memory on every replay — only the
    pointers are preloaded, never the values behind them."""
    H, G, splits, p0 = 8, 2, 8, 60
    qkv = _qkv(H, G)[:1].contiguous()
    k0, v0 = _kv(G)
    cos, sin = _rope()
    ke, ve = k0.clone(), v0.clone()
    eager = []
    for i in range(4):
        pos, rpos = torch.tensor([p0 + i], device=DEV), torch.tensor([_rope_pos(p0) + i], device=DEV)
        eager.append(ops.attention_decode_fused(qkv, ke, ve, pos, rpos, cos, sin, H, G, HS, HS, SCALE, splits).clone())
    assert not torch.equal(eager[0], eager[1])
    kg, vg = k0.clone(), v0.clone()
    ws = ops.AttentionWorkspace(1, H, G, HS, splits, DEV)
    pos, rpos = torch.tensor([p0], device=DEV), torch.tensor([_rope_pos(p0)], device=DEV)
    y = torch.empty(1, H * HS, dtype=torch.bfloat16, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attention_decode_fused(qkv, kg, vg, pos, rpos, cos, sin, H, G, HS, HS, SCALE, splits, workspace=ws, out=y)
        pos.add_(1)
        rpos.add_(1)
    for i in range(4):
        g.replay()
        assert torch.equal(y, eager[i]), i
    assert int(pos) == p0 + 4 and int(rpos) == _rope_pos(p0) + 4
    assert torch.equal(kg, ke) and torch.equal(vg, ve)
    assert int(ws.counters.abs().sum()) == 0
