"""The batched decode attention launch (lga_attention_decode_batch / _kv8) on the MI355X.

The promise under test: row b of one BATCH launch is the one-sequence fused launch on row b of qkv and cache slot b.
The reference is B sequential ``attention_decode_fused(_kv8)`` calls on copies of the slots with the same ``n_splits``;
y and the WHOLE cache tensors (and the fp8 scales) are compared with ``torch.equal``: nothing of another slot moves.
"""

import math

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
HS = 128
S = 96  # cache rows: ops.decode_splits gives 6 splits
SCALE = 1.0 / math.sqrt(HS)
# per-row positions of one launch, dealt from this pool: only the row's own key (every other split empty), fewer keys
# than splits, mid values, the last cache row, and two rows past the cache (no store, all S keys attended)
POS_POOL = [0, 3, 41, S - 1, S, S + 3, 17, 60]


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


_CACHE = {}


def _bf16(shape, name, std=1.0):
    key = ("v", shape, name, std)
    if key not in _CACHE:
        _CACHE[key] = torch.from_numpy(synth.normal(shape, name, 5, std)).to(DEV).to(torch.bfloat16)
    return _CACHE[key]


def _rope(rows):
    from lit_gpt.model import build_rope_cache

    if ("rope", rows) not in _CACHE:
        cos, sin = build_rope_cache(rows, HS, device=torch.device(DEV))
        _CACHE[("rope", rows)] = (cos.float().contiguous(), sin.float().contiguous())
    return _CACHE[("rope", rows)]


def _cache(slots, G, max_seq, fp8):
    """A filled cache of ``slots`` sequences: (k, v) bf16, or (k codes, v codes, k scales, v scales) for fp8 — finite
    e4m3 codes and power-of-two scales that differ per row. Built once per shape; callers clone."""
    key = ("cache", slots, G, max_seq, fp8)
    if key not in _CACHE:
        if not fp8:
            _CACHE[key] = tuple(_bf16((slots, G, max_seq, HS), f"{n}{slots}x{G}x{max_seq}") for n in "kv")
        else:
            out = []
            for n in "kv":
                c = (_bf16((slots, G, max_seq, HS), f"{n}8{slots}x{G}x{max_seq}").float() * 97.0).to(torch.int32) & 0xFF
                c = torch.where((c & 0x7F) == 0x7F, c - 1, c).to(torch.uint8)  # no NaN codes
                out.append(c.contiguous())
            rows = torch.arange(slots * G * max_seq, device=DEV).view(slots, G, max_seq)
            for shift in (0, 2):
                out.append(torch.exp2(-((rows + shift) % 5 + 2).float()).contiguous())
            _CACHE[key] = tuple(out)
    return _CACHE[key]


def _qkv(H, G, rows=8):
    return _bf16((rows, (H + 2 * G) * HS), f"qkv{H}x{G}")


def _sequential(ops, qkv, cache, pos, H, G, n_splits, fp8, rows=None):
    """The reference: one fused one-row launch per row on a copy of its slot. Returns (ys, cache after)."""
    max_seq = cache[0].shape[-2]
    cos, sin = _rope(max_seq)
    ws = ops.AttentionWorkspace(1, H, G, HS, n_splits, DEV)
    after = tuple(t.clone() for t in cache)
    ys = {}
    for b in (range(qkv.shape[0]) if rows is None else rows):
        p = torch.tensor([pos[b]], device=DEV)
        slot = tuple(t[b].clone() for t in cache)
        row = qkv[b:b + 1].contiguous()
        if fp8:
            y = ops.attention_decode_fused_kv8(row, slot, p, p, cos, sin, H, G, HS, HS, SCALE, n_splits, workspace=ws)
        else:
            y = ops.attention_decode_fused(row, slot[0], slot[1], p, p, cos, sin, H, G, HS, HS, SCALE, n_splits,
                                           workspace=ws)
        ys[b] = y[0].clone()
        for t, s in zip(after, slot):
            t[b].copy_(s)
    return ys, after


def _batch(ops, qkv, cache, pos, H, G, n_splits, fp8, ws=None, active=None, out=None):
    B = qkv.shape[0]
    cos, sin = _rope(cache[0].shape[-2])
    ws = ws or ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV)
    p = pos if torch.is_tensor(pos) else torch.tensor(pos, device=DEV)
    if fp8:
        return ops.attention_decode_batch_kv8(qkv, cache, p, cos, sin, H, G, HS, HS, SCALE, n_splits, workspace=ws,
                                              active=active, out=out)
    return ops.attention_decode_batch(qkv, cache[0], cache[1], p, cos, sin, H, G, HS, HS, SCALE, n_splits,
                                      workspace=ws, active=active, out=out)


def _same(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (i, int((g != w).sum()))


def _check(ops, H, G, B, pos, fp8, slots=None, max_seq=S):
    n_splits = ops.decode_splits(G, H // G, HS, max_seq)
    cache0 = _cache(slots or B, G, max_seq, fp8)
    qkv = _qkv(H, G)[:B].contiguous()
    ys, ref = _sequential(ops, qkv, cache0, pos, H, G, n_splits, fp8)
    got = tuple(t.clone() for t in cache0)
    y = _batch(ops, qkv, got, pos, H, G, n_splits, fp8)
    assert y.shape == (B, H * HS)
    for b in range(B):
        assert torch.equal(y[b], ys[b]), (b, pos[b], int((y[b] != ys[b]).sum()))
    _same(got, ref)
    for b in range(B):
        if pos[b] >= max_seq:  # past the cache: nothing stored, the slot is bit-unchanged
            _same([t[b] for t in got], [t[b] for t in cache0])
        else:
            assert not torch.equal(got[0][b], cache0[0][b])
    return n_splits, cache0, got


GEOMS = [(8, 8), (8, 4), (8, 2), (8, 1)]  # q_per_kv 1, 2, 4, 8 (the last two take head slices at 6 splits)
ROWS = [1, 2, 3, 5, 8]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("B", ROWS)
def test_batch_attention_bit_identical_to_sequential_launches(ops, H, G, B, fp8):
    for off in (0, 3, 5):  # three deals of the pool: every edge position is met at every B
        pos = [POS_POOL[(off + b) % len(POS_POOL)] for b in range(B)]
        n_splits, _, _ = _check(ops, H, G, B, pos, fp8)
        assert n_splits == 6


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_batch_attention_leaves_other_slots_alone(ops, fp8):
    _, cache0, got = _check(ops, 8, 4, 2, [41, 7], fp8, slots=4)
    for t, t0 in zip(got, cache0):
        assert torch.equal(t[2:], t0[2:])


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_batch_attention_long_cache_32_splits(ops, fp8):
    n_splits, _, _ = _check(ops, 8, 2, 2, [12270, 40], fp8, max_seq=12288)
    assert n_splits == 32


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,G", [(8, 8), (8, 2)])
def test_batch_attention_idle_rows(ops, H, G, fp8):
    B, pos = 3, [41, 17, S - 1]
    n_splits = ops.decode_splits(G, H // G, HS, S)
    cache0 = _cache(B, G, S, fp8)
    qkv = _qkv(H, G)[:B].contiguous()
    ys, ref = _sequential(ops, qkv, cache0, pos, H, G, n_splits, fp8, rows=(0, 2))
    got = tuple(t.clone() for t in cache0)
    ws = ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV)
    y = torch.full((B, H * HS), 7.0, dtype=torch.bfloat16, device=DEV)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    _batch(ops, qkv, got, pos, H, G, n_splits, fp8, ws=ws, active=active, out=y)
    assert int(y[1].float().abs().sum()) == 0 and int((y[1].view(torch.int16) != 0).sum()) == 0
    assert torch.equal(y[0], ys[0]) and torch.equal(y[2], ys[2])
    _same(got, ref)
    _same([t[1] for t in got], [t[1] for t in cache0])  # the idle row's slot is bit-unchanged
    assert int(ws.counters.abs().sum()) == 0
    # a second launch through the same workspace, every row active: the counters were left armed for it
    ys2, ref2 = _sequential(ops, qkv, got, pos, H, G, n_splits, fp8)
    y2 = _batch(ops, qkv, got, pos, H, G, n_splits, fp8, ws=ws, active=torch.ones_like(active))
    for b in range(B):
        assert torch.equal(y2[b], ys2[b]), b
    _same(got, ref2)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_batch_attention_graph_replay_with_advancing_positions(ops, fp8):
    H, G, B = 8, 4, 3
    n_splits = ops.decode_splits(G, H // G, HS, S)
    qkv = _qkv(H, G)[:B].contiguous()
    ref = tuple(t.clone() for t in _cache(B, G, S, fp8))
    got = tuple(t.clone() for t in ref)
    pos = torch.tensor([10, 40, S - 3], device=DEV)  # the last row walks off the cache during the replays
    ws = ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV)
    y = torch.empty(B, H * HS, dtype=torch.bfloat16, device=DEV)

    def launch():
        _batch(ops, qkv, got, pos, H, G, n_splits, fp8, ws=ws, out=y)
        pos.add_(1)

    rounds = [pos.tolist()]
    launch()  # warm-up: a real round (the reference runs it too)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for i in range(4):
        p = [rounds[0][b] + i for b in range(B)]
        ys, ref = _sequential(ops, qkv, ref, p, H, G, n_splits, fp8)
        if i:
            g.replay()
        for b in range(B):
            assert torch.equal(y[b], ys[b]), (i, b)
        _same(got, ref)
    assert pos.tolist() == [rounds[0][b] + 4 for b in range(B)]
    assert int(ws.counters.abs().sum()) == 0  # re-armed


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_window_and_batch_forms_share_one_workspace(ops, fp8):
    """The model keeps ONE AttentionWorkspace per row count for every decode form (CausalSelfAttention._decode_setup):
    a window of 2 rows and a batch of 2 sequences, launched in turn through the same workspace, must give the bits they
    give with a fresh workspace each — every launch leaves the arrival counters as it found them."""
    H, G, max_seq, n_splits = 4, 2, 64, 4
    qkv = _qkv(H, G)
    cos, sin = _rope(max_seq)

    def run(workspace):
        cache = tuple(t.clone() for t in _cache(2, G, max_seq, fp8))
        ys = []
        for i, p in enumerate((38, 40)):
            rows = qkv[4 * i:4 * i + 2].contiguous()
            pos0 = torch.tensor([p], device=DEV)
            slot0 = tuple(t[0] for t in cache)  # views: the window appends to slot 0 of the batch's cache
            if fp8:
                ys.append(ops.attention_decode_window_kv8(rows, slot0, pos0, cos, sin, H, G, HS, HS, SCALE, n_splits,
                                                          workspace=workspace()))
            else:
                ys.append(ops.attention_decode_window(rows, slot0[0], slot0[1], pos0, cos, sin, H, G, HS, HS, SCALE,
                                                      n_splits, workspace=workspace()))
            ys.append(_batch(ops, qkv[4 * i + 2:4 * i + 4].contiguous(), cache, [p + 2, 43 - p], H, G, n_splits, fp8,
                             ws=workspace()))
        return ys, cache

    shared = ops.AttentionWorkspace(2, H, G, HS, n_splits, DEV)
    got_y, got_cache = run(lambda: shared)
    ref_y, ref_cache = run(lambda: ops.AttentionWorkspace(2, H, G, HS, n_splits, DEV))
    assert len(got_y) == 4
    _same(got_y, ref_y)
    _same(got_cache, ref_cache)
    assert not torch.equal(got_cache[0], _cache(2, G, max_seq, fp8)[0])
    assert int(shared.counters.abs().sum()) == 0  # re-armed by the last launch too


def test_batch_attention_argument_errors(ops):
    H, G = 8, 8
    kc, vc = (t.clone() for t in _cache(8, G, S, False))
    qkv = _bf16((9, (H + 2 * G) * HS), "qkv9")
    cos, sin = _rope(S)
    err = (ValueError, RuntimeError)
    pos = torch.arange(9, device=DEV)
    for B in (0, 9):
        with pytest.raises(err):
            ops.attention_decode_batch(qkv[:B], kc, vc, pos[:B], cos, sin, H, G, HS, HS, 0.1)
    with pytest.raises(err):  # more rows than slots
        ops.attention_decode_batch(qkv[:3].contiguous(), kc[:2], vc[:2], pos[:3], cos, sin, H, G, HS, HS, 0.1)
    with pytest.raises(err):  # splits without a workspace
        ops.attention_decode_batch(qkv[:2].contiguous(), kc, vc, pos[:2], cos, sin, H, G, HS, HS, 0.1, n_splits=6)
    with pytest.raises(ValueError, match="workspace built for"):  # a workspace built for another key
        ops.attention_decode_batch(qkv[:2].contiguous(), kc, vc, pos[:2], cos, sin, H, G, HS, HS, 0.1, n_splits=6,
                                   workspace=ops.AttentionWorkspace(3, H, G, HS, 6, DEV))
    with pytest.raises(err):  # active of the wrong length
        ops.attention_decode_batch(qkv[:2].contiguous(), kc, vc, pos[:2], cos, sin, H, G, HS, HS, 0.1,
                                   active=torch.ones(3, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="q_per_kv"):  # 3 heads per group
        ops.attention_decode_batch(_bf16((2, (6 + 4) * HS), "qkv6x2"), kc[:, :2].contiguous(), vc[:, :2].contiguous(),
                                   pos[:2], cos, sin, 6, 2, HS, HS, 0.1)
    lib = ops.load_library()  # the C entry points check the same before any launch
    p = qkv.data_ptr()
    full = G * S * HS
    f = lib.lga_attention_decode_batch
    for B in (0, 9):
        assert f(p, p, p, p, p, p, p, S, p, p, p, B, full, None, H, G, HS, HS, S, 1, 0.1, None) != 0
        assert b"[1, 8]" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, p, S, p, p, p, 2, full - 1, None, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"slot_stride" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, p, S, p, None, None, 2, full, None, H, G, HS, HS, S, 6, 0.1, None) != 0
    assert b"workspace" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, p, S, p, p, p, 2, full, None, H, G, 64, 64, S, 1, 0.1, None) != 0
    assert b"head_size" in lib.lga_last_error_string()
    f8 = lib.lga_attention_decode_batch_kv8
    assert f8(p, p, p, p, p, p, p, p, p, S, p, p, p, 9, full, G * S, None, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"[1, 8]" in lib.lga_last_error_string()
    assert f8(p, p, p, p, p, p, p, p, p, S, p, p, p, 2, full - 1, G * S, None, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"slot_stride" in lib.lga_last_error_string()
    assert f8(p, p, p, p, p, p, p, p, p, S, p, p, p, 2, full, G * S - 1, None, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"scale_slot_stride" in lib.lga_last_error_string()
    assert torch.equal(kc, _cache(8, G, S, False)[0])  # nothing was launched
