"""The shared-prefix decode attention launch (lga_attention_decode_shared) on the MI355X.

The promise under test: B samples of one prompt, all at position p, whose keys below P only cache slot 0 holds, get the
bits of ``attention_decode_batch`` with ``pos = [p] * B`` and the same ``n_splits`` on a cache whose slots 1.. hold
copies of slot 0's rows [0, P). The SHARED run gets the same cache with those rows of slots >= 1 set to bf16 NaN
(0x7FC0): one stray read of them turns y into NaN, one stray write shows in the whole-tensor comparison.
"""

import math

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
HS = 128
S = 640  # cache rows: with 1, 2 or 5 splits every split runs several 64-key steps
STEP = 64
SCALE = 1.0 / math.sqrt(HS)
GEOMS = [(8, 8), (8, 4), (8, 2), (8, 1)]  # q_per_kv 1, 2, 4, 8
ROWS = [1, 2, 3, 4, 5, 8]
SPLITS = [1, 2, 5]
NAN = 0x7FC0


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


_CACHE = {}


def _bf16(shape, name):
    key = (shape, name)
    if key not in _CACHE:
        _CACHE[key] = torch.from_numpy(synth.normal(shape, name, 5, 1.0)).to(DEV).to(torch.bfloat16)
    return _CACHE[key]


def _rope(rows):
    from lit_gpt.model import build_rope_cache

    if ("rope", rows) not in _CACHE:
        cos, sin = build_rope_cache(rows, HS, device=torch.device(DEV))
        _CACHE[("rope", rows)] = (cos.float().contiguous(), sin.float().contiguous())
    return _CACHE[("rope", rows)]


def _base(G, slots=8, max_seq=S):
    """Eight distinct filled slots; never modified (callers clone)."""
    return tuple(_bf16((slots, G, max_seq, HS), f"sh{n}{slots}x{G}x{max_seq}") for n in "kv")


def _qkv(H, G, rows=8):
    return _bf16((rows, (H + 2 * G) * HS), f"shqkv{H}x{G}")


def _caches(G, B, P_eff, max_seq=S):
    """(the reference's cache, the SHARED run's cache): slots 1.. hold slot 0's rows [0, P_eff) / NaN there."""
    ref = tuple(t[:B].clone() for t in _base(G, max_seq=max_seq))
    got = tuple(t.clone() for t in ref)
    for t in ref:
        t[1:, :, :P_eff] = t[:1, :, :P_eff]
    for t in got:
        t[1:, :, :P_eff].view(torch.int16).fill_(NAN)
    return ref, got


def _shared(ops, qkv, cache, p, P, H, G, n_splits, ws=None, active=None, out=None):
    B = qkv.shape[0]
    cos, sin = _rope(cache[0].shape[-2])
    if n_splits > 1:
        ws = ws or ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV)
    pos = p if torch.is_tensor(p) else torch.tensor([p], device=DEV)
    pre = P if torch.is_tensor(P) else torch.tensor([P], device=DEV)
    return ops.attention_decode_shared(qkv, cache[0], cache[1], pos, pre, cos, sin, H, G, HS, HS, SCALE, n_splits,
                                       workspace=ws, active=active, out=out)


def _batch(ops, qkv, cache, p, H, G, n_splits, ws=None, active=None):
    B = qkv.shape[0]
    cos, sin = _rope(cache[0].shape[-2])
    if n_splits > 1:
        ws = ws or ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV)
    pos = torch.full((B,), p, dtype=torch.int64, device=DEV)
    return ops.attention_decode_batch(qkv, cache[0], cache[1], pos, cos, sin, H, G, HS, HS, SCALE, n_splits,
                                      workspace=ws, active=active)


def _eff(p, P):
    return min(min(max(P, 0), p), S)


def _one(ops, H, G, B, n_splits, p, P, active=None, wss=(None, None)):
    """One (p, P): y and row p of every slot bit-equal to the batch launch; every other row of the SHARED run's cache,
    the poisoned rows and all rows past p included, bit-unchanged."""
    P_eff = _eff(p, P)
    ref, got = _caches(G, B, P_eff)
    want = tuple(t.clone() for t in got)
    qkv = _qkv(H, G)[:B].contiguous()
    act = None if active is None else torch.tensor(active, dtype=torch.int32, device=DEV)
    y_ref = _batch(ops, qkv, ref, p, H, G, n_splits, ws=wss[0], active=act)
    y = torch.full((B, H * HS), 7.0, dtype=torch.bfloat16, device=DEV)
    _shared(ops, qkv, got, p, P, H, G, n_splits, ws=wss[1], active=act, out=y)
    tag = (H, G, B, n_splits, p, P)
    assert not torch.isnan(y.float()).any(), tag
    assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), (tag, int((y != y_ref).sum()))
    if p < S:  # the new rows are the batch launch's; nothing else moved
        for w, r in zip(want, ref):
            w[:, :, p] = r[:, :, p]
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int16), w.view(torch.int16)), tag
    return y, got


def _pairs(n_splits):
    """(p, P) pairs on every boundary of the split / step / prefix geometry."""
    p = 600
    chunk = -(-(p + 1) // n_splits)
    k_lo = chunk * (n_splits - 1) if n_splits > 1 else 0  # the last split: it also holds the generated suffix
    k_mid = chunk * (n_splits // 2)
    out = [(p, P) for P in (0, 1, p - 1, p, chunk, chunk + 1, k_lo + STEP + 37, k_mid + 2 * STEP + 37, k_lo + 5,
                            max(p - chunk - 70, 0), STEP, p + 9, -5)]
    for q in (S - 1, S, S + 3):
        out += [(q, 0), (q, 300), (q, q)]
    return out


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("B", ROWS)
def test_shared_attention_bit_identical_to_batch(ops, H, G, B):
    for n_splits in SPLITS:
        wss = (None, None)
        if n_splits > 1:  # one workspace each for the whole sweep: every launch re-arms it
            wss = tuple(ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV) for _ in range(2))
        for p, P in _pairs(n_splits):
            _one(ops, H, G, B, n_splits, p, P, wss=wss)
        if n_splits > 1:
            assert int(wss[1].counters.abs().sum()) == 0


def test_shared_attention_changes_the_cache(ops):
    """(the comparison above is not vacuous: the launch appends, and slot 0's prefix does reach the other rows)"""
    y, got = _one(ops, 8, 8, 2, 2, 600, 300)
    assert not torch.equal(got[0][:, :, 600], _base(8)[0][:2, :, 600])
    ref = tuple(t[:2].clone() for t in _base(8))  # slot 1 with its OWN rows [0, 300): another y[1]
    y_own = _batch(ops, _qkv(8, 8)[:2].contiguous(), ref, 600, 8, 8, 2)
    assert torch.equal(y[0], y_own[0]) and not torch.equal(y[1], y_own[1])


@pytest.mark.parametrize("H,G", [(8, 8), (8, 4), (8, 2)])
@pytest.mark.parametrize("active", [[0, 1, 0, 1], [1, 0, 1, 1], [0, 0, 0, 1], [0, 1, 1, 0, 0, 0, 0, 1]])
def test_shared_attention_idle_rows(ops, H, G, active):
    B = len(active)
    for n_splits in (1, 5):
        for p, P in ((600, 300), (600, 600), (S + 3, 100)):
            y, _ = _one(ops, H, G, B, n_splits, p, P, active=active)  # (idle slots: compared bit-unchanged there)
            for b in range(B):
                assert active[b] or int((y[b].view(torch.int16) != 0).sum()) == 0, (b, p, P)
    y = torch.full((B, H * HS), 7.0, dtype=torch.bfloat16, device=DEV)
    ref, got = _caches(G, B, 300)
    want = tuple(t.clone() for t in got)
    _shared(ops, _qkv(H, G)[:B].contiguous(), got, 600, 300, H, G, 5, out=y,
            active=torch.zeros(B, dtype=torch.int32, device=DEV))  # nobody active: y = 0, nothing moves
    assert int((y.view(torch.int16) != 0).sum()) == 0
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int16), w.view(torch.int16))


def test_shared_attention_graph_replay_with_advancing_position(ops):
    H, G, B, n_splits, P = 8, 4, 3, 5, 300
    p0 = 597  # chunk = ceil((p + 1) / 5) goes 120 -> 121 at p = 600, inside the six positions
    qkv = _qkv(H, G)[:B].contiguous()
    ref, got = _caches(G, B, P)
    pos = torch.tensor([p0], device=DEV)
    pre = torch.tensor([P], device=DEV)
    ws = ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV)
    ws_ref = ops.AttentionWorkspace(B, H, G, HS, n_splits, DEV)
    y = torch.empty(B, H * HS, dtype=torch.bfloat16, device=DEV)

    def launch():
        _shared(ops, qkv, got, pos, pre, H, G, n_splits, ws=ws, out=y)
        pos.add_(1)

    launch()  # warm-up: a real round (the reference runs it too)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    chunks = set()
    for i in range(7):
        if i:
            g.replay()
        y_ref = _batch(ops, qkv, ref, p0 + i, H, G, n_splits, ws=ws_ref)
        chunks.add(-(-(p0 + i + 1) // n_splits))
        assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), i
        for a, b in zip(got, ref):
            assert torch.equal(a[:, :, P:], b[:, :, P:]) and torch.equal(a[0], b[0]), i
            assert int((a[1:, :, :P].view(torch.int16) != NAN).sum()) == 0, i
    assert len(chunks) == 2 and int(pos) == p0 + 7
    assert int(ws.counters.abs().sum()) == 0  # re-armed


def test_window_batch_and_shared_forms_share_one_workspace(ops):
    """The model keeps ONE AttentionWorkspace per row count for every decode form: a window of 2 rows, a batch of 2
    sequences and 2 samples behind a shared prefix, launched in turn through the same workspace, give the bits they
    give with a fresh workspace each — every launch leaves the arrival counters as it found them."""
    H, G, max_seq, n_splits = 4, 2, 192, 4
    qkv = _bf16((12, (H + 2 * G) * HS), "shqkv12")
    cos, sin = _rope(max_seq)

    def run(workspace):
        cache = tuple(t[:2].clone() for t in _base(G, max_seq=max_seq))
        ys = []
        for i, p in enumerate((150, 160)):
            r = qkv[6 * i:6 * i + 6]
            ys.append(_shared(ops, r[:2].contiguous(), cache, p, 100, H, G, n_splits, ws=workspace()))
            ys.append(ops.attention_decode_window(r[2:4].contiguous(), cache[0][0], cache[1][0],
                                                  torch.tensor([p + 1], device=DEV), cos, sin, H, G, HS, HS, SCALE,
                                                  n_splits, workspace=workspace()))
            ys.append(ops.attention_decode_batch(r[4:6].contiguous(), cache[0], cache[1],
                                                 torch.tensor([p + 3, 40 + i], device=DEV), cos, sin, H, G, HS, HS,
                                                 SCALE, n_splits, workspace=workspace()))
        ys.append(_shared(ops, qkv[:2].contiguous(), cache, 170, 100, H, G, n_splits, ws=workspace()))
        return ys, cache

    shared = ops.AttentionWorkspace(2, H, G, HS, n_splits, DEV)
    got_y, got_cache = run(lambda: shared)
    ref_y, ref_cache = run(lambda: ops.AttentionWorkspace(2, H, G, HS, n_splits, DEV))
    assert len(got_y) == 7
    for a, b in zip(got_y + list(got_cache), ref_y + list(ref_cache)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert not torch.equal(got_cache[0], _base(G, max_seq=max_seq)[0][:2])
    assert int(shared.counters.abs().sum()) == 0  # re-armed by the last launch too


def test_shared_attention_argument_errors(ops):
    H, G = 8, 8
    kc, vc = (t.clone() for t in _base(G))
    qkv = _bf16((9, (H + 2 * G) * HS), "shqkv9")
    cos, sin = _rope(S)
    err = (ValueError, RuntimeError)
    pos = torch.tensor([40], device=DEV)
    pre = torch.tensor([20], device=DEV)
    for B in (0, 9):
        with pytest.raises(err):
            ops.attention_decode_shared(qkv[:B], kc, vc, pos, pre, cos, sin, H, G, HS, HS, 0.1)
    with pytest.raises(err):  # no prefix length
        ops.attention_decode_shared(qkv[:2].contiguous(), kc, vc, pos, None, cos, sin, H, G, HS, HS, 0.1)
    with pytest.raises(err):  # one position per row: that is the batch form
        ops.attention_decode_shared(qkv[:2].contiguous(), kc, vc, torch.tensor([40, 40], device=DEV), pre, cos, sin, H,
                                    G, HS, HS, 0.1)
    with pytest.raises(err):  # more rows than slots
        ops.attention_decode_shared(qkv[:3].contiguous(), kc[:2], vc[:2], pos, pre, cos, sin, H, G, HS, HS, 0.1)
    with pytest.raises(err):  # splits without a workspace
        ops.attention_decode_shared(qkv[:2].contiguous(), kc, vc, pos, pre, cos, sin, H, G, HS, HS, 0.1, n_splits=5)
    with pytest.raises(NotImplementedError):  # an fp8 cache
        ops._attention_decode("shared", qkv[:2].contiguous(), (kc, vc, kc, vc), pos, pos, cos, sin, H, G, HS, HS, 0.1,
                              1, None, None, prefix_len=pre)
    lib = ops.load_library()  # the C entry point checks the same before any launch
    p = qkv.data_ptr()
    full = G * S * HS
    f = lib.lga_attention_decode_shared
    for B in (0, 9):
        assert f(p, p, p, p, p, p, p, S, p, p, p, B, full, None, H, G, HS, HS, S, 1, 0.1, None) != 0
        assert b"[1, 8]" in lib.lga_last_error_string()
    assert f(p, p, p, p, None, p, p, S, p, p, p, 2, full, None, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"null" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, p, S, p, p, p, 2, full - 1, None, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"slot_stride" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, p, S, p, None, None, 2, full, None, H, G, HS, HS, S, 5, 0.1, None) != 0
    assert b"workspace" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, p, S, p, p, p, 2, full, None, H, G, 64, 64, S, 1, 0.1, None) != 0
    assert b"head_size" in lib.lga_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(kc, _base(G)[0])  # nothing was launched
