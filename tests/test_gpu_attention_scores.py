"""The bf16 and fp8 attention kernels on peaked and large-magnitude scores (tests/attention_profiles.py): every other
attention test draws q, k ~ N(0, 1), where no score leaves +-3.5 nats — the softmax never needs its maximum and no
weight ever says "this key, exactly", so a wrong rescale factor, a lost partial or a key dropped at a split edge dilutes
to rounding level. Here one key (or two) carries the whole softmax, or every score sits 160 log2 units from zero, at
every place the kernels merge states: row groups, waves, splits, combine rounds, the new key scored from registers,
the MFMA prefill's skipped rescale.

Each case is built on the CPU, its profile's precondition is asserted on the float64 reference BEFORE the GPU result is
looked at, and the result must lie within the reference's per-(row, head) tolerance, derived from the data
(attention_profiles.reference). The fused forms' reference reads the cache rows the launch holds afterwards, the
appended row read back included. Every test prints its worst error / tolerance; the values measured on the MI355X are
in the docstrings. tests/test_attention_profiles_host.py shows without a GPU that this tolerance rejects four wrong
softmaxes.
"""

import numpy as np
import pytest
import torch

import attention_profiles as ap
from oracle import model as om

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_CODE = 0x7F


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return _ops


_ROPE = {}


def _rope(hs):
    if hs not in _ROPE:
        cos, sin = om.build_rope_cache(ap.LONG_S, hs, 10000)
        _ROPE[hs] = (cos.to(DEV), sin.to(DEV))
    return _ROPE[hs]


def _bf(a) -> torch.Tensor:
    """bf16-representable float32 values -> a bf16 device tensor (the cast is exact)."""
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV).to(torch.bfloat16)


def _np(t) -> np.ndarray:
    return t.float().cpu().numpy()


def _nan_cache(rows, S):
    """(G, S, hs) bf16 with ``rows`` (G, n, hs) at its head and NaN behind."""
    G, n, hs = rows.shape
    c = torch.full((G, S, hs), float("nan"), dtype=torch.bfloat16, device=DEV)
    c[:, :n] = _bf(rows)
    return c


def _codes(vals, scale):
    """Values of the fp8 grid and their row scales -> e4m3 codes (exactly)."""
    x = torch.from_numpy(np.ascontiguousarray(vals / scale[..., None], dtype=np.float32))
    c = x.to(torch.float8_e4m3fn)
    assert torch.equal(c.float(), x), "not on the fp8 grid"
    return c.view(torch.uint8)


def _launch(ops, form, c, H, G, hs, n_splits):
    """One decode row under ``form``. Returns y (H, hs) float64 and the K / V rows 0..p the launch scored (fused
    forms: read back from the cache afterwards; row p is what the launch appended, and must be what the case
    expected)."""
    p, L = c.p, c.p + 1
    S = L + 3  # NaN rows behind the position: a read past p cannot pass
    pos = torch.tensor([p], dtype=torch.int64, device=DEV)
    if form == "rows":
        y = ops.attention(_bf(c.q), _nan_cache(c.k, S), _nan_cache(c.v, S), pos, H, G, hs, c.scale, n_splits=n_splits)
        return _np(y).astype(np.float64).reshape(H, hs), c.k, c.v
    qpk = H // G
    qkv = np.concatenate([c.q_raw.reshape(G, qpk, hs), c.k_raw[:, None], c.v_raw[:, None]], axis=1).reshape(1, -1)
    cos, sin = _rope(hs)
    if form == "fused":
        kd, vd = _nan_cache(c.k[:, :p], S), _nan_cache(c.v[:, :p], S)
        y = ops.attention_decode_fused(_bf(qkv), kd, vd, pos, pos, cos, sin, H, G, hs, hs, c.scale, n_splits=n_splits)
        k, v = _np(kd[:, :L]), _np(vd[:, :L])
    else:
        cache = []
        for vals, sc in ((c.k, c.k_scale), (c.v, c.v_scale)):
            codes = torch.full((G, S, hs), NAN_CODE, dtype=torch.uint8)
            codes[:, :p] = _codes(vals[:, :p], sc[:, :p])
            cache.append(codes.to(DEV))
        for sc in (c.k_scale, c.v_scale):
            s = torch.ones(G, S)
            s[:, :p] = torch.from_numpy(np.ascontiguousarray(sc[:, :p], dtype=np.float32))
            cache.append(s.to(DEV))
        y = ops.attention_decode_fused_kv8(_bf(qkv), tuple(cache), pos, pos, cos, sin, H, G, hs, hs, c.scale,
                                           n_splits=n_splits)
        k, v = (_np(cache[i][:, :L].view(torch.float8_e4m3fn)) * _np(cache[i + 2][:, :L])[..., None] for i in (0, 1))
    assert np.array_equal(k[:, :p], c.k[:, :p]) and np.array_equal(v[:, :p], c.v[:, :p]), "cache rows below p changed"
    assert np.array_equal(k[:, p], c.k[:, p]), "the appended key is not the specification's"
    return _np(y).astype(np.float64).reshape(H, hs), k, v


def _run(ops, form, H, G, hs, n_splits, spec) -> float:
    """Build, check the precondition on the reference, launch, compare. Returns the worst error / tolerance."""
    c = ap.build(form, H, G, hs, spec)
    y, k, v = _launch(ops, form, c, H, G, hs, n_splits)
    r = ap.reference(c.q, k, v, [c.p], c.scale)
    ap.check_case(c, r)
    worst = r.worst(y[None])
    what = (form, H, G, hs, n_splits, spec["profile"], spec["p"], spec.get("name"))
    assert np.all(np.isfinite(y)), what
    assert worst <= 1.0, (what, worst)
    if c.profile == "one_hot":  # y[h] is V[g, j_h], and so is the reference
        for h in range(H):
            vj = v[h // (H // G), c.hot[h]].astype(np.float64)
            assert np.all(np.abs(r.ref[0, h] - vj) <= 0.1 * r.tol[0, h]), (what, h)
            assert np.all(np.abs(y[h] - vj) <= r.tol[0, h]), (what, h, c.hot[h])
    return worst


_SHAPES = lambda form: sorted({g[:3] for g in ap.geoms(form)}, reverse=True)  # noqa: E731
_FORM_SHAPES = [(form, *g) for form in ap.FORMS for g in _SHAPES(form)]
_FORM_GEOMS = [(form, *g) for form in ap.FORMS for g in ap.geoms(form)]


@pytest.mark.parametrize("n_splits", ap.SWEEP_SPLITS)
@pytest.mark.parametrize("form,H,G,hs", _FORM_SHAPES)
def test_decode_every_key_is_the_hot_key_once(ops, form, H, G, hs, n_splits):
    """Cache length 200: over ceil(200 / H) launches each of the keys 0..199 is the hot key of one head, so the hot key
    meets every row group, unroll slot, pipeline buffer, the odd-step tail and (7 splits) every split edge; key 199 is
    the fused forms' new key. y[h] must be V[g, j_h]. Measured on the MI355X: worst error / tol = 0.0000 in every case
    (y is V[g, j_h] bit for bit)."""
    worst = max(_run(ops, form, H, G, hs, n_splits, spec) for spec in ap.sweep_specs(H, G))
    print(f"sweep {form} H{H} G{G} hs{hs} x{n_splits}: worst error / tol = {worst:.4f}")


@pytest.mark.parametrize("p,n_splits", ap.long_runs())
@pytest.mark.parametrize("form,H,G,hs", _FORM_SHAPES)
def test_decode_long_cache_split_edges_and_pairs(ops, form, H, G, hs, p, n_splits):
    """2304-row caches at 8, 36 and 256 splits (the second and later rounds of attn_combine; the 2050-key run leaves
    28 splits with no key): hot keys at 0, chunk - 1, chunk, the last cached key and p; two_peaks and runner_up with
    the pair in one row group, two row groups of a wave, two waves, two splits of a round, two rounds, and {the new
    key, a cached twin} in the fused forms. Measured on the MI355X: worst error / tol = 0.9854 (lga_attention, fused)
    and 0.9819 (fp8) — the pairs' averages of two V rows, where the bf16 output rounding alone reaches 2^-8 |ref|; the
    one-hot launches are exact."""
    worst = max(_run(ops, form, H, G, hs, n_splits, spec) for spec in ap.long_specs(H, G, p, n_splits, form != "rows"))
    print(f"long {form} H{H} G{G} hs{hs} p{p} x{n_splits}: worst error / tol = {worst:.4f}")


@pytest.mark.parametrize("p", ap.PROFILE_P)
@pytest.mark.parametrize("form,H,G,hs,n_splits", _FORM_GEOMS)
def test_decode_all_profiles(ops, form, H, G, hs, n_splits, p):
    """All seven profiles for every instantiation the dispatcher can pick, at p = 199 and p = 2303. Measured on the
    MI355X, worst error / tol over the geometries (lga_attention / fused / fp8): one_hot 0 / 0 / 0, two_peaks 0.986 /
    0.986 / 0.969, runner_up 0.969 / 0.969 / 0.928, offset_pos 0.828 / 0.794 / 0.819, offset_neg 0.827 / 0.817 / 0.777,
    ramp_up 0.962 / 0.948 / 0.937, sink 0.961 / 0.948 / 0.951 (the share of the bound that is not the bf16 output
    rounding is 2^-21 (1 + A) max|v|: no case comes near using it)."""
    worst = {s["profile"]: _run(ops, form, H, G, hs, n_splits, s) for s in ap.profile_specs(H, G, p)}
    print(f"profiles {form} H{H} G{G} hs{hs} x{n_splits} p{p}: " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("H,G,hs,n_splits", ap.DECODE_GEOMS)
def test_decode_fp8_row_scales_spread_over_2_13(ops, H, G, hs, n_splits):
    """fp8 cache rows with magnitudes 2^-8 .. 2^5: the row scales of K and of V differ by 2^13 inside one launch; one
    hot key and two peaks. Measured on the MI355X: worst error / tol = 0.8403."""
    worst = max(_run(ops, "kv8", H, G, hs, n_splits, spec) for spec in ap.spread_specs(H, G))
    print(f"fp8 spread H{H} G{G} x{n_splits}: worst error / tol = {worst:.4f}")


@pytest.mark.parametrize("n_splits", [1, 7])
@pytest.mark.parametrize("T", [2, 15])
@pytest.mark.parametrize("H,G,hs", [(8, 8, 128), (32, 8, 128), (8, 1, 128), (4, 2, 64)])
def test_small_T_rows_each_with_its_own_hot_key(ops, H, G, hs, T, n_splits):
    """lga_attention below the MFMA threshold: T rows of one launch at unrelated positions, every (row, head) with a
    hot key of its own. Measured on the MI355X: worst error / tol = 0.0000 in every case."""
    qpk = H // G
    scale = 1.0 / np.sqrt(hs)
    order = [(t * 7) % T for t in range(T)]
    positions = [i * qpk + qpk - 1 + (i * 53) % 60 for i in order]
    hot = [[i * qpk + h % qpk for h in range(H)] for i in order]
    S = max(positions) + 1
    q = ap.normal((T, H, hs), 7, T, H, G, hs)
    k = ap.normal((G, S, hs), 8, T, H, G, hs)
    v = ap.normal((G, S, hs), 9, T, H, G, hs)
    for t in range(T):
        k = ap.one_hot(q[t], k, hot[t], scale)
    r = ap.reference(q, k, v, positions, scale)
    for t in range(T):
        for h in range(H):
            ap.check_one_hot(r, t, h, hot[t][h])
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    y = ops.attention(_bf(q), _nan_cache(k, S + 3), _nan_cache(v, S + 3), pos, H, G, hs, scale, n_splits=n_splits)
    y = _np(y).astype(np.float64).reshape(T, H, hs)
    worst = r.worst(y)
    print(f"small T{T} H{H} G{G} hs{hs} x{n_splits}: worst error / tol = {worst:.4f}")
    assert np.all(np.isfinite(y)) and worst <= 1.0, worst
    for t in range(T):
        for h in range(H):
            assert np.all(np.abs(y[t, h] - v[h // qpk, hot[t][h]]) <= r.tol[t, h]), (t, h)


@pytest.mark.parametrize("T,start", ap.PREFILL_ROWS)
@pytest.mark.parametrize("H,G", ap.PREFILL_GEOMS)
@pytest.mark.parametrize("hs", ap.PREFILL_HS)
def test_prefill_mfma_profiles(ops, hs, H, G, T, start):
    """The MFMA flash attention (T >= 16): one block, a partial block, a pair, an odd block count whose middle block
    has no partner. One hot key per query row (the last wave's rows on 0, 31, 32, 63, 64, the first key of the last
    tile, pos - 1 and the diagonal), two peaks in one 16-key group / the two halves of a tile / two tiles, ramp_up
    (every tile moves every row's max), sink (the skip path after tile 0), rows of one wave alternating between the
    two (the rescale branch while half its rows have c = 1), both offsets. The tolerance carries the bf16 P term.
    Measured on the MI355X, worst error / tol over all shapes: one_hot 0.0000, two_peaks 0.807, ramp_up 0.816, sink
    0.795, mixed 0.816, offset_pos 0.699, offset_neg 0.711."""
    worst = {}
    for kind in ap.PREFILL_KINDS:
        for pair in (ap.prefill_pairs(T, start) if kind == "two_peaks" else [None]):
            c = ap.prefill_case(kind, T, start, H, G, hs, T, start, H, G, hs, pair=pair)
            r = ap.reference(c.q, c.k, c.v, c.positions, c.scale, mfma=True)
            for fn, t, h, extra in c.checks:
                fn(r, t, h, *extra)
            pos = torch.from_numpy(c.positions).to(DEV)
            # (max_seq = start + T: the last tile's rows past the cache come back as zeros, as the kernel states)
            y = ops.attention(_bf(c.q), _bf(c.k), _bf(c.v), pos, H, G, hs, c.scale, n_splits=1)
            y = _np(y).astype(np.float64).reshape(T, H, hs)
            w = r.worst(y)
            worst[kind] = max(worst.get(kind, 0.0), w)
            assert np.all(np.isfinite(y)), (kind, pair)
            assert w <= 1.0, (kind, pair, w)
    print(f"prefill hs{hs} H{H} G{G} T{T} start{start}: " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))


# ----------------------------------------------------------------------------- the multi-row forms: bit identity
MULTI_GEOMS = [(8, 8), (8, 4), (8, 2), (8, 1)]  # 1, 2, 4, 8 heads per workgroup at n_splits = 1
MULTI_PROFILES = ("one_hot", "two_peaks", "offset_pos")
MULTI_S = 256
FILL = 7.0  # cache rows past a sequence's position (finite: the forms' own helpers compare whole caches)


def _multi_case(profile, positions, H, G, quantize=None, hs=128):
    """One fused-form row per position over ONE K / V of MULTI_S rows (a window's rows share their sequence; a batch's
    slots all get it): every (row, head) has hot keys of its own below the smallest position, built from the row's q
    as its position ropes it. Returns qkv (M, (H + 2G) hs), k, v (G, S, hs) float32 (fp8: the dequantized values,
    with their scales)."""
    M, qpk, scale = len(positions), H // G, 1.0 / np.sqrt(hs)
    key = (31, M, H, G, positions[0])
    u = ap.group_dirs(G, hs, *key)
    qt = ap.directed_q(M, H, G, u, *key) if profile == "offset_pos" else ap.normal((M, H, hs), *key, 1)
    q_raw = np.zeros_like(qt)
    k = (ap.offset_k(u, MULTI_S, ap.OFFSET_C, *key) if profile == "offset_pos"
         else ap.normal((G, MULTI_S, hs), *key, 2).copy())
    low = min(positions)
    assert low >= 4 * M * qpk + 8
    for r, p in enumerate(positions):
        rope, inv = ap.oracle_rope(p, hs, MULTI_S)
        q_raw[r] = ap.bf16(inv(qt[r]))
        qr = rope(q_raw[r])
        first = [3 + r * qpk + h % qpk for h in range(H)]
        if profile == "one_hot":
            k = ap.one_hot(qr, k, first, scale)
        elif profile == "two_peaks":
            k = ap.two_peaks(qr, k, [(a, low - 1 - a) for a in first], scale)
    v = ap.normal((G, MULTI_S, hs), *key, 3)
    kn, vn = ap.normal((M, G, 1, hs), *key, 4), ap.normal((M, G, 1, hs), *key, 5)
    qkv = np.concatenate([q_raw.reshape(M, G, qpk, hs), kn, vn], axis=2).reshape(M, -1)
    if quantize is None:
        return qkv, k, v, None, None
    (k, ks), (v, vs) = quantize(k), quantize(v)
    return qkv, k, v, ks, vs


def _slots(k, v, ks, vs, positions, slots):
    """The caches of ``slots`` sequences, sequence b filled up to its position (FILL behind): (k, v) bf16 or (k codes, v
    codes, k scales, v scales)."""
    out = []
    for vals, sc in ((k, ks), (v, vs)):
        if sc is None:
            t = _bf(vals)[None].repeat(slots, 1, 1, 1)
        else:
            t = _codes(vals, sc).to(DEV)[None].repeat(slots, 1, 1, 1)
        for b, p in enumerate(positions):
            t[b, :, p:] = 0x38 if sc is not None else FILL  # (0x38: the e4m3 code of 1.0)
        out.append(t.contiguous())
    if ks is not None:
        for sc in (ks, vs):
            out.append(torch.from_numpy(np.ascontiguousarray(sc))[None].repeat(slots, 1, 1).to(DEV).contiguous())
    return tuple(out)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("n_splits", [1, 5])
@pytest.mark.parametrize("H,G", MULTI_GEOMS)
def test_batch_form_bit_identical_on_peaked_scores(ops, H, G, n_splits, fp8):
    """tests/test_gpu_batch_attention.py's bit-identity check (its _sequential and _batch, as they are) on one_hot,
    two_peaks and offset_pos inputs: three sequences at different positions in one launch against three one-row
    launches — y and every slot, bit for bit (on the MI355X: identical)."""
    import test_gpu_batch_attention as tb

    positions = [199, 150, 171]
    for profile in MULTI_PROFILES:
        qkv, k, v, ks, vs = _multi_case(profile, positions, H, G, ap.kv8_quantize if fp8 else None)
        cache0 = _slots(k, v, ks, vs, positions, len(positions))
        qd = _bf(qkv)
        ys, want = tb._sequential(ops, qd, cache0, positions, H, G, n_splits, fp8)
        got = tuple(t.clone() for t in cache0)
        y = tb._batch(ops, qd, got, positions, H, G, n_splits, fp8)
        for b in range(len(positions)):
            assert torch.isfinite(y[b].float()).all(), (profile, b)
            assert torch.equal(y[b], ys[b]), (profile, b, int((y[b] != ys[b]).sum()))
        tb._same(got, want)
        assert not torch.equal(got[0], cache0[0])


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("n_splits", [1, 5])
@pytest.mark.parametrize("H,G", MULTI_GEOMS)
def test_window_form_bit_identical_on_peaked_scores(ops, H, G, n_splits, fp8):
    """A verify window of three rows at positions 150..152 against three successive one-row launches (the check of
    tests/test_gpu_speculative.py and tests/test_gpu_kv8.py), on one_hot, two_peaks and offset_pos inputs."""
    import test_gpu_batch_attention as tb

    positions = [150, 151, 152]
    cos, sin = tb._rope(MULTI_S)
    for profile in MULTI_PROFILES:
        qkv, k, v, ks, vs = _multi_case(profile, positions, H, G, ap.kv8_quantize if fp8 else None)
        seq = tuple(t[0].contiguous() for t in _slots(k, v, ks, vs, positions[:1], 1))
        win = tuple(t.clone() for t in seq)
        qd = _bf(qkv)
        ws1 = ops.AttentionWorkspace(1, H, G, 128, n_splits, DEV)
        wsm = ops.AttentionWorkspace(len(positions), H, G, 128, n_splits, DEV)
        p0 = torch.tensor(positions[:1], device=DEV)
        ys = []
        for r, p in enumerate(positions):
            pos = torch.tensor([p], device=DEV)
            row = qd[r:r + 1].contiguous()
            if fp8:
                ys.append(ops.attention_decode_fused_kv8(row, seq, pos, pos, cos, sin, H, G, 128, 128, tb.SCALE,
                                                         n_splits, workspace=ws1).clone())
            else:
                ys.append(ops.attention_decode_fused(row, seq[0], seq[1], pos, pos, cos, sin, H, G, 128, 128,
                                                     tb.SCALE, n_splits, workspace=ws1).clone())
        if fp8:
            y = ops.attention_decode_window_kv8(qd, win, p0, cos, sin, H, G, 128, 128, tb.SCALE, n_splits,
                                                workspace=wsm)
        else:
            y = ops.attention_decode_window(qd, win[0], win[1], p0, cos, sin, H, G, 128, 128, tb.SCALE, n_splits,
                                            workspace=wsm)
        for r in range(len(positions)):
            assert torch.isfinite(y[r].float()).all(), (profile, r)
            assert torch.equal(y[r], ys[r][0]), (profile, r, int((y[r] != ys[r][0]).sum()))
        tb._same(win, seq)


@pytest.mark.parametrize("n_splits", [1, 5])
@pytest.mark.parametrize("H,G", MULTI_GEOMS)
def test_shared_form_bit_identical_on_peaked_scores(ops, H, G, n_splits):
    """tests/test_gpu_shared_attention.py's check (its _shared and _batch) on peaked inputs: three samples of one prompt
    at p = 199 behind a prefix of 120 rows, against the batch form on caches whose slots all hold the prefix."""
    import test_gpu_shared_attention as ts

    p, P, B = 199, 120, 3
    for profile in MULTI_PROFILES:
        qkv, k, v, _, _ = _multi_case(profile, [p] * B, H, G)
        ref = _slots(k, v, None, None, [p] * B, B)
        got = tuple(t.clone() for t in ref)
        for t in got:
            t[1:, :, :P].view(torch.int16).fill_(ts.NAN)  # only slot 0 holds the prefix
        qd = _bf(qkv)
        y_ref = ts._batch(ops, qd, ref, p, H, G, n_splits)
        y = ts._shared(ops, qd, got, p, P, H, G, n_splits)
        assert torch.isfinite(y.float()).all(), profile
        assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), (profile, int((y != y_ref).sum()))
        for g_, r_ in zip(got, ref):
            assert torch.equal(g_[:, :, p], r_[:, :, p])


@pytest.mark.parametrize("n_splits", [1, 5])
@pytest.mark.parametrize("H,G", MULTI_GEOMS)
def test_shared_form_reads_the_prefix_from_slot_0_alone(ops, H, G, n_splits):
    """A decoy: rows [0, P) of slots 1.. hold, for every head, a key that would score 20 nats above the true hot key.
    The true hot key of samples 0 and 2 sits at the end of the prefix in slot 0, that of sample 1 at P.. in its own
    slot; y must be the true key's V (the decoys' V rows are 100 away), within the reference's tolerance. Measured on
    the MI355X: worst error / tol = 0.0000 in every case."""
    import test_gpu_shared_attention as ts

    p, P, B, hs = 199, 120, 3, 128
    qpk, scale = H // G, 1.0 / np.sqrt(hs)
    key = (41, H, G)
    rope, inv = ap.oracle_rope(p, hs, MULTI_S)
    q_raw = ap.bf16(inv(ap.normal((B, H, hs), *key, 1)))
    qr = rope(q_raw)
    k = np.repeat(ap.normal((1, G, MULTI_S, hs), *key, 2), B, axis=0)
    v = np.repeat(ap.normal((1, G, MULTI_S, hs), *key, 3), B, axis=0)
    hot = np.zeros((B, H), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            g, i = h // qpk, h % qpk
            row = ap.hot_row(qr[b, h], ap.BETA, scale)
            if b == 1:  # in the sample's own slot, right behind the prefix
                hot[b, h] = P + i
                k[b, g, hot[b, h]] = row
            else:  # in the prefix, which only slot 0 holds: P - 1 downwards
                hot[b, h] = P - 1 - (b * qpk + i)
                k[0, g, hot[b, h]] = row
            if b > 0:  # the decoy, in the rows of slot b that must never be read
                k[b, g, 5 + i] = ap.hot_row(qr[b, h], ap.BETA + 20.0, scale)
                v[b, g, 5 + i] = 100.0
    kn, vn = ap.normal((B, G, 1, hs), *key, 4), ap.normal((B, G, 1, hs), *key, 5)
    qkv = np.concatenate([q_raw.reshape(B, G, qpk, hs), kn, vn], axis=2).reshape(B, -1)
    kd, vd = _bf(k), _bf(v)
    kd[:, :, p:], vd[:, :, p:] = FILL, FILL
    y = _np(ts._shared(ops, _bf(qkv), (kd, vd), p, P, H, G, n_splits)).astype(np.float64).reshape(B, H, hs)
    kd, vd = _np(kd), _np(vd)
    worst = 0.0
    for b in range(B):  # what sample b attends: slot 0 below P, its own slot from P on (the appended row read back)
        kb = np.concatenate([kd[0, :, :P], kd[b, :, P:p + 1]], axis=1)
        vb = np.concatenate([vd[0, :, :P], vd[b, :, P:p + 1]], axis=1)
        r = ap.reference(qr[b:b + 1], kb, vb, [p], scale)
        for h in range(H):
            ap.check_one_hot(r, 0, h, hot[b, h])
            assert np.all(np.abs(y[b, h] - vb[h // qpk, hot[b, h]]) <= r.tol[0, h]), (b, h)
        worst = max(worst, r.worst(y[b:b + 1]))
    print(f"shared decoy H{H} G{G} x{n_splits}: worst error / tol = {worst:.4f}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------- adapter prefix attention
ADAPTER_GEOMS = [(4, 4, 128, 128), (8, 2, 128, 128), (4, 2, 64, 16)]  # H, G, hs, rope_n_elem
ADAPTER_T = 3


def _adapter_case(kind, H, G, hs, n, aT):
    """tests/test_gpu_adapter.py's case dict on a profile: T rows whose heads all point along their group's direction
    d_g (the prefix is one K for every row), key ``hot`` of the prefix scoring BETA_ROWS on it."""
    import adapter_spec as spec
    import test_gpu_adapter as ta

    T, qpk, scale = ADAPTER_T, H // G, 1.0 / hs ** 0.5
    key = (51, H, G, hs, aT)
    theta = 1.0 / (10000 ** (torch.arange(0, n, 2, dtype=torch.float32) / n))
    ang = torch.outer(torch.arange(ta.ROPE_ROWS, dtype=torch.float32), theta).repeat(1, 2)
    cos, sin = torch.cos(ang), torch.sin(ang)
    pos = torch.tensor([5, 90, 33])
    u = ap.group_dirs(G, hs, *key)
    d = ap.rng(*key, 1).standard_normal((G, hs))
    ak = ap.normal((G, aT, hs), *key, 2).copy()
    av = ap.normal((G, aT, hs), *key, 3)
    length = (1.0 + 0.125 * (np.arange(H) % qpk))[None, :, None] * (1.0 + np.arange(T) / 8.0)[:, None, None]
    hot = None
    if kind in ("offset_pos", "offset_neg"):
        qt = ap.directed_q(T, H, G, u, *key)
        ak = ap.offset_k(u, aT, ap.OFFSET_C if kind == "offset_pos" else -ap.OFFSET_C, *key)
    else:
        qt = length * np.repeat(d, qpk, axis=0)[None]
        row = ap.bf16(ap.BETA_ROWS * d / (scale * (d * d).sum(-1, keepdims=True)))
        hot = {"first": (0,), "last": (aT - 1,), "two_peaks": (0, aT - 1)}[kind]
        for j in hot:
            ak[:, j] = row
    q_raw = np.array(qt, dtype=np.float64)
    c64, s64 = cos[pos].double().numpy()[:, None, :], sin[pos].double().numpy()[:, None, :]
    q_raw[..., :n] = ap.unrope(qt[..., :n], c64, s64)
    q_raw = ap.bf16(q_raw)
    qr = q_raw.astype(np.float64)  # what the kernel scores with: bf16(rope(q)) on the first n elements
    half = n // 2
    rot = np.concatenate((-qr[..., half:n], qr[..., :half]), axis=-1)
    qr[..., :n] = qr[..., :n] * c64 + rot * s64
    qr = ap.bf16(qr)
    kn = ap.normal((T, G, 2, hs), *key, 4)
    qkv = np.concatenate([q_raw.reshape(T, G, qpk, hs), kn], axis=2).reshape(T, -1)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    gating = f64(ap.bf16(0.5 * (1.0 + np.arange(H) / H) * (1.0 - 2.0 * (np.arange(H) % 2))))
    c = dict(qkv=f64(qkv), ak=f64(ak), av=f64(av), y=f64(ap.normal((T, H * hs), *key, 5)), gating=gating, cos=cos,
             sin=sin, pos=pos, scale=scale)
    parts = {}
    c["ref"] = spec.prefix_attention_spec(c["y"], c["qkv"], c["ak"], c["av"], c["gating"], cos, sin, pos, H, G, hs, n,
                                          scale, parts=parts)
    c["tol"] = (c["gating"].abs().view(1, H, 1) * ta._ulp(parts["ay"]) + ta._ulp(parts["t"])
                + ta._ulp(c["ref"].view(T, H, hs))).view(T, H * hs)
    return c, ap.reference(qr, ak, av, [aT - 1] * T, scale), hot


@pytest.mark.parametrize("aT", [1, 10, 64])
@pytest.mark.parametrize("H,G,hs,n", ADAPTER_GEOMS)
def test_adapter_prefix_attention_on_peaked_scores(ops, H, G, hs, n, aT):
    """lga_adapter_attention with the hot key at prefix index 0 and at aT - 1, two peaks, and both offsets, against
    tests/adapter_spec.py with the tolerance tests/test_gpu_adapter.py uses for the added term (one bf16 step per
    rounding point of the term, at most 1 % of the elements off the specification's bits). Measured on the MI355X:
    the one-hot and two-peak cases carry the specification's bits everywhere; the offsets differ from them on at most
    0.20 % of the elements, by one bf16 step, and stay 4.6e-5 and more inside the tolerance."""
    import test_gpu_adapter as ta

    for kind in ("first", "last", "two_peaks", "offset_pos", "offset_neg"):
        if kind == "two_peaks" and aT == 1:
            continue
        c, r, hot = _adapter_case(kind, H, G, hs, n, aT)
        for t in range(ADAPTER_T):
            for h in range(H):
                if kind in ("first", "last"):
                    ap.check_one_hot(r, t, h, hot[0])
                elif kind == "two_peaks":
                    ap.check_two_peaks(r, t, h, *hot)
                else:
                    getattr(ap, "check_" + kind)(r, t, h)
        got = ta._run(ops, c, H, G, hs, n)
        assert torch.isfinite(got).all(), kind
        ta._check(got, c["ref"], c["tol"], f"adapter {kind} H{H} G{G} hs{hs} rope{n} aT{aT}")
        assert not torch.equal(got, c["y"])
