"""Score profiles for the bf16 / fp8 attention kernels, in numpy only (no GPU; torch is imported by the two adapters of
the rope and fp8 specifications alone, when they are called): generators of q / K / V whose
softmax is peaked or sits far from zero, the float64 reference with its per-(row, head) tolerance, the precondition
each profile states on that reference, and four deliberately wrong fp32 softmaxes for the host-side mutation checks.

With q, k ~ N(0, 1) and scale = 1 / sqrt(hs) no score leaves about +-3.5 nats: exp() of a raw score neither overflows
nor flushes, and every weight is about 1 / L, so a dropped max subtraction, a wrong rescale factor or a lost partial
dilutes to rounding level. The profiles here make the softmax say "this key, exactly" or put every score beyond what
fp32 exp() survives without the running maximum:

    one_hot     one hot key per head (score BETA = 40 nats; the others stay below ~14)
    two_peaks   two bit-identical hot rows per head: weights 0.5 / 0.5
    runner_up   a hot key and a second key 1 nat below it (tuned on the storage grid to within 1e-3 nat)
    offset_pos  every score large and positive (2^160 and more in the kernels' log2 units)
    offset_neg  every score large and negative
    ramp_up     scores rise linearly with the key index, the newest key highest
    sink        key 0 highest, scores fall linearly

All arrays are float32 holding bf16-representable values (q, v and bf16 K rows) or values of the fp8 storage grid
(kv8_spec: e4m3 codes times a power-of-two row scale). Shapes: q (T, H, hs), k / v (G, S, hs), positions (T,): query
row t attends keys 0..positions[t] of group h // (H // G).
"""

import math

import numpy as np

LOG2E = 1.4426950408889634
OUTSIDE = 2.0 ** -30  # the mass a peaked profile may leave outside its hot key(s)
BETA = 40.0  # hot score in nats (24 leaves 1.6e-7 outside at 2304 keys and 8 heads per group: not enough)
BETA_ROWS = 64.0  # hot score where a whole prompt's rows point at keys of one K (hot_directions)
OFFSET_C = 128.0  # offset profiles: the component of every key along the group direction
OFFSET_C_FP8 = 160.0  # (e4m3 rounding spreads the scores by ~0.2 c: a larger c keeps them past 160 log2 units)
OFFSET_LOG2 = 160.0
RAMP_NATS = 64.0  # rise (fall) of ramp_up (sink) between key 0 and key p
PROFILES = ("one_hot", "two_peaks", "runner_up", "offset_pos", "offset_neg", "ramp_up", "sink")


def seed(*key) -> int:
    """A stable seed from small ints."""
    s = 0x9E3779B9
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


def rng(*key):
    return np.random.default_rng(seed(*key))


def round_to_bf16(x) -> np.ndarray:
    """float64 -> the nearest bf16 value (ties to even), as float64."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    q = np.exp2(np.maximum(e - 8, -133).astype(np.float64))
    return np.rint(x / q) * q


def bf16(x) -> np.ndarray:
    """The nearest bf16 values as float32 (what the device tensors are made of)."""
    return round_to_bf16(x).astype(np.float32)


def is_bf16(x) -> bool:
    x = np.asarray(x)
    return x.dtype == np.float32 and bool(np.all((x.view(np.uint32) & 0xFFFF) == 0))


_NORMAL = {}


def normal(shape, *key) -> np.ndarray:
    """N(0, 1) rounded to bf16, a read-only array kept for the last few (shape, key): callers copy before writing."""
    at = (tuple(shape), key)
    if at not in _NORMAL:
        while len(_NORMAL) >= 6:
            _NORMAL.pop(next(iter(_NORMAL)))
        a = bf16(rng(*key).standard_normal(shape))
        a.setflags(write=False)
        _NORMAL[at] = a
    return _NORMAL[at]


_QUANT = {}


def _quantized(quantize, a, shape, *key):
    """quantize(a) for a = normal(shape, *key), kept like normal()'s arrays (read-only)."""
    at = (tuple(shape), key)
    if at not in _QUANT:
        while len(_QUANT) >= 4:
            _QUANT.pop(next(iter(_QUANT)))
        _QUANT[at] = quantize(a)
        for x in _QUANT[at]:
            x.setflags(write=False)
    return _QUANT[at]


def unrope(y, cos, sin) -> np.ndarray:
    """The rotate-half RoPE undone in float64: rope(unrope(y)) = y. cos / sin are the table rows (hs values each, the
    two halves equal); rounding the result to bf16 and roping it on the device gives y back within two roundings."""
    y = np.asarray(y, dtype=np.float64)
    half = y.shape[-1] // 2
    rot = np.concatenate((-y[..., half:], y[..., :half]), axis=-1)
    return y * np.asarray(cos, np.float64) - rot * np.asarray(sin, np.float64)


# ------------------------------------------------------------------------------------------------- storage grids
def _ulp(x, mant_bits, row_scale=None):
    """The grid step at x: bf16 (mant_bits = 7) or e4m3 codes times row_scale (mant_bits = 3, exponents >= -6)."""
    c = np.abs(np.asarray(x, np.float64)) / (1.0 if row_scale is None else row_scale)
    _, e = np.frexp(np.where(c == 0, 1.0, c))
    e = np.where(c == 0, -10 ** 6, e - 1)  # c = m 2^e, m in [1, 2)
    e = np.maximum(e, -6 if row_scale is not None else -126)
    return np.exp2((e - mant_bits).astype(np.float64)) * (1.0 if row_scale is None else row_scale)


def tune_rows(rows, qvec, scale, targets, mant_bits=7, row_scale=None) -> np.ndarray:
    """Move elements of each row of ``rows`` (n, hs) by one grid step, greedily from the coarsest coordinate to the
    finest, until scale * (row . q) meets ``targets`` (n,) as closely as the grid allows (about 1e-3 nat); ``qvec`` is
    (hs,) or one query per row (n, hs). The element of largest magnitude stays (it fixes an fp8 row's scale) and no
    other element may pass it. Returns the tuned rows (float64, on the grid)."""
    rows = np.array(rows, dtype=np.float64)
    n = rows.shape[0]
    qv = np.broadcast_to(np.asarray(qvec, np.float64), rows.shape)
    targets = np.broadcast_to(np.asarray(targets, np.float64), (n,))
    rs = None if row_scale is None else np.broadcast_to(np.asarray(row_scale, np.float64), (n,))
    amax = np.abs(rows).max(axis=1)
    top = np.abs(rows).argmax(axis=1)
    ar = np.arange(n)
    score = scale * (rows * qv).sum(axis=1)
    for _ in range(2):
        step = _ulp(rows, mant_bits, None if rs is None else rs[:, None]) * np.abs(qv)  # per grid step
        order = np.argsort(-step, axis=1)
        for c in range(rows.shape[1]):
            i = order[:, c]
            err = targets - score
            qi = qv[ar, i]
            u = _ulp(rows[ar, i], mant_bits, rs)
            d = np.sign(err) * np.sign(qi) * u  # the move that raises / lowers the score as needed
            gain = np.abs(qi) * u * scale
            new = rows[ar, i] + d
            ok = (gain < 2 * np.abs(err)) & (i != top) & (np.abs(new) < amax) & (gain > 0)
            rows[ar, i] = np.where(ok, new, rows[ar, i])
            score = score + np.where(ok, d * qi * scale, 0.0)
    return rows


# ---------------------------------------------------------------------------------------------------- generators
def hot_row(qvec, beta, scale) -> np.ndarray:
    """bf16(beta q / (scale |q|^2)): the key whose score on q is beta."""
    qv = np.asarray(qvec, np.float64)
    return bf16(beta * qv / (scale * (qv @ qv)))


def _group(h, H, G):
    return h // (H // G)


def one_hot(q, k, hot, scale, beta=BETA) -> np.ndarray:
    """k (G, S, hs) with key hot[h] of head h's group replaced by head h's hot row (q (H, hs): one query row). The
    heads of a group want different keys of the same K."""
    H, G = q.shape[0], k.shape[0]
    assert len({(_group(h, H, G), hot[h]) for h in range(H)}) == H, "one key per head"
    k = k.copy()
    for h in range(H):
        k[_group(h, H, G), hot[h]] = hot_row(q[h], beta, scale)
    return k


def two_peaks(q, k, pairs, scale, beta=BETA) -> np.ndarray:
    """Keys a != b of pairs[h] both hold head h's hot row, bit for bit."""
    H, G = q.shape[0], k.shape[0]
    k = k.copy()
    for h in range(H):
        a, b = pairs[h]
        assert a != b
        k[_group(h, H, G), a] = k[_group(h, H, G), b] = hot_row(q[h], beta, scale)
    return k


def runner_up(q, k, pairs, scale, beta=BETA, quantize=None, fixed=None) -> np.ndarray:
    """Key a of pairs[h] scores beta, key b exactly 1 nat less: b's row is tuned on the storage grid against the score
    a's row really has. ``quantize`` (rows -> (values on the fp8 grid, row scales)) is applied first for fp8 caches;
    the other rows are left to the caller's own quantization. ``fixed``: a key index whose row is not replaced."""
    mant_bits = 7 if quantize is None else 3
    H, G = q.shape[0], k.shape[0]
    k = k.copy()
    q64 = q.astype(np.float64)
    gs = np.arange(H) // (H // G)
    a, b = (np.array([pr[i] for pr in pairs]) for i in (0, 1))
    assert np.all(a != b)
    qq = (q64 * q64).sum(-1, keepdims=True)
    ra = bf16(beta * q64 / (scale * qq)).astype(np.float64)
    rb = bf16((beta - 1.0) * q64 / (scale * qq)).astype(np.float64)
    if fixed is not None:  # (a row the launch itself writes: taken as it is)
        ra = np.where((a == fixed)[:, None], k[gs, a].astype(np.float64), ra)
    sb = None
    if quantize is not None:
        ra = quantize(ra)[0].astype(np.float64)
        rb, sb = (x.astype(np.float64) for x in quantize(rb))
    sa = scale * (ra * q64).sum(-1)
    k[gs, a] = ra
    k[gs, b] = tune_rows(rb, q64, scale, sa - 1.0, mant_bits, sb)
    return k


def group_dirs(G, hs, *key) -> np.ndarray:
    """One unit vector per query group (float64)."""
    u = rng(*key, 77).standard_normal((G, hs))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def directed_q(T, H, G, u, *key, sign=1.0, noise=1.0) -> np.ndarray:
    """q[t, h] = sign gamma_h sqrt(hs) u_g + N(0, noise^2) orthogonal to u_g, gamma_h spread over [1, 1.5] inside each
    group: scale q . (c u_g) = sign gamma_h c. ``sign`` may be (T,) (rows of one launch looking both ways)."""
    hs = u.shape[1]
    qpk = H // G
    n = rng(*key, 78).standard_normal((T, H, hs)) * noise
    ug = np.repeat(u, qpk, axis=0)  # (H, hs)
    n -= (n * ug).sum(-1, keepdims=True) * ug
    gamma = 1.0 + 0.5 * (np.arange(H) % qpk) / max(qpk - 1, 1)
    sg = np.broadcast_to(np.asarray(sign, np.float64), (T,))[:, None, None]
    return bf16(sg * gamma[None, :, None] * math.sqrt(hs) * ug[None] + n)


def offset_k(u, S, c, *key) -> np.ndarray:
    """K_j = N(0, 1) + c u_g."""
    G, hs = u.shape
    return bf16(rng(*key, 79).standard_normal((G, S, hs)) + c * u[:, None, :])


def ramp_k(u, r) -> np.ndarray:
    """K_j = r_j u_g: with q from directed_q and scale = 1 / sqrt(hs), head h scores gamma_h r_j on key j; r (S,) in
    nats."""
    return bf16(np.asarray(r, np.float64)[None, :, None] * u[:, None, :])


def ramp_values(S, p, nats=RAMP_NATS, sign=1.0) -> np.ndarray:
    """r_j = sign nats j / p over the keys 0..S-1 (ramp_up: sign = 1, sink: sign = -1)."""
    return sign * nats * np.arange(S, dtype=np.float64) / max(p, 1)


def hot_directions(T, H, G, S, hs, hot, scale, *key, beta=BETA_ROWS):
    """A whole prompt of one-hot rows over ONE K: every key j is a random direction d_j scaled so that a query along
    it scores beta, and row t's heads all point along d of hot[t] (lengths 1 .. 1.375 inside a group, so rows and
    heads that share a key still differ). Returns q (T, H, hs), k (G, S, hs)."""
    qpk = H // G
    d = rng(*key, 80).standard_normal((G, S, hs))
    k = bf16(beta * d / (scale * (d * d).sum(-1, keepdims=True)))
    q = np.zeros((T, H, hs), np.float32)
    for h in range(H):
        q[:, h] = bf16((1.0 + 0.375 * (h % qpk) / max(qpk - 1, 1)) * d[h // qpk, np.asarray(hot)])
    return q, k


# ----------------------------------------------------------- the two specifications the fused forms are built on
# (the only places that need torch, imported when called: the module itself stays numpy only)
_ROPE = {}


def oracle_rope(p, hs, rope_rows):
    """(rope, inv) for decode_case at position p: rope(x) = bf16(oracle.model.apply_rope(bf16 x)) on the fp32 table
    row p, as float32; inv its float64 inverse."""
    import torch

    from oracle import model as om

    if (hs, rope_rows) not in _ROPE:
        _ROPE[(hs, rope_rows)] = om.build_rope_cache(rope_rows, hs, 10000)
    cos, sin = _ROPE[(hs, rope_rows)]
    c, s = cos[p], sin[p]

    def rope(x):
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
        return om.apply_rope(t, c, s).float().numpy()

    return rope, (lambda y: unrope(y, c.numpy(), s.numpy()))


def kv8_quantize(rows):
    """tests/kv8_spec.py on numpy rows: (values the fp8 cache gives back, row scales)."""
    import torch

    import kv8_spec

    _, s, deq = kv8_spec.kv8_round(torch.from_numpy(np.array(rows, dtype=np.float32)))
    return deq.numpy(), s.numpy()


# ------------------------------------------------------------------------------------------- one decode row
class Case:
    """q (1, H, hs): the roped query the kernel scores with; k, v (G, p + 1, hs): the rows the cache holds once the
    launch is over (fp8: the dequantized values, with k_scale / v_scale (G, p + 1)). Fused forms: q_raw (H, hs),
    k_raw, v_raw (G, hs) are the un-roped contents of the qkv row, and row p of k / v is what the launch is expected
    to append (the tests read the row back and use that)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def decode_case(profile, H, G, hs, p, *key, hot=None, pairs=None, rope=None, inv=None, quantize=None, beta=BETA,
                k_exp=None, v_exp=None) -> Case:
    """One decode row at position p under ``profile``. ``hot`` (H,) / ``pairs`` (H, 2) name the hot keys of one_hot /
    of two_peaks and runner_up. lga_attention takes q roped (rope = inv = None). The fused forms rope q and the new
    key themselves: ``rope(x)`` must be bf16(rope(x)) at this row's position exactly as the kernels compute it
    (oracle.model.apply_rope, to which lga_rope_kv_append is pinned bit for bit) and ``inv(y)`` its float64 inverse
    (unrope); every cache row is then built in roped space from the roped q, the new key's row p is taken as the launch
    will store it, and a twin or runner-up of the new key is derived from that stored row. ``quantize(rows) ->
    (values, scales)`` is the fp8 cache format (kv8_spec.kv8_round) for the fp8 form. ``k_exp`` / ``v_exp`` (p + 1,):
    powers of two on the magnitude of the ordinary K rows / of all V rows."""
    assert profile in PROFILES
    scale = 1.0 / math.sqrt(hs)
    fused = rope is not None
    L = p + 1
    qpk = H // G
    u = group_dirs(G, hs, *key)
    if profile in ("offset_pos", "offset_neg"):
        qt = directed_q(1, H, G, u, *key)[0]
    elif profile in ("ramp_up", "sink"):
        # (an fp8 K row is off its direction by 2^-4 relative: a q component across u_g would turn that into nats)
        qt = directed_q(1, H, G, u, *key, noise=0.0 if quantize is not None else 0.25)[0]
    else:
        qt = normal((H, hs), *key, 1)
    q_raw = bf16(inv(qt)) if fused else None
    q = rope(q_raw) if fused else qt
    k = normal((G, L, hs), *key, 2)
    v = normal((G, L, hs), *key, 3)
    if k_exp is not None:
        k = k * np.exp2(np.asarray(k_exp, np.float32))[None, :, None]
    if v_exp is not None:
        v = v * np.exp2(np.asarray(v_exp, np.float32))[None, :, None]
    r = None
    if profile == "one_hot":
        k = one_hot(q, k, hot, scale, beta)
    elif profile == "two_peaks":
        k = two_peaks(q, k, pairs, scale, beta)
    elif profile == "runner_up":
        if fused:  # the new key can only be the hot one of a pair: its row is not tuned
            pairs = [(b, a) if b == p else (a, b) for a, b in pairs]
        k = one_hot(q, k, [a for a, _ in pairs], scale, beta)
    elif profile in ("offset_pos", "offset_neg"):
        c = OFFSET_C_FP8 if quantize is not None else OFFSET_C
        k = offset_k(u, L, c if profile == "offset_pos" else -c, *key)
    else:
        r = ramp_values(L, p, sign=1.0 if profile == "ramp_up" else -1.0)
        if profile == "ramp_up":
            r[p] += 4.0  # the newest key stands clear of its neighbours' rounding, whatever form stores it
        k = ramp_k(u, r)
    k_raw = v_raw = None
    if fused:
        k_raw = bf16(inv(k[:, p]))
        v_raw = v[:, p].copy()
        k[:, p] = rope(k_raw)
        if quantize is not None:
            k[:, p] = quantize(k[:, p])[0]
        if profile == "two_peaks":
            for h, (a, b) in enumerate(pairs):
                if p in (a, b):
                    k[h // qpk, a] = k[h // qpk, b] = k[h // qpk, p]
    if profile == "runner_up":
        k = runner_up(q, k, pairs, scale, beta, quantize, fixed=p if fused else None)
    k_scale = v_scale = None
    if quantize is not None:
        base = normal((G, L, hs), *key, 2)
        if k_exp is None and r is None and k.shape == base.shape:  # quantize the rows the profile wrote, reuse the rest
            kq, ks = _quantized(quantize, base, (G, L, hs), *key, 2)
            wrote = np.any(k != base, axis=-1)
            kq, ks = kq.copy(), ks.copy()
            kq[wrote], ks[wrote] = quantize(k[wrote])
            k, k_scale = kq, ks
        else:
            k, k_scale = quantize(k)
        v, v_scale = _quantized(quantize, v, (G, L, hs), *key, 3) if v_exp is None else quantize(v)
        if r is not None:  # e4m3 rounding is +-0.2 nat on these rows: put every stored row back on the ramp
            n = p if fused else L
            for g in range(G):
                k[g, :n] = tune_rows(k[g, :n], q[g * qpk], scale, r[:n], 3, k_scale[g, :n])
    assert is_bf16(q) and is_bf16(k) and is_bf16(v)
    return Case(profile=profile, q=q[None], k=k, v=v, k_scale=k_scale, v_scale=v_scale, q_raw=q_raw, k_raw=k_raw,
                v_raw=v_raw, hot=hot, pairs=pairs, p=p, scale=scale)


def check_case(c: Case, r: "Reference", t=0):
    """The profile's precondition on every head of row t of the reference."""
    H = r.ref.shape[1]
    for h in range(H):
        if c.profile == "one_hot":
            check_one_hot(r, t, h, c.hot[h])
        elif c.profile == "two_peaks":
            check_two_peaks(r, t, h, *c.pairs[h])
        elif c.profile == "runner_up":
            check_runner_up(r, t, h, *c.pairs[h])
        else:
            globals()["check_" + c.profile](r, t, h)


# ----------------------------------------------------------------- the plan of tests/test_gpu_attention_scores.py
# (shared with tests/test_attention_profiles_host.py, which checks every precondition without a GPU)
FORMS = ("rows", "fused", "kv8")  # lga_attention at T = 1, lga_attention_decode_fused, ..._fused_kv8
# (H, G, hs, n_splits): one geometry per instantiation the dispatcher can pick (Q1, Q1_FEW, Q2, Q4, Q8, head slices)
DECODE_GEOMS = [(32, 32, 128, 1), (8, 8, 128, 1), (16, 8, 128, 1), (32, 8, 128, 1), (8, 1, 128, 1), (8, 1, 128, 7)]
ROWS_GEOMS = [(4, 2, 64, 1), (12, 12, 64, 1)]  # lga_attention only (the fused forms are hs = 128)
SWEEP_P = 199
SWEEP_SPLITS = (1, 7)
LONG_S = 2304
LONG_P = (2047, 2303)
LONG_SPLITS = (8, 36, 256)
LONG_EXTRA = [(2049, 256)]  # 2048 and 2304 keys fill all 256 splits; 2050 keys (chunk 9) leave 28 splits with no key
PROFILE_P = (199, 2303)


def long_runs():
    return [(p, n) for p in LONG_P for n in LONG_SPLITS] + LONG_EXTRA


def geoms(form):
    return DECODE_GEOMS + (ROWS_GEOMS if form == "rows" else [])


def sweep_hot(H, G, p=SWEEP_P):
    """The launches of the every-key sweep: in launch i head h wants key (i H + h) mod (p + 1), so ceil((p + 1) / H)
    launches make every key the hot key of some head (the heads of a group always want different keys)."""
    L = p + 1
    return [[(i * H + h) % L for h in range(H)] for i in range((L + H - 1) // H)]


def default_hot(H, p):
    return [(17 * h + 3) % (p + 1) for h in range(H)]


def default_pairs(H, G, p):
    qpk = H // G
    return [(5 + h % qpk, p - 20 - h % qpk) for h in range(H)]


def long_hot(H, G, p, n_splits):
    """Hot keys at the edges of the split ranges: 0, chunk - 1, chunk, the last cached key, p (and the next edges for
    the later heads of a wide group), dealt so that the heads of a group differ."""
    chunk = (p + n_splits) // n_splits
    cand = []
    for j in (0, chunk - 1, chunk, p - 1, p, 2 * chunk - 1, 2 * chunk, p - 2, 3 * chunk - 1, 3 * chunk):
        if 0 <= j <= p and j not in cand:
            cand.append(j)
    qpk = H // G
    assert len(cand) >= qpk
    return [cand[(h % qpk + h // qpk) % len(cand)] for h in range(H)]


def long_pairs(H, G, p, n_splits, fused):
    """{name: pairs (H, 2)}: the two keys of every head's pair in one row group (64 keys apart: the same row group
    whether a workgroup has 16, 32 or 64 of them), in two row groups of one wave (neighbours), in two waves (8
    apart), in two splits of one combine round, in two rounds (8 splits apart) and, for the fused forms, {a cached
    twin, the new key}. Head i of a group takes the pair shifted by i (2 i for the neighbours), which keeps the
    relation. Placements the split length does not allow are left out."""
    chunk = (p + n_splits) // n_splits
    qpk = H // G
    s = min(2, n_splits - 1)
    lo, hi = s * chunk, min((s + 1) * chunk, p + 1)
    out = {}

    def put(name, a, b, step=1, inside=True):
        pr = [(a + step * (h % qpk), b + step * (h % qpk)) for h in range(H)]
        top = max(max(x) for x in pr)
        if top <= p - 2 and (not inside or top < hi):
            out[name] = pr

    put("one-row-group", lo, lo + 64)
    put("one-wave", lo, lo + 1, step=2)
    put("two-waves", lo, lo + 8)
    put("two-splits", 0, chunk, inside=False)
    if n_splits > 8:
        put("two-rounds", 0, 8 * chunk, inside=False)
    if fused:
        for name, twin in (("new-key-and-neighbour", p - 1), ("new-key-and-key-0", 0)):
            out[name] = [(twin, p) if h % qpk == 0 else (1 + 2 * (h % qpk), 2 + 2 * (h % qpk)) for h in range(H)]
    return out


def sweep_specs(H, G):
    return [dict(profile="one_hot", p=SWEEP_P, hot=hot) for hot in sweep_hot(H, G)]


def long_specs(H, G, p, n_splits, fused):
    out = [dict(profile="one_hot", p=p, hot=long_hot(H, G, p, n_splits))]
    for name, pairs in long_pairs(H, G, p, n_splits, fused).items():
        out += [dict(profile=prof, p=p, pairs=pairs, name=name) for prof in ("two_peaks", "runner_up")]
    return out


def profile_specs(H, G, p):
    return [dict(profile=prof, p=p, hot=default_hot(H, p), pairs=default_pairs(H, G, p)) for prof in PROFILES]


def spread_specs(H, G, p=SWEEP_P):
    """fp8 only: row magnitudes over 2^-8 .. 2^5, so the row scales of K and of V differ by 2^13 (the hot score is
    raised to 160 nats: an ordinary K row 2^5 times as long scores up to ~110)."""
    e = (np.arange(p + 1) * 5) % 14 - 8
    return [dict(profile=prof, p=p, hot=default_hot(H, p), pairs=default_pairs(H, G, p), beta=160.0, k_exp=e,
                 v_exp=(e + 9) % 14 - 8) for prof in ("one_hot", "two_peaks")]


def build(form, H, G, hs, spec) -> Case:
    """decode_case for one spec of the plan under ``form`` (the fused forms rope at position p of a LONG_S-row table,
    the fp8 form stores kv8_spec's format)."""
    kw = {k: v for k, v in spec.items() if k not in ("profile", "p", "name")}
    p = spec["p"]
    if form != "rows":
        kw["rope"], kw["inv"] = oracle_rope(p, hs, LONG_S)
    if form == "kv8":
        kw["quantize"] = kv8_quantize
    return decode_case(spec["profile"], H, G, hs, p, H, G, hs, p, **kw)


# ---------------------------------------------------------------------------------------------- MFMA prefill
PREFILL_GEOMS = [(8, 2), (6, 3)]
PREFILL_HS = (64, 128)
PREFILL_ROWS = [(16, 0), (100, 0), (129, 0), (300, 37)]  # one block, a partial block, a pair, an odd block count
PREFILL_PAIRS = [(2, 9), (5, 40), (5, 70)]  # one 16-key group, the two 32-key halves of a tile, two tiles
PREFILL_SLOPE = 0.5  # nats per key: 32 per 64-key tile
PREFILL_KINDS = ("one_hot", "two_peaks", "ramp_up", "sink", "mixed", "offset_pos", "offset_neg")


def prefill_hot(T, start):
    """Row t's hot key: (37 t + 11) mod (pos_t + 1); the last eight rows are forced onto 0, 31, 32, 63, 64, the first
    key of the row's last tile, pos_t - 1 and pos_t (the diagonal), clipped to 0..pos_t."""
    hot = [(37 * t + 11) % (start + t + 1) for t in range(T)]
    for i, t in enumerate(range(max(T - 8, 0), T)):
        pos = start + t
        forced = (0, 31, 32, 63, 64, 64 * (pos // 64), pos - 1, pos)[i + 8 - min(T, 8)]  # (T < 8: the last ones)
        hot[t] = max(min(forced, pos), 0)
    return hot


def prefill_pairs(T, start):
    top = start + T - 1
    out = [pr for pr in PREFILL_PAIRS if pr[1] <= top]
    if top >= 192 + 70:
        out += [(a + 128, b + 128) for a, b in PREFILL_PAIRS]
    return out


def prefill_case(kind, T, start, H, G, hs, *key, pair=None) -> Case:
    """T query rows at positions start .. start + T - 1 over one K of S = start + T rows. ``checks`` lists
    (check function, row, head, extra arguments) for every (row, head) the profile's precondition applies to."""
    scale = 1.0 / math.sqrt(hs)
    S = start + T
    qpk = H // G
    pos = np.arange(start, start + T)
    v = normal((G, S, hs), *key, 3)
    u = group_dirs(G, hs, *key)
    checks = []
    rows_heads = [(t, h) for t in range(T) for h in range(H)]
    if kind == "one_hot":
        hot = prefill_hot(T, start)
        q, k = hot_directions(T, H, G, S, hs, hot, scale, *key)
        checks = [(check_one_hot, t, h, (hot[t],)) for t, h in rows_heads]
    elif kind == "two_peaks":
        a, b = pair
        d = rng(*key, 81).standard_normal((G, hs))
        k = normal((G, S, hs), *key, 2).copy()
        row = bf16(BETA_ROWS * d / (scale * (d * d).sum(-1, keepdims=True)))
        k[:, a] = k[:, b] = row
        q = np.zeros((T, H, hs), np.float32)
        for h in range(H):
            c = (1.0 + 0.125 * (h % qpk)) * (1.0 + (np.arange(T) % 4) / 8.0)
            q[:, h] = bf16(c[:, None] * d[h // qpk][None, :])
        for t, h in rows_heads:
            if pos[t] >= max(a, b):
                checks.append((check_two_peaks, t, h, (a, b)))
            elif pos[t] >= min(a, b):
                checks.append((check_one_hot, t, h, (min(a, b),)))
    elif kind in ("ramp_up", "sink", "mixed"):
        sign = {"ramp_up": 1.0, "sink": -1.0}.get(kind, np.where(np.arange(T) % 2 == 0, -1.0, 1.0))
        q = directed_q(T, H, G, u, *key, sign=sign, noise=0.25)
        k = ramp_k(u, PREFILL_SLOPE * np.arange(S))
        sg = np.broadcast_to(sign, (T,))
        for t, h in rows_heads:
            if pos[t] >= 127:  # 63.5 nats and more between key 0 and the row's own key
                checks.append((check_ramp_up if sg[t] > 0 else check_sink, t, h, ()))
    else:
        q = directed_q(T, H, G, u, *key)
        k = offset_k(u, S, OFFSET_C if kind == "offset_pos" else -OFFSET_C, *key)
        checks = [(check_offset_pos if kind == "offset_pos" else check_offset_neg, t, h, ()) for t, h in rows_heads]
    assert is_bf16(q) and is_bf16(k) and is_bf16(v)
    return Case(profile=kind, q=q, k=k, v=v, positions=pos, scale=scale, checks=checks)


# -------------------------------------------------------------------------------------- reference and tolerance
class Reference:
    """ref, tol (T, H, hs); scores (nats, scale included; -inf past the row's position) and weights (T, H, S)."""

    def __init__(self, ref, tol, scores, weights):
        self.ref, self.tol, self.scores, self.weights = ref, tol, scores, weights

    def worst(self, got) -> float:
        return float(np.max(np.abs(np.asarray(got, np.float64) - self.ref) / self.tol))


def reference(q, k, v, positions, scale, mfma=False) -> Reference:
    """float64 softmax(scale q K^T) V over keys 0..positions[t] and, per (row, head), the tolerance

        tol = 2^-8 |ref| + 2^-21 (1 + A) max|v|   (+ 2^-8 W for the MFMA prefill)

    A = scale max_j sum_i |q_i k_ji| and max|v| over the attended keys. The second term is the fp32 bound of
    test_f32_attention_matches_fp64 — 8 u (u = 2^-24) for exp, the sums and the division, times (1 + score magnitude)
    because an error of u |s| in a score moves its weight by that much relatively — with |s| replaced by its
    cancellation-free majorant A (the bf16 products are exact, the fp32 accumulation errs by u times the sum of the
    magnitudes, and these scores cancel). 2^-8 |ref| is the bf16 output rounding. MFMA prefill (T >= 16): P enters the
    P.V product rounded to bf16 (2^-8 relative per weight, whatever its sign: W = sum_j p_j |v_j|) while l sums the
    unrounded weights."""
    q64, k64, v64 = (np.asarray(a, np.float64) for a in (q, k, v))
    T, H, hs = q64.shape
    G, S, _ = k64.shape
    qpk = H // G
    pos = np.asarray(positions, dtype=np.int64)
    assert pos.shape == (T,) and pos.min() >= 0 and pos.max() < S
    mask = np.arange(S)[None, :] <= pos[:, None]  # (T, S)
    ref = np.zeros((T, H, hs))
    tol = np.zeros((T, H, hs))
    scores = np.full((T, H, S), -np.inf)
    weights = np.zeros((T, H, S))
    for g in range(G):
        hh = slice(g * qpk, (g + 1) * qpk)
        s = np.einsum("tqd,jd->tqj", q64[:, hh], k64[g]) * scale
        s = np.where(mask[:, None, :], s, -np.inf)
        w = np.exp(s - s.max(axis=-1, keepdims=True))
        p = w / w.sum(axis=-1, keepdims=True)
        A = np.einsum("tqd,jd->tqj", np.abs(q64[:, hh]), np.abs(k64[g])) * scale
        A = np.where(mask[:, None, :], A, 0.0).max(axis=-1)  # (T, qpk)
        vmax = np.maximum.accumulate(np.abs(v64[g]).max(axis=-1))[pos]  # (T,)
        r = p @ v64[g]
        ref[:, hh] = r
        t = 2.0 ** -8 * np.abs(r) + (2.0 ** -21 * (1.0 + A) * vmax[:, None])[..., None]
        if mfma:
            t = t + 2.0 ** -8 * (p @ np.abs(v64[g]))
        tol[:, hh] = t
        scores[:, hh] = s
        weights[:, hh] = p
    return Reference(ref, tol, scores, weights)


# ------------------------------------------------------------------------------------------------ preconditions
def check_one_hot(r: Reference, t, h, j):
    w = r.weights[t, h, j]
    assert w >= 1.0 - OUTSIDE, ("one_hot", t, h, j, 1.0 - w)


def check_two_peaks(r: Reference, t, h, a, b):
    wa, wb = r.weights[t, h, a], r.weights[t, h, b]
    assert abs(wa - 0.5) <= 1e-3 and abs(wb - 0.5) <= 1e-3, ("two_peaks", t, h, wa, wb)
    assert wa + wb >= 1.0 - OUTSIDE, ("two_peaks", t, h, 1.0 - wa - wb)


def check_runner_up(r: Reference, t, h, a, b):
    wa, wb = r.weights[t, h, a], r.weights[t, h, b]
    assert wa + wb >= 1.0 - OUTSIDE, ("runner_up", t, h, 1.0 - wa - wb)
    assert abs(wa / wb / math.e - 1.0) <= 0.02, ("runner_up", t, h, wa / wb)


def _attended(r: Reference, t, h):
    s = r.scores[t, h]
    return s[np.isfinite(s)]


def check_offset_pos(r: Reference, t, h):
    assert _attended(r, t, h).min() * LOG2E >= OFFSET_LOG2, ("offset_pos", t, h, _attended(r, t, h).min())


def check_offset_neg(r: Reference, t, h):
    assert _attended(r, t, h).max() * LOG2E <= -OFFSET_LOG2, ("offset_neg", t, h, _attended(r, t, h).max())


def check_ramp_up(r: Reference, t, h, rise=60.0, every=16):
    """The newest key is the highest, at least ``rise`` nats above key 0, and the running maximum is renewed at least
    every ``every`` keys."""
    s = _attended(r, t, h)
    assert s[-1] == s.max() and s[-1] - s[0] >= rise, ("ramp_up", t, h, s[0], s[-1], s.max())
    run = np.maximum.accumulate(s)
    new = np.flatnonzero(np.concatenate(([True], run[1:] > run[:-1])))
    gaps = np.diff(np.concatenate((new, [len(s)])))
    assert gaps.max() <= every, ("ramp_up: running maximum", t, h, int(gaps.max()))


def check_sink(r: Reference, t, h, fall=60.0):
    s = _attended(r, t, h)
    assert s[0] == s.max() and s[0] - s[-1] >= fall, ("sink", t, h, s[0], s[-1], s.max())


# --------------------------------------------------------------------- the kernels' split softmax, and four mutants
def split_ranges(p, n_splits):
    """attn_split_range: split i of n_splits over the keys 0..p is [i chunk, min((i + 1) chunk, p + 1))."""
    L = p + 1
    chunk = (L + n_splits - 1) // n_splits
    return [(min(i * chunk, L), min((i + 1) * chunk, L)) for i in range(n_splits)]


M_FLOOR = np.float32(-1e30)


def split_softmax(q, k, v, p, scale, n_splits, mutation=None) -> np.ndarray:
    """One query row (q (H, hs)) in fp32 as the decode kernels keep it: a partial (m, l, o) per split in log2 units
    (an empty split: m = -1e30, l = 0, o = 0), merged in split order, divided once and rounded to bf16. ``mutation``
    makes it wrong on purpose:

        "no_max"        exp2 of the raw scores: no maximum anywhere
        "keep_larger"   the merge keeps the partial with the larger m and drops the other
        "stale_l"       the merge rescales o but adds the l's as they are
        "drop_last"     every split's range ends one key early
    """
    assert mutation in (None, "no_max", "keep_larger", "stale_l", "drop_last")
    f32 = np.float32
    H, hs = q.shape
    G = k.shape[0]
    sl2 = f32(f32(scale) * f32(LOG2E))
    out = np.zeros((H, hs), np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for h in range(H):
            g = _group(h, H, G)
            s = (k[g, :p + 1].astype(f32) @ q[h].astype(f32)) * sl2
            parts = []
            for lo, hi in split_ranges(p, n_splits):
                if mutation == "drop_last":
                    hi = max(hi - 1, lo)
                if hi <= lo:
                    parts.append((M_FLOOR, f32(0), np.zeros(hs, f32)))
                    continue
                m = f32(0) if mutation == "no_max" else s[lo:hi].max()
                e = np.exp2(s[lo:hi] - m).astype(f32)
                parts.append((m, e.sum(dtype=f32), (e[:, None] * v[g, lo:hi].astype(f32)).sum(axis=0, dtype=f32)))
            m, l, o = parts[0]
            for mb, lb, ob in parts[1:]:
                if mutation == "keep_larger":
                    if mb > m:
                        m, l, o = mb, lb, ob
                    continue
                mn = max(m, mb)
                ca, cb = np.exp2(f32(m - mn)), np.exp2(f32(mb - mn))
                l = l + lb if mutation == "stale_l" else l * ca + lb * cb
                o = o * ca + ob * cb
                m = mn
            out[h] = o / l
    return np.where(np.isfinite(out), bf16(np.where(np.isfinite(out), out, 0.0)), out)
