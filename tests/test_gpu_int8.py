"""bnb.int8 (LLM.int8) on the MI355X: the int8 kernels and the model path against tests/int8_spec.py.

The integer accumulation is exact, so wherever the outlier term is absent (or multiplies zero weights) the kernels
must reproduce the spec's bf16 bits; with outlier columns the fp32 accumulation order is the kernel's and the bound
is written in the test.
"""

import zlib

import numpy as np
import pytest
import torch

import int8_spec as spec
import parity
from oracle import model as om
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GEMV_SHAPES = [(1000, 256), (77, 1376), (640, 4096), (4096, 11008)]


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(torch.bfloat16)


def bits(t):
    """bf16 tensor / bf16-valued fp32 array -> uint16 bit patterns."""
    if isinstance(t, torch.Tensor):
        return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return spec.bf16_bits(t)


_CACHE = {}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def weights(N, K, name="w"):
    """Asymmetric random bf16 weights (a swapped lane map changes every output), their spec quantization and the
    device copies; computed once per shape."""
    key = (N, K, name)
    if key not in _CACHE:
        w = spec.bf16_round(_rng(f"{name}{N}x{K}").standard_normal((N, K), dtype=np.float32) * np.float32(0.02))
        q, s = spec.quantize_weight(w)
        _CACHE[key] = (w, q, s, torch.from_numpy(q).to(DEV), torch.from_numpy(s).to(DEV))
    return _CACHE[key]


def act(shape, name):
    """bf16 N(0, 1) activations with no |x| >= 6."""
    x = spec.bf16_round(synth.normal(shape, name, 5, 1.0))
    assert np.abs(x).max() < spec.TAU
    return x


# ------------------------------------------------------------------------------------------------ 1. weight quantizer
@pytest.mark.parametrize("in_bf16", [False, True])
def test_weight_quantizer_bit_exact(ops, in_bf16):
    w = _rng("qz").standard_normal((96, 512), dtype=np.float32) * np.float32(0.02)
    w[3] = 0.0  # a zero row: s_w = 0, q = 0
    w[5, 7] = 0.5  # a row with one large element
    # row 9: absmax exactly 127 -> W * (127 / s_w) = W, so these sit exactly on .5 ties (round to even)
    w[9] = 0.0
    w[9, 0] = 127.0
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5, -63.5, 126.5, -126.5], np.float32)
    w[9, 1:1 + ties.size] = ties
    # row 10: absmax 63.5 -> factor exactly 2: k + 0.25 maps to the tie 2k + 0.5
    w[10] = 0.0
    w[10, 0] = -63.5
    w[10, 1:9] = np.array([0.25, 0.75, 1.25, -0.25, -0.75, 10.25, -10.75, 31.25], np.float32)
    if in_bf16:
        w = spec.bf16_round(w)
    wt = torch.from_numpy(w).to(DEV)
    qw, sc = ops.int8_quantize(wt.to(torch.bfloat16) if in_bf16 else wt)
    q_ref, s_ref = spec.quantize_weight(w)
    assert list(q_ref[9, 1:7]) == [0, 2, 2, 0, -2, -2] and not q_ref[3].any() and s_ref[3] == 0
    np.testing.assert_array_equal(sc.cpu().numpy(), s_ref)
    np.testing.assert_array_equal(qw.cpu().numpy(), q_ref)


# ------------------------------------------------------------------------------------------------ 2. GEMV, no outliers
@pytest.mark.parametrize("N,K", GEMV_SHAPES)
def test_gemv_without_outliers_bit_exact(ops, N, K):
    _, q, s, qd, sd = weights(N, K)
    x = act((K,), f"x{K}")
    bias = spec.bf16_round(synth.normal((N,), "bias", 5, 0.1))
    res = spec.bf16_round(synth.normal((N,), "res", 5, 1.0))
    xd = dev_bf16(x)
    for b, r in ((None, None), (bias, None), (None, res), (bias, res)):
        y = ops.int8_gemv(xd, qd, sd, bias=None if b is None else dev_bf16(b),
                          residual=None if r is None else dev_bf16(r))
        ref = spec.linear(x, q, s, bias=b, residual=r)[0]
        np.testing.assert_array_equal(bits(y), bits(ref), err_msg=f"bias={b is not None} residual={r is not None}")


# ------------------------------------------------------------------------------------------------ 3. GEMV, outliers
def plant_outliers(x, n_out, name):
    """n_out outlier columns: the first column at exactly 6.0 (an outlier), its chunk neighbour column 1, the last
    column, then random ones; column 5 (inside the first chunk) holds 5.96875 — just below tau, NOT an outlier."""
    K = x.size
    x = x.copy()
    x[5] = 5.96875
    cols = [0, 1, K - 1][:n_out] if n_out <= 3 else None
    vals = [6.0, -7.5, 9.0]
    if cols is None:
        rng = _rng(f"{name}{K}")
        rest = rng.choice(np.setdiff1d(np.arange(2, K - 1), [5]), n_out - 3, replace=False)
        cols = [0, 1, K - 1] + sorted(rest.tolist())
        vals = vals + (rng.uniform(6.0, 12.0, n_out - 3) * rng.choice([-1.0, 1.0], n_out - 3)).tolist()
    x[cols] = spec.bf16_round(np.array(vals[:len(cols)], np.float32))
    return x, np.array(sorted(cols))


def outlier_tol(ref, x, O, K):
    """|y - ref| <= |ref| 2^-7 + eps, the form of test_gemv_matches_reference: 2^-7 |ref| covers the bf16 output
    rounding (2^-8 relative) twice over. There eps = 1e-3 sqrt(K / 4096) * 0.02 * mean|x| * 4: the fp32 accumulation
    allowance, 4e-3 / 64 of the typical output magnitude 0.02 sqrt(K) mean|x| (0.02 = the weights' standard
    deviation). Here the integer part of the sum is exact; what is left in fp32 is the dequantization of the integer
    sum (three roundings), the |O| outlier products and their sum, and the final additions. Their magnitude follows
    the same law with the outlier columns counted by their own size: 0.02 (sqrt(K) mean|x| over the other columns +
    the outliers' 2-norm), so eps keeps the factor 4e-3 / 64 on that magnitude."""
    rest = np.abs(x[~O]).mean() if (~O).any() else 0.0
    mag = 0.02 * (np.sqrt(K) * rest + np.sqrt((x[O].astype(np.float64) ** 2).sum()))
    return np.abs(ref) * 2 ** -7 + (4e-3 / 64) * mag


@pytest.mark.parametrize("n_out", [1, 3, 40])
@pytest.mark.parametrize("N,K", GEMV_SHAPES)
def test_gemv_with_outliers(ops, N, K, n_out):
    _, q, s, qd, sd = weights(N, K)
    x, cols = plant_outliers(act((K,), f"x{K}"), n_out, "po")
    a, s_x, O = spec.quantize_act(x)
    np.testing.assert_array_equal(np.nonzero(O)[0], cols)  # 5.96875 is not an outlier, 6.0 is
    assert s_x[0] == np.float32(5.96875)
    xd = dev_bf16(x)
    # the outlier set the kernel used, exactly: with the weight columns of the true outlier columns zeroed the outlier
    # term is exactly 0 and y must equal the spec's bits, which depend on s_x = max over exactly the other columns
    # (5.96875 counted in, 6.0 counted out) and on every outlier column being zeroed in the int8 image
    qz = q.copy()
    qz[:, cols] = 0
    yz = ops.int8_gemv(xd, torch.from_numpy(qz).to(DEV), sd)
    np.testing.assert_array_equal(bits(yz), bits(spec.linear(x, qz, s)[0]))
    # ... and through the prefill quantizer on the same row
    xq, sx, clist, count, flags = ops.int8_quantize_act(xd.view(1, K))
    assert int(count.item()) == n_out
    np.testing.assert_array_equal(clist[:n_out].cpu().numpy(), cols)
    np.testing.assert_array_equal(xq.cpu().numpy(), a)
    # the full product against the spec in float64
    bias = spec.bf16_round(synth.normal((N,), "bias", 5, 0.1))
    y = ops.int8_gemv(xd, qd, sd, bias=dev_bf16(bias)).float().cpu().numpy()
    ref = spec.linear_exact(x, q, s, bias=bias)[0]
    err = np.abs(y - ref) - outlier_tol(ref, x, O, K)
    print(f"N={N} K={K} |O|={n_out}: max |y - ref| {np.abs(y - ref).max():.3e}, max over the bound {err.max():.3e}")
    assert err.max() <= 0


def test_gemv_every_column_an_outlier(ops):
    N, K = 640, 256
    _, q, s, qd, sd = weights(N, K)
    rng = _rng("allout")
    x = spec.bf16_round((rng.uniform(6.0, 12.0, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32))
    a, s_x, O = spec.quantize_act(x)
    assert O.all() and s_x[0] == 0 and not a.any()
    y = ops.int8_gemv(dev_bf16(x), qd, sd).float().cpu().numpy()
    ref = spec.linear_exact(x, q, s)[0]
    assert np.all(np.isfinite(y))
    err = np.abs(y - ref) - outlier_tol(ref, x, O, K)
    print(f"all {K} columns outliers: max |y - ref| {np.abs(y - ref).max():.3e}, max over the bound {err.max():.3e}")
    assert err.max() <= 0
    # tau <= 0 disables the decomposition: the same x is then an ordinary row, bit-exact
    y0 = ops.int8_gemv(dev_bf16(x), qd, sd, threshold=0.0)
    np.testing.assert_array_equal(bits(y0), bits(spec.linear(x, q, s, tau=0.0)[0]))


# ------------------------------------------------------------------------------------------------ 4. fused RMSNorm
def test_gemv_fused_rmsnorm(ops):
    """The prologue's sum of squares runs in another order than the oracle's, a 1-ulp difference of the normalised
    row can move an int8 step: not bit-exact. The kernel must be as close to the exact product as the spec evaluated
    on the oracle's normalised row (tests/parity.py constants)."""
    N, K = 1536, 1024
    _, q, s, qd, sd = weights(N, K)
    x = spec.bf16_round(synth.normal((K,), "xf", 5, 2.0))
    nw = spec.bf16_round(1.0 + synth.normal((K,), "nw", 5, 0.2))
    res = spec.bf16_round(synth.normal((N,), "res", 5, 1.0))
    bias = spec.bf16_round(synth.normal((N,), "bias", 5, 0.1))
    y = ops.int8_gemv(dev_bf16(x), qd, sd, bias=dev_bf16(bias), residual=dev_bf16(res), norm_weight=dev_bf16(nw),
                      eps=1e-5).float().cpu().numpy().astype(np.float64)
    xn = om.rms_norm(torch.from_numpy(x).bfloat16(), torch.from_numpy(nw).bfloat16(), 1e-5).float().numpy()
    exact = xn.astype(np.float64) @ spec.dequantize_weight(q, s).T + bias + res
    ref = spec.linear(xn, q, s, bias=bias, residual=res)[0].astype(np.float64)
    top = np.abs(exact).max()
    for name, f in (("max", lambda e: np.abs(e).max()), ("rms", lambda e: np.sqrt((e ** 2).mean()))):
        got, own = f(y - exact), f(ref - exact)
        print(f"fused norm {name}: kernel {got:.4e}, spec {own:.4e}")
        assert got <= parity.ACC_FACTOR * own + parity.ACC_SLACK * top, name


# ------------------------------------------------------------------------------------------------ 5. dual SwiGLU
@pytest.mark.parametrize("N,K", [(11008, 4096), (640, 1376)])
@pytest.mark.parametrize("n_out", [0, 3])
def test_gemv_swiglu(ops, N, K, n_out):
    _, q1, s1, q1d, s1d = weights(N, K, "s1")
    _, q2, s2, q2d, s2d = weights(N, K, "s2")
    x = act((K,), f"xs{K}")
    if n_out:
        x, _ = plant_outliers(x, n_out, "ps")
    y = ops.int8_gemv_swiglu(dev_bf16(x), q1d, s1d, q2d, s2d).float().cpu().numpy()
    a = spec.linear_exact(x, q1, s1)[0]
    b = spec.linear_exact(x, q2, s2)[0]
    ref = (a / (1 + np.exp(-a))) * b
    err = np.abs(y - ref) - np.abs(ref) * 2 ** -6
    print(f"swiglu N={N} K={K} |O|={n_out}: max |y - ref| {np.abs(y - ref).max():.3e}, over the bound {err.max():.3e}")
    assert err.max() <= 1e-3  # the bound of test_gemv_swiglu


# ------------------------------------------------------------------------------------------------ 6. quantize_act
@pytest.mark.parametrize("M,K", [(5, 1376), (130, 4096), (200, 256)])
def test_quantize_act_bit_exact(ops, M, K):
    x = act((M, K), f"qa{M}x{K}")
    x[1, :] = 0.0  # a row of zeros
    x[0, 3] = 6.0  # the same column from different rows
    x[M - 1, 3] = -11.0
    x[2, K - 1] = 7.0  # different columns, different rows
    x[3, 0] = -6.5
    x[4, 17] = 5.96875  # not an outlier
    x[4, 40], x[4, 41] = 8.0, -8.0  # two in one 16-B chunk
    x = spec.bf16_round(x)
    a, s_x, O = spec.quantize_act(x)
    assert sorted(np.nonzero(O)[0].tolist()) == sorted({3, K - 1, 0, 40, 41}) and s_x[1] == 0
    xq, sx, cols, count, flags = ops.int8_quantize_act(dev_bf16(x))
    n = int(count.item())
    assert n == int(O.sum())
    got = cols[:n].cpu().numpy()
    assert set(got.tolist()) == set(np.nonzero(O)[0].tolist()) and len(set(got.tolist())) == n
    np.testing.assert_array_equal(flags.cpu().numpy() != 0, O)
    np.testing.assert_array_equal(sx.cpu().numpy(), s_x)
    np.testing.assert_array_equal(xq.cpu().numpy(), a)
    # tau <= 0: no outlier column
    xq0, sx0, _, count0, _ = ops.int8_quantize_act(dev_bf16(x), threshold=0.0)
    a0, s0, _ = spec.quantize_act(x, tau=0.0)
    assert int(count0.item()) == 0
    np.testing.assert_array_equal(sx0.cpu().numpy(), s0)
    np.testing.assert_array_equal(xq0.cpu().numpy(), a0)


# ------------------------------------------------------------------------------------------------ 7. GEMM
GEMM_SHAPES = [(200, 768, 256), (5, 640, 1376), (130, 4096, 11008), (2, 77, 256)]


def run_gemm(ops, x, qd, sd, bias=None, residual=None):
    xd = dev_bf16(x)
    xq, sx, cols, count, _ = ops.int8_quantize_act(xd)
    return ops.int8_gemm(xd, xq, sx, cols, count, qd, sd, bias=None if bias is None else dev_bf16(bias),
                         residual=None if residual is None else dev_bf16(residual))


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_without_outliers_bit_exact(ops, M, N, K):
    _, q, s, qd, sd = weights(N, K)
    x = act((M, K), f"gx{M}x{K}")
    bias = spec.bf16_round(synth.normal((N,), "bias", 5, 0.1))
    res = spec.bf16_round(synth.normal((M, N), "gres", 5, 1.0))
    for b, r in ((None, None), (bias, res)):
        y = run_gemm(ops, x, qd, sd, b, r)
        np.testing.assert_array_equal(bits(y), bits(spec.linear(x, q, s, bias=b, residual=r)))


@pytest.mark.parametrize("n_out", [1, 17])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_with_outlier_columns(ops, M, N, K, n_out):
    _, q, s, qd, sd = weights(N, K)
    x = act((M, K), f"gx{M}x{K}")
    rng = _rng(f"go{M}{K}{n_out}")
    cols = np.array([0] if n_out == 1 else sorted([0, 1, K - 1] + rng.choice(np.arange(2, K - 1), n_out - 3,
                                                                              replace=False).tolist()))
    for i, c in enumerate(cols):  # each outlier column is planted in one row; the other rows keep N(0, 1) there
        x[(3 * i) % M, c] = [6.0, -9.5, 7.25][i % 3]
    x = spec.bf16_round(x)
    a, s_x, O = spec.quantize_act(x)
    np.testing.assert_array_equal(np.nonzero(O)[0], cols)
    y = run_gemm(ops, x, qd, sd, None, None).float().cpu().numpy()
    ref = spec.linear_exact(x, q, s)
    tol = np.stack([outlier_tol(ref[m], x[m], O, K) for m in range(M)])
    print(f"M={M} N={N} K={K} |O|={n_out}: max |y - ref| {np.abs(y - ref).max():.3e}, "
          f"max over the bound {(np.abs(y - ref) - tol).max():.3e}")
    assert (np.abs(y - ref) - tol).max() <= 0


def test_gemm_integer_tile_exact(ops):
    """Asymmetric small integers straight into the A and B operands, scales 127 * 127 * C = 1: y is the int32 tile."""
    M, N, K = 200, 768, 256
    A = np.zeros((M, K), np.int8)
    for m in range(M):
        A[m, (7 * m + 3) % K] += 1 + m % 3
        A[m, (13 * m + 5) % K] -= 2
    B = _rng("itile").integers(-40, 41, (N, K)).astype(np.int8)
    acc = A.astype(np.int64) @ B.astype(np.int64).T
    assert np.abs(acc).max() <= 256  # exact in bf16
    one = lambda n: torch.full((n,), 127.0, dtype=torch.float32, device=DEV)
    zero_i = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = ops.int8_gemm(torch.zeros(M, K, dtype=torch.bfloat16, device=DEV), torch.from_numpy(A).to(DEV), one(M),
                      torch.zeros(K, dtype=torch.int32, device=DEV), zero_i, torch.from_numpy(B).to(DEV), one(N))
    np.testing.assert_array_equal(y.float().cpu().numpy().astype(np.int64), acc)


# ------------------------------------------------------------------------------------------------ 8. one format
@pytest.mark.parametrize("N,K", GEMV_SHAPES)
def test_gemv_equals_gemm_rows(ops, N, K):
    _, q, s, qd, sd = weights(N, K)
    x = act((K,), f"x{K}")
    y1 = ops.int8_gemv(dev_bf16(x), qd, sd)
    y2 = run_gemm(ops, np.stack([x, x]), qd, sd)
    np.testing.assert_array_equal(bits(y2[0]), bits(y1))
    np.testing.assert_array_equal(bits(y2[1]), bits(y1))


# ------------------------------------------------------------------------------------------------ 9. model level
MODEL_CFGS = {
    "mha": ("Llama-2-7b-hf", dict(n_layer=2, n_embd=512, n_head=4, intermediate_size=640, vocab_size=1000,
                                   padding_multiple=64, block_size=256)),
    "neox": ("pythia-160m", dict(n_layer=2, n_embd=512, n_head=4, intermediate_size=640, vocab_size=1000,
                                  padding_multiple=64, block_size=256)),
}


def _cfg(key):
    from lit_gpt import Config

    name, kw = MODEL_CFGS[key]
    return Config.from_name(name, **kw)


def _state(cfg, seed, outlier_channel=False):
    sd = {k: (spec.bf16_round(v) if v.dtype == np.float32 else v) for k, v in synth.state_dict(cfg, seed=seed).items()}
    if outlier_channel:
        sd["transformer.wte.weight"][:, 7] = spec.bf16_round(sd["transformer.wte.weight"][:, 7] * 40)
    return sd


def build_gpu_model(cfg, sd, max_seq):
    from lit_gpt import GPT
    from lit_gpt.quantize import Int8Linear, QuantizedPrecision

    model = GPT(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(device=DEV, dtype=torch.bfloat16)
    QuantizedPrecision("bnb.int8").convert_module(model, DEV)
    assert isinstance(model.lm_head, Int8Linear)
    assert not any(type(m) is torch.nn.Linear for m in model.modules())
    model.max_seq_length = max_seq
    model.set_kv_cache(1, device=DEV)
    return model.eval()


class Int8Oracle(om.OracleGPT):
    """The oracle with every Linear replaced by the spec's: its bf16 rounding points (dtype bf16) or the same
    decomposition accumulated in float64."""

    def __init__(self, cfg, sd, dtype):
        super().__init__(cfg, sd, dtype=dtype)
        self.q8 = {}
        self.outlier_calls = 0

    def _lin(self, prefix, x):
        if prefix not in self.q8:
            self.q8[prefix] = spec.quantize_weight(self.p[f"{prefix}.weight"].float().numpy())
        q, s = self.q8[prefix]
        b = self.p.get(f"{prefix}.bias")
        b = None if b is None else b.float().numpy()
        xn = x.float().numpy()
        self.outlier_calls += int(spec.quantize_act(xn)[2].any())
        if self.dtype == torch.bfloat16:
            return torch.from_numpy(spec.linear(xn, q, s, bias=b)).to(torch.bfloat16)
        return torch.from_numpy(spec.linear_exact(xn, q, s, bias=b))


class _OutlierWatch:
    """Counts the product's Linear calls that saw a non-empty outlier set (eager runs only)."""

    def __init__(self, ops):
        self.ops, self.seen = ops, 0

    def __enter__(self):
        ops = self.ops
        self._orig = (ops.int8_quantize_act, ops.int8_gemv)

        def qact(x, **kw):
            out = self._orig[0](x, **kw)
            self.seen += int(out[3].item() > 0)
            return out

        def gemv(x, qw, sc, **kw):
            xn = x if kw.get("norm_weight") is None else ops.rmsnorm(x.view(1, -1), kw["norm_weight"],
                                                                     kw.get("eps", 1e-5))
            self.seen += int((xn.float().abs() >= spec.TAU).any().item())
            return self._orig[1](x, qw, sc, **kw)

        ops.int8_quantize_act, ops.int8_gemv = qact, gemv
        return self

    def __exit__(self, *exc):
        self.ops.int8_quantize_act, self.ops.int8_gemv = self._orig


@pytest.mark.parametrize("key,outlier_channel", [("mha", False), ("neox", False), ("mha", True)])
@torch.inference_mode()
def test_model_teacher_forced_logits(ops, key, outlier_channel):
    """12-token prefill + 8 decode steps against the spec oracle in bf16 and in float64 (tests/parity.py bounds).
    Random-init activations never reach 6.0, and a uniformly larger embedding table would not change that (every
    Linear input has passed a norm, which divides a uniform scale out again); so the outlier sub-case scales ONE
    embedding channel by 40 — the shape LLM.int8 outliers take, a few large feature dimensions — and checks that
    Linear calls on both sides really saw outlier columns."""
    cfg = _cfg(key)
    sd = _state(cfg, 21, outlier_channel)
    T, N = 12, 8
    model = build_gpu_model(cfg, sd, T + N)
    prompt = torch.from_numpy(synth.token_ids(T, cfg.vocab_size, seed=21))
    stream = torch.from_numpy(synth.token_ids(N, cfg.vocab_size, seed=22))
    with _OutlierWatch(ops) as watch:
        got = [model(prompt.view(1, -1).to(DEV), torch.arange(T, device=DEV))[0, -1].float().cpu()]
        for i in range(N):
            got.append(model(stream[i:i + 1].view(1, 1).to(DEV), torch.tensor([T + i], device=DEV))[0, -1].float()
                       .cpu())
    exp = {}
    for dt in (torch.bfloat16, torch.float64):
        ref = Int8Oracle(cfg, sd, dt)
        ref.set_kv_cache(T + N)
        out = [ref.forward(prompt, torch.arange(T))[-1]]
        for i in range(N):
            out.append(ref.forward(stream[i:i + 1], torch.tensor([T + i]))[-1])
        exp[dt] = out
        assert (ref.outlier_calls > 0) == outlier_channel
    assert (watch.seen > 0) == outlier_channel, watch.seen
    for i, g in enumerate(got):
        parity.check_step(g, exp[torch.bfloat16][i], exp[torch.float64][i], f"int8 {key} step {i}")


@pytest.mark.parametrize("key", ["mha", "neox"])
@torch.inference_mode()
def test_model_generate_graph_equals_eager_and_sampling_reproducible(key):
    from generate.base import generate

    cfg = _cfg(key)
    sd = _state(cfg, 31)
    T, N = 12, 8
    model = build_gpu_model(cfg, sd, T + N)
    prompt = torch.from_numpy(synth.token_ids(T, cfg.vocab_size, seed=31)).to(DEV)

    def run(**kw):
        for b in model.transformer.h:
            b.attn.kv_cache.reset_parameters()
        return generate(model, prompt, T + N, **kw).cpu()

    y_graph = run(temperature=0.0, use_graph=True)
    y_eager = run(temperature=0.0, use_graph=False)
    assert y_graph.shape == (T + N,) and torch.equal(y_graph, y_eager)
    streams = []
    for _ in range(2):
        torch.manual_seed(7)
        streams.append(run(temperature=0.8, top_k=50))
    assert torch.equal(streams[0], streams[1])


# ------------------------------------------------------------------------------------------------ 10. refusals
def _no_model(monkeypatch):
    import generate.base as gb

    def boom(*a, **kw):
        raise AssertionError("the model was instantiated before the refusal")

    monkeypatch.setattr(gb, "GPT", boom)
    return gb


def test_build_model_refuses_int8_moe(monkeypatch):
    from lit_gpt import Config

    gb = _no_model(monkeypatch)
    with pytest.raises(NotImplementedError, match="bnb.int8"):
        gb.build_model(Config.from_name("Mixtral-8x7B-v0.1"), quantize="bnb.int8", device=DEV)


def test_build_model_refuses_int8_tensor_parallel(monkeypatch):
    from lit_gpt import Config

    class Fabric:
        world_size, global_rank = 2, 0

    gb = _no_model(monkeypatch)
    with pytest.raises(NotImplementedError, match="bnb.int8"):
        gb.build_model(Config.from_name("Llama-2-7b-hf"), quantize="bnb.int8", device=DEV, fabric=Fabric())
