"""The weight kernels, bit for bit, on operands with ONE right answer (tests/exact_operands.py).

Every other test of the GEMVs and GEMMs over a weight format compares with an fp64 product under a bf16 tolerance, on
Gaussian weights: a single wrong column sits at the edge of that tolerance, the codes and scales are the few a
quantizer emits for N(0, 0.02^2), and nothing looks at what a kernel does beside its operands. Here:

 (a) an identity GEMM, X = v I, must return the dequantized weight: every (n, k), code and scale in one launch;
 (b) one-hot sweeps of the decode GEMVs, x = v e_k, must return column k of the weight (full-range family);
 (c) dense products on the integer family, whose fp32 sum is exact in any order, must equal the int64 product pushed
     through the kernels' documented rounding points: h = bf16(sum + bias), y = bf16(h + residual),
     SwiGLU y = bf16(bf16(silu(bf16 a)) * bf16 b);
 (d) the dense calls again with every operand a view into an arena of NaN / 0xFF poison and the output a view into a
     sentinel-filled buffer: the same bits, finite, and not a byte changed outside the views. All accesses of a correct
     kernel stay inside the views, and the arenas keep a wrong one inside allocated memory.

There is no tolerance in this file: outputs are compared as bf16 values with +0 == -0 and NaN equal to nothing.

SwiGLU forms: fc_1 holds positive values only (a >= 32, where bf16(silu(bf16 a)) == bf16 a for any sane exp), so the
sign decode of the dual instantiations is covered only through fc_2.

Out of scope: int8 (tests/test_gpu_int8.py is already bit-exact against its integer spec), the MoE expert and grouped
kernels, LoRA, attention, and the fused RMSNorm (not exact).
"""

import functools

import pytest
import torch

import exact_operands as xo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
Q4 = ("int4", "nf4", "fp4")
ROWS_FORMATS = Q4 + ("fp8",)  # the formats with a multi-row decode GEMV
SWIGLU_EXPS = (-100, 100)  # fc_2 of the one-hot SwiGLU sweeps: 64 a * 64 b stays a normal bf16


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


@functools.lru_cache(maxsize=None)
def weight(family, fmt, N, K, positive=False, exp_range=None, seed=0):
    """(Weight, its operands on the device), built once per module."""
    w = (xo.full_range(fmt, N, K, exp_range) if family == "full" else xo.integer(fmt, N, K, seed, positive))
    return w, tuple(t.to(DEV) for t in w.operands)


@pytest.fixture(scope="module", autouse=True)
def release_weights():
    """The cached weights (host W' and device operands) live as long as this module's tests, no longer."""
    yield
    weight.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def dev(t):
    return None if t is None else t.to(DEV, torch.bfloat16)


def assert_same(y, expected, what):
    """y (bf16, device) against the expected values (fp32, exact in bf16): equal as numbers, so +0 == -0, and a NaN
    or a wrong infinity is a mismatch."""
    y = y.float().cpu()
    assert y.shape == expected.shape, f"{what}: shape {tuple(y.shape)} vs {tuple(expected.shape)}"
    bad = ~(y == expected)
    if bool(bad.any()):
        at = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ; first at {at}: "
                             f"got {float(y[at])!r}, expected {float(expected[at])!r}")


# ------------------------------------------------------------------------------------------------ the entry points
def gemv(ops, w, o, x, **kw):
    if w.fmt == "bf16":
        return ops.bf16_gemv(x, o[0], **kw)
    if w.fmt == "fp8":
        return ops.fp8_gemv(x, *o, **kw)
    if w.fmt == "mxfp4":
        return ops.mxfp4_gemv(x, *o, **kw)
    return ops.q4_gemv(x, o[0], o[1], w.N, w.K, w.group, xo.Q4_FMT[w.fmt], **kw)


def gemv_swiglu(ops, w, o1, o2, x, **kw):
    if w.fmt == "bf16":
        return ops.bf16_gemv_swiglu(x, o1[0], o2[0], **kw)
    if w.fmt == "fp8":
        return ops.fp8_gemv_swiglu(x, *o1, *o2, **kw)
    if w.fmt == "mxfp4":
        return ops.mxfp4_gemv_swiglu(x, *o1, *o2, **kw)
    return ops.q4_gemv_swiglu(x, *o1, *o2, w.N, w.K, w.group, xo.Q4_FMT[w.fmt], **kw)


def gemv_rows(ops, w, o, x, **kw):
    if w.fmt == "fp8":
        return ops.fp8_gemv_rows(x, *o, **kw)
    return ops.q4_gemv_rows(x, o[0], o[1], w.N, w.K, w.group, xo.Q4_FMT[w.fmt], **kw)


def gemv_swiglu_rows(ops, w, o1, o2, x, **kw):
    if w.fmt == "fp8":
        return ops.fp8_gemv_swiglu_rows(x, *o1, *o2, **kw)
    return ops.q4_gemv_swiglu_rows(x, *o1, *o2, w.N, w.K, w.group, xo.Q4_FMT[w.fmt], **kw)


def gemm(ops, entry, w, o, x, **kw):
    if entry == "fp8_gemm":
        return ops.fp8_gemm(x, *o, **kw)
    if entry == "mxfp4_gemm":
        return ops.mxfp4_gemm(x, *o, **kw)
    if entry == "bf16_gemm":
        return ops.bf16_gemm(x, o[0], **kw)
    if entry == "q4_gemm":
        return ops.q4_gemm(x, o[0], o[1], w.N, w.K, w.group, xo.Q4_FMT[w.fmt], **kw)
    assert entry == "q4_gemm_fused"
    if w.fmt == "bf16":
        return ops.q4_gemm_fused(x, o[0], None, w.N, w.K, 64, 2, **kw)
    return ops.q4_gemm_fused(x, o[0], o[1], w.N, w.K, w.group, xo.Q4_FMT[w.fmt], **kw)


def gemm_swiglu(ops, w, o1, o2, x, **kw):
    if w.fmt == "bf16":
        return ops.q4_gemm_swiglu(x, o1[0], None, o2[0], None, w.N, w.K, 64, 2, **kw)
    return ops.q4_gemm_swiglu(x, o1[0], o1[1], o2[0], o2[1], w.N, w.K, w.group, xo.Q4_FMT[w.fmt], **kw)


GEMM_CASES = [(entry, fmt, N, K) for entry, fmts in xo.GEMM_FORMATS.items() for fmt in fmts
              for N, K in xo.GEMM_SHAPES[entry]]
GEMV_CASES = [(fmt, N, K) for fmt in xo.FORMATS for N, K in xo.gemv_shapes(fmt)]
ROWS_CASES = [c for c in GEMV_CASES if c[0] in ROWS_FORMATS]


# ------------------------------------------------------------------------------------------------ (a) identity GEMM
def identity_runs(ops, entry, fmt, N, K):
    """X = v I at M = K, at M = K + 1 with a zero last row (the M tail of a tile), and its first 64 rows (the short
    prompt's tile): Y[m] must be v W'[:, m]."""
    w, o = weight("full", fmt, N, K)
    v2 = 1.0 if fmt == "mxfp4" else 2.0  # 6 * 2^125 * 2 is no bf16
    for M, v in ((K, 1.0), (K + 1, v2), (min(K, 64), 1.0)):
        d = min(M, K)
        x = torch.zeros(M, K)
        x[torch.arange(d), torch.arange(d)] = v
        expected = torch.zeros(M, N)
        expected[:d] = xo.bf16_round(v * w.deq.T[:d].double())
        assert_same(gemm(ops, entry, w, o, dev(x)), expected, f"{entry} {fmt} N={N} K={K} M={M} v={v}")


@pytest.mark.parametrize("entry,fmt,N,K", GEMM_CASES)
def test_identity_gemm_returns_the_weight(ops, entry, fmt, N, K):
    identity_runs(ops, entry, fmt, N, K)


@pytest.mark.parametrize("fmt", xo.GEMM_FORMATS["q4_gemm_fused"])
@pytest.mark.parametrize("env,K", xo.Q4F_IDENTITY_ENV)
def test_identity_fused_gemm_wide_tiles_and_split_k(ops, fmt, env, K, monkeypatch):
    assert (136, K) in xo.GEMM_SHAPES["q4_gemm_fused"]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if "LGA_Q4F_SPLITS" in env:  # this shape splits
        assert ops.load_library().lga_q4f_workspace_bytes(K, 136, K, 0) > 0
    identity_runs(ops, "q4_gemm_fused", fmt, 136, K)


# ------------------------------------------------------------------------------------------------ (b) one-hot sweeps
def one_hot(cols, K, values):
    x = torch.zeros(len(cols), K)
    x[torch.arange(len(cols)), torch.tensor(cols)] = values
    return dev(x)


@pytest.mark.parametrize("fmt,N,K", GEMV_CASES)
def test_one_hot_gemv_returns_the_column(ops, fmt, N, K):
    w, o = weight("full", fmt, N, K)
    cols = xo.one_hot_columns(K, seed=N)
    x = one_hot(cols, K, 1.0)
    y = torch.empty(len(cols), N, dtype=torch.bfloat16, device=DEV)
    for i in range(len(cols)):
        gemv(ops, w, o, x[i], out=y[i])
    assert_same(y, w.deq.T[cols].contiguous(), f"gemv {fmt} N={N} K={K}, row = column index in {cols[:4]}...")


@pytest.mark.parametrize("fmt", Q4)
@pytest.mark.parametrize("N,K", xo.Q4_GEMV_VARIANT_SHAPES)
@pytest.mark.parametrize("variant", xo.Q4_GEMV_VARIANTS)
def test_one_hot_q4_gemv_variants(ops, fmt, N, K, variant):
    w, o = weight("full", fmt, N, K)
    cols = xo.one_hot_columns(K, seed=variant + 1)
    x = one_hot(cols, K, 2.0)
    y = torch.empty(len(cols), N, dtype=torch.bfloat16, device=DEV)
    for i in range(len(cols)):
        gemv(ops, w, o, x[i], out=y[i], variant=variant)
    assert_same(y, xo.bf16_round(2.0 * w.deq.T[cols].double()), f"q4_gemv {fmt} N={N} K={K} variant={variant}")


@pytest.mark.parametrize("fmt,N,K", GEMV_CASES)
def test_one_hot_gemv_swiglu(ops, fmt, N, K):
    w1, o1 = weight("integer", fmt, N, K, True)  # positive: a = 64 w1 >= 32
    w2, o2 = weight("full", fmt, N, K, False, SWIGLU_EXPS)
    cols = xo.one_hot_columns(K, seed=N + 1)
    x = one_hot(cols, K, 64.0)
    y = torch.empty(len(cols), N, dtype=torch.bfloat16, device=DEV)
    for i in range(len(cols)):
        gemv_swiglu(ops, w1, o1, o2, x[i], out=y[i])
    a, b = 64.0 * w1.deq.T[cols].double(), xo.bf16_round(64.0 * w2.deq.T[cols].double()).double()
    assert bool((a >= 32).all()) and torch.equal(xo.bf16_round(a).double(), a)
    assert_same(y, xo.bf16_round(a * b), f"gemv_swiglu {fmt} N={N} K={K}")


@pytest.mark.parametrize("fmt,N,K", ROWS_CASES)
def test_one_hot_gemv_rows(ops, fmt, N, K):
    w, o = weight("full", fmt, N, K)
    w1, o1 = weight("integer", fmt, N, K, True)
    w2, o2 = weight("full", fmt, N, K, False, SWIGLU_EXPS)
    cols = xo.one_hot_columns(K, seed=N + 2)
    n = len(cols)
    v = torch.tensor([1.0, 2.0, 0.5]).repeat(n)[:n]
    x, xs = one_hot(cols, K, v), one_hot(cols, K, 64.0)
    expected = xo.bf16_round(v.double()[:, None] * w.deq.T[cols].double())
    a, b = 64.0 * w1.deq.T[cols].double(), xo.bf16_round(64.0 * w2.deq.T[cols].double()).double()
    for M in (1, 3, 8):
        # every launch has M rows and every column runs at every M: where M does not divide the list, the last launch
        # starts at n - M and repeats some columns of the one before
        starts = sorted(set(range(0, n - M + 1, M)) | {n - M})
        y = torch.full((n, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        ys = torch.full((n, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        for i in starts:
            gemv_rows(ops, w, o, x[i:i + M], out=y[i:i + M])
            gemv_swiglu_rows(ops, w1, o1, o2, xs[i:i + M], out=ys[i:i + M])
        assert_same(y, expected, f"gemv_rows {fmt} N={N} K={K} M={M}")
        assert_same(ys, xo.bf16_round(a * b), f"gemv_swiglu_rows {fmt} N={N} K={K} M={M}")


# ------------------------------------------------------------------------------------------------ (c), (d) dense
class Plain:
    """Operands as they are, outputs freshly allocated."""

    def place(self, t, scale=False):
        return t

    def out(self, *shape):
        return torch.empty(*shape, dtype=torch.bfloat16, device=DEV)

    def check(self, what):
        pass


class Arenas:
    """Every operand a 16-B-aligned view 4 KB inside a buffer of poison (bf16 activations, weights, bias and residual:
    NaN 0x7FC0; code bytes and scales of any type (place(t, scale=True)): 0xFF, NaN for e4m3, e8m0, bf16 and fp32, the
    extreme code for the 4-bit formats); every output a view into a buffer of the sentinel 0x5A5A."""
    PAD = 4096

    def __init__(self):
        self.inputs, self.outputs = [], []

    def _buffer(self, nbytes, pattern16):
        buf = torch.empty(2 * self.PAD + (nbytes + 15) // 16 * 16, dtype=torch.uint8, device=DEV)
        buf.view(torch.int16).fill_(pattern16)
        return buf

    def place(self, t, scale=False):
        if t is None:
            return None
        nbytes = t.numel() * t.element_size()
        buf = self._buffer(nbytes, 0x7FC0 if t.dtype == torch.bfloat16 and not scale else -1)
        view = buf[self.PAD:self.PAD + nbytes].view(t.dtype).view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 0 and view.is_contiguous()
        self.inputs.append((buf, buf.clone()))
        return view

    def out(self, *shape):
        nbytes = 2 * int(torch.Size(shape).numel())
        buf = self._buffer(nbytes, 0x5A5A)
        self.outputs.append((buf, nbytes))
        return buf[self.PAD:self.PAD + nbytes].view(torch.bfloat16).view(*shape)

    def check(self, what):
        torch.cuda.synchronize()
        for buf, before in self.inputs:
            assert torch.equal(buf, before), f"{what}: an operand's arena was written"
        for buf, nbytes in self.outputs:
            outside = torch.cat([buf[:self.PAD], buf[self.PAD + nbytes:]])
            assert bool((outside == 0x5A).all()), f"{what}: a store outside the output"


def placed(mem, o):
    """A weight's operands (weight,) or (codes, scales) through mem: the second one is the scales."""
    return tuple(mem.place(t, scale=i == 1) for i, t in enumerate(o))


def dense_operands(w, shape_x, epilogue, positive=False, M=None):
    x = xo.activations(shape_x, seed=w.K + (M or 0), positive=positive)
    bias = xo.small_ints((w.N,), 11) if epilogue else None
    res = xo.small_ints((w.N,) if M is None else (M, w.N), 12) if epilogue else None
    xo.assert_order_free(x, w.deq, bias, xo.UNIT[w.fmt])
    return x, bias, res


def dense_gemv(ops, fmt, N, K, epilogue, mem, **kw):
    w, o = weight("integer", fmt, N, K)
    x, bias, res = dense_operands(w, (K,), epilogue)
    y = gemv(ops, w, placed(mem, o), mem.place(dev(x)), bias=mem.place(dev(bias)),
             residual=mem.place(dev(res)), out=mem.out(N), **kw)
    return y, xo.expect_linear(x, w.deq, bias, res)


def dense_gemv_swiglu(ops, fmt, N, K, mem, rows=None):
    w1, o1 = weight("integer", fmt, N, K, True)
    w2, o2 = weight("integer", fmt, N, K, False, None, 1)
    x, _, _ = dense_operands(w1, (K,) if rows is None else (rows, K), False, positive=True, M=rows)
    xo.assert_order_free(x, w2.deq, None, xo.UNIT[fmt])
    f = gemv_swiglu if rows is None else gemv_swiglu_rows
    y = f(ops, w1, placed(mem, o1), placed(mem, o2), mem.place(dev(x)),
          out=mem.out(N) if rows is None else mem.out(rows, N))
    return y, xo.expect_swiglu(x, w1.deq, w2.deq)


def dense_gemv_rows(ops, fmt, N, K, M, epilogue, mem):
    w, o = weight("integer", fmt, N, K)
    x, bias, res = dense_operands(w, (M, K), epilogue, M=M)
    y = gemv_rows(ops, w, placed(mem, o), mem.place(dev(x)), bias=mem.place(dev(bias)),
                  residual=mem.place(dev(res)), out=mem.out(M, N))
    return y, xo.expect_linear(x, w.deq, bias, res)


def dense_gemm(ops, entry, fmt, N, K, M, epilogue, mem):
    w, o = weight("integer", fmt, N, K)
    x, bias, res = dense_operands(w, (M, K), epilogue, M=M)
    y = gemm(ops, entry, w, placed(mem, o), mem.place(dev(x)), bias=mem.place(dev(bias)),
             residual=mem.place(dev(res)), out=mem.out(M, N))
    return y, xo.expect_linear(x, w.deq, bias, res)


def dense_gemm_swiglu(ops, fmt, N, K, M, mem):
    w1, o1 = weight("integer", fmt, N, K, True)
    w2, o2 = weight("integer", fmt, N, K, False, None, 1)
    x, _, _ = dense_operands(w1, (M, K), False, positive=True, M=M)
    xo.assert_order_free(x, w2.deq, None, xo.UNIT[fmt])
    y = gemm_swiglu(ops, w1, placed(mem, o1), placed(mem, o2), mem.place(dev(x)),
                    out=mem.out(M, N))
    return y, xo.expect_swiglu(x, w1.deq, w2.deq)


def in_arenas(run, what):
    """(d): run(mem) -> (y, expected) once plainly and once inside poisoned arenas."""
    y0, expected = run(Plain())
    mem = Arenas()
    y1, _ = run(mem)
    mem.check(what)
    assert bool(torch.isfinite(y1.float()).all()), f"{what}: not finite inside the arenas"
    assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)), f"{what}: other bits inside the arenas"
    assert_same(y1, expected, what + " (arenas)")


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("fmt,N,K", GEMV_CASES)
def test_dense_gemv(ops, fmt, N, K, epilogue):
    y, expected = dense_gemv(ops, fmt, N, K, epilogue, Plain())
    assert_same(y, expected, f"gemv {fmt} N={N} K={K} epilogue={epilogue}")


@pytest.mark.parametrize("fmt", Q4)
@pytest.mark.parametrize("N,K", xo.Q4_GEMV_VARIANT_SHAPES)
@pytest.mark.parametrize("variant", xo.Q4_GEMV_VARIANTS)
def test_dense_q4_gemv_variants(ops, fmt, N, K, variant):
    what = f"q4_gemv {fmt} N={N} K={K} variant={variant}"
    for epilogue in (False, True):
        y, expected = dense_gemv(ops, fmt, N, K, epilogue, Plain(), variant=variant)
        assert_same(y, expected, what)
    in_arenas(lambda mem: dense_gemv(ops, fmt, N, K, True, mem, variant=variant), what)


@pytest.mark.parametrize("fmt,N,K", GEMV_CASES)
def test_dense_gemv_swiglu(ops, fmt, N, K):
    y, expected = dense_gemv_swiglu(ops, fmt, N, K, Plain())
    assert_same(y, expected, f"gemv_swiglu {fmt} N={N} K={K}")


@pytest.mark.parametrize("fmt,N,K", ROWS_CASES)
def test_dense_gemv_rows(ops, fmt, N, K):
    for M in xo.ROWS_M:
        for epilogue in (False, True):
            y, expected = dense_gemv_rows(ops, fmt, N, K, M, epilogue, Plain())
            assert_same(y, expected, f"gemv_rows {fmt} N={N} K={K} M={M} epilogue={epilogue}")
        y, expected = dense_gemv_swiglu(ops, fmt, N, K, Plain(), rows=M)
        assert_same(y, expected, f"gemv_swiglu_rows {fmt} N={N} K={K} M={M}")


@pytest.mark.parametrize("M", xo.GEMM_M)
@pytest.mark.parametrize("entry,fmt,N,K", GEMM_CASES)
def test_dense_gemm(ops, entry, fmt, N, K, M):
    for epilogue in (False, True):
        y, expected = dense_gemm(ops, entry, fmt, N, K, M, epilogue, Plain())
        assert_same(y, expected, f"{entry} {fmt} N={N} K={K} M={M} epilogue={epilogue}")


@pytest.mark.parametrize("fmt", xo.GEMM_FORMATS["q4_gemm_fused"])
@pytest.mark.parametrize("env,M,K", xo.Q4F_DENSE_ENV)
def test_dense_fused_gemm_and_swiglu(ops, fmt, env, M, K, monkeypatch):
    """(c) and (d) of q4_gemm_fused and q4_gemm_swiglu under the planner's knobs: the short and the long prompt's
    tiles, the 256-wide tile, split-K."""
    assert (136, K) in xo.GEMM_SHAPES["q4_gemm_fused"]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if "LGA_Q4F_SPLITS" in env:
        assert ops.load_library().lga_q4f_workspace_bytes(M, 136, K, 0) > 0
        assert ops.load_library().lga_q4f_workspace_bytes(M, 136, K, 1) > 0
    what = f"fmt={fmt} N=136 K={K} M={M} {env}"
    y, expected = dense_gemm(ops, "q4_gemm_fused", fmt, 136, K, M, False, Plain())
    assert_same(y, expected, "q4_gemm_fused, no epilogue, " + what)
    in_arenas(lambda mem: dense_gemm(ops, "q4_gemm_fused", fmt, 136, K, M, True, mem), "q4_gemm_fused " + what)
    in_arenas(lambda mem: dense_gemm_swiglu(ops, fmt, 136, K, M, mem), "q4_gemm_swiglu " + what)


# ------------------------------------------------------------------------------------------------ (d) poisoned arenas
@pytest.mark.parametrize("fmt,N,K", GEMV_CASES)
def test_gemv_inside_poisoned_arenas(ops, fmt, N, K):
    in_arenas(lambda mem: dense_gemv(ops, fmt, N, K, True, mem), f"gemv {fmt} N={N} K={K}")
    in_arenas(lambda mem: dense_gemv_swiglu(ops, fmt, N, K, mem), f"gemv_swiglu {fmt} N={N} K={K}")


@pytest.mark.parametrize("fmt,N,K", ROWS_CASES)
def test_gemv_rows_inside_poisoned_arenas(ops, fmt, N, K):
    in_arenas(lambda mem: dense_gemv_rows(ops, fmt, N, K, 5, True, mem), f"gemv_rows {fmt} N={N} K={K} M=5")
    in_arenas(lambda mem: dense_gemv_swiglu(ops, fmt, N, K, mem, rows=8), f"gemv_swiglu_rows {fmt} N={N} K={K} M=8")


@pytest.mark.parametrize("M", [17, 129])  # both tile heights
@pytest.mark.parametrize("entry,fmt,N,K", GEMM_CASES)
def test_gemm_inside_poisoned_arenas(ops, entry, fmt, N, K, M):
    in_arenas(lambda mem: dense_gemm(ops, entry, fmt, N, K, M, True, mem), f"{entry} {fmt} N={N} K={K} M={M}")
