"""Per-kernel parity for the GPT-NeoX and ``--precision 32-true`` ops on the MI355X: the ten ops that
tests/test_gpu_kernels.py does not call — ``lga_layernorm``, ``lga_gelu`` (csrc/norm_rope.hip), the whole of
csrc/fp32.hip (``lga_f32_linear``, ``lga_f32_layernorm``, ``lga_f32_gelu``, ``lga_f32_add``,
``lga_f32_rope_kv_append``, ``lga_f32_attention``), ``lga_argmax_f32`` (csrc/sample.hip) and the fp32-row form of
``lga_embedding`` — each through ``lit_gpt.ops`` against a float64 reference of the same operation on the same
fp32 (or bf16) input bits, at every branch the kernels have (K % 4 != 0, bias-free LayerNorm, tanh GELU, GQA / MQA,
head sizes other than 64, L < 4, L across the 256-thread softmax stride, the 65,535-block grid cap, the largest
``max_seq``).

u = 2^-24 is the fp32 unit roundoff throughout. Every tolerance is derived next to its assertion from the kernel's
own rounding count or from the number formats, never from what the kernel returned; the measured maxima are written
in the docstrings for the reader.
"""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as om

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


def _seed(*key) -> int:
    """A stable seed from small ints (hash() of str is salted per process; this is not)."""
    s = 0x9E3779B9
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


def _normal(shape, *key, std=1.0, mean=0.0) -> np.ndarray:
    r = np.random.default_rng(_seed(*key))
    return (mean + std * r.standard_normal(shape)).astype(np.float32)


def _gpu(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offset_view(a: np.ndarray, off: int) -> torch.Tensor:
    """``a`` on the device as a contiguous view ``off`` elements into a fresh buffer (off = 1: a pointer aligned to
    the element size only)."""
    buf = torch.zeros(a.size + off, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[off:].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off * buf.element_size()
    return view


def round_to_bf16(x: np.ndarray) -> np.ndarray:
    """float64 -> the nearest bf16 value (ties to even, bf16 subnormals included), returned as float64: ONE rounding
    of the float64 reference (a cast through fp32 would round twice)."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)  # |x| = m * 2^e, m in [0.5, 1)
    q = np.exp2(np.maximum(e - 8, -133).astype(np.float64))  # 8 significant bits; the subnormal quantum is 2^-133
    y = np.rint(x / q) * q  # np.rint rounds half to even and keeps the sign of zero
    return np.where(np.abs(y) >= 2.0 ** 128, np.copysign(np.inf, x), y)


def _bf16_exact(x: np.ndarray) -> torch.Tensor:
    """float values that are already bf16-representable -> a bf16 tensor (the cast is exact)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    assert torch.equal(t.float(), torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
    return t


# =============================================================================================== 1. lga_f32_linear
LINEAR_SHAPES = [(1, 5, 64), (3, 7, 770), (2, 9, 3072), (2, 1030, 768), (8, 3, 11008), (1, 4, 1), (1, 1, 4)]


def _linear_case(M, N, K):
    x = _normal((M, K), 1, M, N, K)
    w = _normal((N, K), 2, M, N, K, std=0.05)
    b = _normal((N,), 3, M, N, K, std=0.5)
    res = _normal((M, N), 4, M, N, K)
    return x, w, b, res


def _linear_ref_and_bound(x, w, b, res):
    """fp64 x W^T (+ b) (+ res) and the per-element bound (ceil(K/64) + 8) u (sum_k |x_k w_k| + |b| + |res|): the
    kernel's longest rounding chain is ceil(K/64) fmas on one lane (the K % 4 != 0 loop; the float4 loop has the
    same count), 6 butterfly adds of wave_sum and the two adds of bias and residual — ceil(K/64) + 8 roundings, each
    at most u times a partial sum that sum |x w| + |b| + |res| dominates."""
    K = x.shape[1]
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref = x64 @ w64.T
    mag = np.abs(x64) @ np.abs(w64).T
    if b is not None:
        ref = ref + b.astype(np.float64)
        mag = mag + np.abs(b.astype(np.float64))
    if res is not None:
        ref = ref + res.astype(np.float64)
        mag = mag + np.abs(res.astype(np.float64))
    return ref, (math.ceil(K / 64) + 8) * U * mag


@pytest.mark.parametrize("use_bias,use_res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_f32_linear_matches_fp64(ops, M, N, K, use_bias, use_res):
    """K % 4 != 0 (770, 1: the scalar loop), K < 64 (lanes with no element), N % 4 != 0 (the partial last
    workgroup), all four bias / residual forms. Measured on the MI355X: error at most 0.13 of the bound (0.002 at
    K = 11008)."""
    x, w, b, res = _linear_case(M, N, K)
    b = b if use_bias else None
    res = res if use_res else None
    y = ops.f32_linear(_gpu(x), _gpu(w), bias=None if b is None else _gpu(b),
                       residual=None if res is None else _gpu(res))
    assert y.shape == (M, N) and y.dtype == torch.float32
    ref, bound = _linear_ref_and_bound(x, w, b, res)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    print(f"f32_linear {M}x{N}x{K} bias={use_bias} res={use_res}: max err / bound = {np.max(err / bound):.4f}")
    assert np.all(err <= bound), float(np.max(err / bound))


@pytest.mark.parametrize("which", ["x", "w", "both"])
def test_f32_linear_odd_float_offset_with_scalar_k(ops, which):
    """x and / or W as contiguous views one float into their buffers (4-B aligned only): with K % 4 != 0 the kernel
    takes scalar loads and the result must be as correct as from aligned pointers."""
    M, N, K = 3, 7, 770
    x, w, b, res = _linear_case(M, N, K)
    xd = _offset_view(x, 1) if which in ("x", "both") else _gpu(x)
    wd = _offset_view(w, 1) if which in ("w", "both") else _gpu(w)
    assert (xd.data_ptr() | wd.data_ptr()) % 16 != 0
    y = ops.f32_linear(xd, wd, bias=_gpu(b), residual=_gpu(res))
    ref, bound = _linear_ref_and_bound(x, w, b, res)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= bound), float(np.max(err / bound))


@pytest.mark.parametrize("which", ["x", "w"])
def test_f32_linear_refuses_misaligned_vector_k(ops, which):
    """The same offset with K % 4 == 0 would put the 16-B loads on a 4-B boundary: the call must raise the
    "16-B aligned" error and write nothing."""
    M, N, K = 3, 7, 768
    x, w, _, _ = _linear_case(M, N, K)
    xd = _offset_view(x, 1) if which == "x" else _gpu(x)
    wd = _offset_view(w, 1) if which == "w" else _gpu(w)
    y = torch.full((M, N), -777.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        ops.f32_linear(xd, wd, out=y)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.full((M, N), -777.0))


def test_f32_linear_refuses_65536_rows(ops):
    """grid.y holds at most 65,535 rows: M = 65536 must raise, not launch."""
    x = torch.zeros(65536, 4, dtype=torch.float32, device=DEV)
    w = torch.zeros(3, 4, dtype=torch.float32, device=DEV)
    y = torch.full((65536, 3), -777.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="lga_f32_linear"):
        ops.f32_linear(x, w, out=y)
    torch.cuda.synchronize()
    assert bool((y == -777.0).all())
    assert ops.f32_linear(x[:65535], w).shape == (65535, 3)  # the largest M it takes


# ======================================================================== 2. lga_f32_layernorm and lga_layernorm
LN_SHAPES = [(3, 768), (5, 1000), (7, 5), (2, 8192), (2, 11008), (4, 257), (1, 1), (2, 128)]
LN_EPS = 1e-5
LN_FAMILIES_F32 = {"N(0,1)": (0.0, 1.0), "N(0,1e-3)": (0.0, 1e-3), "1000+N(0,1)": (1000.0, 1.0),
                   "1e4+N(0,1)": (1e4, 1.0)}
LN_FAMILIES_BF16 = {"N(0,1)": (0.0, 1.0), "N(0,1e-3)": (0.0, 1e-3), "50+N(0,3)": (50.0, 3.0)}


def _ln_ref_and_bound(x, w, b):
    """fp64 LayerNorm (mean, biased variance, (x - mean) rstd w + b) and the fp32 bound per element
    u (8 max|x_row| rstd |w| + 4 (|ref| + |b|)): the first term is the rounding of the fp32 mean (a sum of n terms
    of size max|x| over a 256-lane tree, a few u max|x|) carried through x - mean and scaled by rstd |w|; the second
    is the two multiplies, the add and rstd's own error on the result."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    b64 = np.zeros_like(w64) if b is None else b.astype(np.float64)
    mean = x64.mean(axis=1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    ref = (x64 - mean) * rstd * w64 + b64
    xmax = np.abs(x64).max(axis=1, keepdims=True)
    bound = U * (8 * xmax * rstd * np.abs(w64) + 4 * (np.abs(ref) + np.abs(b64)))
    return ref, bound


def _ln_params(n, bias, *key):
    w = _normal((n,), 11, n, *key, std=0.2, mean=1.0)
    b = _normal((n,), 12, n, *key, std=0.1) if bias else None
    return w, b


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,n", LN_SHAPES)
def test_f32_layernorm_matches_fp64(ops, rows, n, bias):
    """n below, at, above and far above the 256-thread stride, n = 1, with and without bias, on unit-scale rows,
    rows where eps dominates the variance, and rows whose mean is 1e3 / 1e4 times their spread (a one-pass
    E[x^2] - mean^2 variance misses this bound about 100 times over there). Measured on the MI355X: error at most
    0.28 of the bound over all cases."""
    w, b = _ln_params(n, bias, 0)
    worst = 0.0
    for fi, (fam, (mean, std)) in enumerate(LN_FAMILIES_F32.items()):
        x = _normal((rows, n), 13, rows, n, fi, std=std, mean=mean)
        y = ops.layernorm(_gpu(x), _gpu(w), None if b is None else _gpu(b), LN_EPS)
        assert y.dtype == torch.float32 and y.shape == (rows, n)
        ref, bound = _ln_ref_and_bound(x, w, b)
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        worst = max(worst, ratio)
        assert np.all(err <= bound), (fam, ratio)
    print(f"f32_layernorm {rows}x{n} bias={bias}: max err / bound = {worst:.4f}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,n", LN_SHAPES)
def test_bf16_layernorm_matches_fp64(ops, rows, n, bias):
    """lga_layernorm on bf16 inputs and weights (rounded to bf16 first, then exact in the reference): fp32
    statistics and one bf16 cast, so |y - ref| <= 2^-8 |ref| (the output rounding, half a bf16 ulp is 2^-9 |ref| at
    worst 2^-8 below a power of two) plus the fp32 bound, and y is the correctly rounded bf16(ref) wherever the fp32
    error does not straddle a rounding boundary: at least 99 % of every case. Measured on the MI355X: the smallest
    share of exact matches over all cases is 99.71 % (4 x 257, 50 + N(0, 3))."""
    w, b = _ln_params(n, bias, 1)
    w = round_to_bf16(w)
    b = None if b is None else round_to_bf16(b)
    for fi, (fam, (mean, std)) in enumerate(LN_FAMILIES_BF16.items()):
        x = round_to_bf16(_normal((rows, n), 14, rows, n, fi, std=std, mean=mean))
        y = ops.layernorm(_bf16_exact(x).to(DEV), _bf16_exact(w).to(DEV),
                          None if b is None else _bf16_exact(b).to(DEV), LN_EPS)
        assert y.dtype == torch.bfloat16 and y.shape == (rows, n)
        ref, bound32 = _ln_ref_and_bound(x, w, b)
        got = y.float().cpu().numpy().astype(np.float64)
        err = np.abs(got - ref)
        bound = 2.0 ** -8 * np.abs(ref) + bound32
        assert np.all(err <= bound), (fam, float(np.max(err / np.maximum(bound, 1e-300))))
        share = float(np.mean(got == round_to_bf16(ref)))
        print(f"bf16 layernorm {rows}x{n} bias={bias} {fam}: {share:.4%} equal bf16(ref)")
        assert share >= 0.99, (fam, share)


# ============================================================================== 3. lga_gelu and lga_f32_gelu
def _all_bf16_values() -> np.ndarray:
    """Every bf16 value with 2^-126 <= |v| <= 64 once, and +0 / -0 (as float32; bf16 subnormal inputs are left out:
    whether the device keeps them is not this kernel's arithmetic), plus one trailing 0.5 so that the element count
    is odd."""
    bits = np.arange(0x0080, 0x4280 + 1, dtype=np.uint32)  # 2^-126 (exponent field 1) .. 64.0 (0x4280)
    bits = np.concatenate([bits, bits | 0x8000, np.array([0x0000, 0x8000, 0x3F00], dtype=np.uint32)])
    v = (bits << 16).view(np.float32)
    assert v.size % 2 == 1 and np.abs(v[:-3]).min() == 2.0 ** -126 and np.abs(v).max() == 64.0
    return v


def _gelu_ref(v: np.ndarray, approximate: str) -> np.ndarray:
    return F.gelu(torch.from_numpy(v.astype(np.float64)), approximate=approximate).numpy()


@pytest.mark.parametrize("approximate", ["none", "tanh"])
def test_bf16_gelu_exhaustive(ops, approximate):
    """Every bf16 input of the domain, each sent once (33,797 elements: a partial last workgroup). Against F.gelu
    in float64: |y - ref| <= 2^-8 |ref| + 2^-20 |v| — the bf16 output rounding plus the fp32 cancellation in
    1 + erf(x) (1 + tanh) for x << 0, which is u relative to 1, so about u |v| / 2 absolute and far above a bf16
    ulp of the tiny result there (the reference's own fp32 formula has it too); where the result is a bf16
    subnormal (|v| < 2^-125) the output rounding is the absolute 2^-134 instead. y must be the correctly rounded
    bf16(ref) on at least 99 % of the inputs, and the sign of every zero result (gelu(-0.0), the underflowed
    negative tail) must be what float64-then-round gives. Measured on the MI355X: 99.66 % (erf, 114 of 33,797
    differ) and 99.73 % (tanh, 90 differ) exact matches, no bound violation."""
    v = _all_bf16_values()
    y = ops.gelu(_bf16_exact(v).to(DEV), approximate)
    assert y.dtype == torch.bfloat16
    got = y.float().cpu().numpy()
    ref = _gelu_ref(v, approximate)
    err = np.abs(got.astype(np.float64) - ref)
    # 2^-134 is half the bf16 subnormal quantum: for |v| < 2^-125 the result 0.5 v is a bf16 subnormal, where even
    # the correctly rounded value is up to 2^-134 away (2^-7 |ref|), so the relative term alone cannot hold there
    bound = np.maximum(2.0 ** -8 * np.abs(ref), 2.0 ** -134) + 2.0 ** -20 * np.abs(v.astype(np.float64))
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (bad.size, v[bad[:8]], got[bad[:8]], ref[bad[:8]])
    want = round_to_bf16(ref)
    share = float(np.mean(got.astype(np.float64) == want))
    print(f"bf16 gelu {approximate}: {share:.4%} equal bf16(ref) ({int(np.sum(got != want))} of {v.size} differ)")
    assert share >= 0.99, share
    zero = want == 0.0
    assert zero[-3] and zero[-2] and np.signbit(want[-2]) and not np.signbit(want[-3])  # +0 -> +0, -0 -> -0
    assert np.signbit(want[np.flatnonzero(v == -64.0)[0]])  # the underflowed tail is -0.0
    assert np.all(got[zero] == 0.0), v[zero][got[zero] != 0.0][:8]
    assert np.array_equal(np.signbit(got[zero]), np.signbit(want[zero]))
    under = got == 0.0  # ... and wherever the fp32 formula underflows before float64 does
    assert np.array_equal(np.signbit(got[under]), np.signbit(want[under]))


GELU_F32_FACTOR = 8


@pytest.mark.parametrize("approximate", ["none", "tanh"])
def test_f32_gelu_matches_fp64(ops, approximate):
    """The same values widened to fp32 plus 4,096 fp32 values uniform in [-12, 12]: |y - ref| <= 8 u |v|. The fp32
    formula itself (torch on the CPU) has max error 1.55 u |v| in both modes, which leaves 5x for the device's
    erff / tanhf; a swapped mode or a 1 % wrong constant is 100x outside. Measured on the MI355X:
    max err / (u |v|) = 1.551 (erf) and 1.644 (tanh), so the factor stays 8."""
    r = np.random.default_rng(_seed(31))
    v = np.concatenate([_all_bf16_values(), r.uniform(-12.0, 12.0, 4096).astype(np.float32)])
    y = ops.gelu(_gpu(v), approximate)
    assert y.dtype == torch.float32
    got = y.cpu().numpy().astype(np.float64)
    ref = _gelu_ref(v, approximate)
    err = np.abs(got - ref)
    av = np.abs(v.astype(np.float64))
    nz = av > 0
    print(f"f32 gelu {approximate}: max err / (u |v|) = {np.max(err[nz] / (U * av[nz])):.3f}")
    bad = np.flatnonzero(~(err <= GELU_F32_FACTOR * U * av))
    assert bad.size == 0, (bad.size, v[bad[:8]], got[bad[:8]], ref[bad[:8]])


# ================================================================ 4. lga_f32_add and the fp32 form of lga_embedding
@pytest.mark.parametrize("n", [1, 255, 256, 257, 768 * 9, 65535 * 256 + 513])
def test_f32_add_bit_exact(ops, n):
    """One rounding per element: bit-identical to the CPU's a + b. The last size is past the 65,535-block grid cap
    (the stride loop runs a second time for its 513 last elements)."""
    g = torch.Generator().manual_seed(_seed(41, n))
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g) * 3.0
    y = ops.add(a.to(DEV), b.to(DEV))
    assert y.dtype == torch.float32
    assert torch.equal(y.cpu().view(torch.int32), (a + b).view(torch.int32))


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("V,C", [(500, 128), (300, 768)])
def test_f32_embedding_bit_exact(ops, V, C, idx_dtype):
    """fp32 rows move as 2 C 16-bit words: every gathered row is a byte copy; ids 0, V - 1 and a repeat."""
    table = torch.from_numpy(_normal((V, C), 42, V, C))
    table[V - 1, C - 1] = float("nan")  # a byte copy keeps any bit pattern
    table[0, 0] = -0.0
    ids = torch.tensor([0, V - 1, 7, V // 2, 7, V - 1, 0, 1, V - 2], dtype=idx_dtype)
    y = ops.embedding(ids.to(DEV), table.to(DEV))
    assert y.dtype == torch.float32 and y.shape == (ids.numel(), C)
    assert torch.equal(y.cpu().view(torch.int32), table[ids.long()].view(torch.int32))


# ===================================================================================== 5. lga_f32_rope_kv_append
ROPE_T, ROPE_S = 7, 40
ROPE_CACHE_POS = [3, 4, 5, 6, 7, 8, 30]
SENTINEL = -777.25


@pytest.mark.parametrize("H,G,hs,n_elem", [(4, 4, 32, 8), (12, 12, 64, 16), (8, 2, 64, 64), (2, 1, 256, 64),
                                           (6, 3, 80, 20)])
def test_f32_rope_kv_append_bit_exact(ops, H, G, hs, n_elem):
    """x cos + rotate_half(x) sin with each op rounded once (mul_rn / add_rn) is what torch computes in fp32 on the
    CPU: q and the appended k rows are bit-identical to it on the first n_elem dims, byte copies above them, v is a
    byte copy, and every cache row that is not in cache_pos keeps its sentinel. rope_pos differs from cache_pos (the
    kernel takes both), q_per_kv > 1 in two cases, one head size (80) is no power of two."""
    qpk = H // G
    qkv = _normal((ROPE_T, (H + 2 * G) * hs), 51, H, G, hs)
    cache_pos = torch.tensor(ROPE_CACHE_POS, dtype=torch.int64)
    rope_pos = cache_pos + 5
    cos, sin = om.build_rope_cache(ROPE_S + 5, n_elem)
    assert cos.dtype == torch.float32 and cos.shape == (ROPE_S + 5, n_elem)
    kc = torch.full((G, ROPE_S, hs), SENTINEL, dtype=torch.float32, device=DEV)
    vc = torch.full((G, ROPE_S, hs), SENTINEL, dtype=torch.float32, device=DEV)
    q = ops.rope_kv_append(_gpu(qkv), kc, vc, cache_pos.to(DEV), rope_pos.to(DEV), cos.to(DEV), sin.to(DEV),
                           H, G, hs, n_elem)
    assert q.dtype == torch.float32 and q.shape == (ROPE_T, H, hs)

    x = torch.from_numpy(qkv).view(ROPE_T, G, qpk + 2, hs)
    c, s = cos[rope_pos][:, None, None, :], sin[rope_pos][:, None, None, :]  # (T, 1, 1, n_elem)

    def rope(t):  # (T, G, slots, hs) fp32, torch's own op-by-op rounding
        head = t[..., :n_elem]
        rot = torch.cat((-head[..., n_elem // 2:], head[..., :n_elem // 2]), dim=-1)
        return torch.cat((head * c + rot * s, t[..., n_elem:]), dim=-1)

    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    q_ref = rope(x[:, :, :qpk]).reshape(ROPE_T, H, hs)
    k_ref = rope(x[:, :, qpk:qpk + 1])[:, :, 0]  # (T, G, hs)
    v_ref = x[:, :, qpk + 1]
    assert torch.equal(bits(q.cpu()), bits(q_ref))
    assert torch.equal(bits(q.cpu()[..., n_elem:]), bits(x[:, :, :qpk].reshape(ROPE_T, H, hs)[..., n_elem:]))
    kc, vc = kc.cpu(), vc.cpu()
    assert torch.equal(bits(kc[:, cache_pos]), bits(k_ref.transpose(0, 1)))
    assert torch.equal(bits(kc[:, cache_pos][..., n_elem:]), bits(x[:, :, qpk].transpose(0, 1)[..., n_elem:]))
    assert torch.equal(bits(vc[:, cache_pos]), bits(v_ref.transpose(0, 1)))
    other = torch.ones(ROPE_S, dtype=torch.bool)
    other[cache_pos] = False
    assert bool((kc[:, other] == SENTINEL).all()) and bool((vc[:, other] == SENTINEL).all())


# ========================================================================================== 6. lga_f32_attention
F32_ATTENTION_MAX_SEQ = 32768  # the limit csrc/fp32.hip states (scores in LDS)
ATTN_GEOMS = [(4, 4, 32), (12, 12, 64), (8, 2, 64), (6, 1, 80), (4, 2, 128), (2, 1, 256)]
ATTN_SEQS = [(40, [0, 1, 2, 3, 4, 39]), (300, [255, 256, 257, 299]), (2304, [1000, 2303])]
ATTN_CASES = [(H, G, hs, S, pos) for (H, G, hs) in ATTN_GEOMS for (S, pos) in ATTN_SEQS]
ATTN_CASES.append((2, 1, 64, F32_ATTENTION_MAX_SEQ, [0, 16384, 32767]))
_ATTN_IDS = [f"H{H}-G{G}-hs{hs}-S{S}" for (H, G, hs, S, _) in ATTN_CASES]


def _attn_inputs(H, G, hs, S, positions, dominant):
    T = len(positions)
    q = _normal((T, H, hs), 61, H, G, hs, S)
    k = _normal((G, S, hs), 62, H, G, hs, S)
    v = _normal((G, S, hs), 63, H, G, hs, S)
    if dominant:
        # key p of each query points along that query: score 6 |q| ~ 6 sqrt(hs) against O(1) for the others, so
        # its softmax weight is 1 - O(e^-20). The heads of a group share the key, so they share the direction
        # (with different lengths).
        qpk = H // G
        for g in range(G):
            for j in range(1, qpk):
                q[:, g * qpk + j] = q[:, g * qpk] * np.float32(1.0 + 0.125 * j)
            for t, p in enumerate(positions):
                d = q[t, g * qpk].astype(np.float64)
                k[g, p] = (6.0 * d / np.linalg.norm(d) * math.sqrt(hs)).astype(np.float32)
    return q, k, v


def _attn_ref_and_bound(q, k, v, positions, scale):
    """fp64 softmax(q K^T scale) V over keys 0..p of the head's group, and per (t, h) the bound
    2^-21 (1 + max_j |s_j|) max|v| over the attended rows: 8 u for the fp32 exp, sums and the division, times
    (1 + max|s|) because an error of u |s| in a score (the fp32 dot product and the scaling) moves its weight by
    that much relatively, times the magnitude of what is averaged."""
    T, H, hs = q.shape
    G = k.shape[0]
    ref = np.zeros((T, H, hs))
    bound = np.zeros((T, H, 1))
    k64, v64 = k.astype(np.float64), v.astype(np.float64)
    for t, p in enumerate(positions):
        for h in range(H):
            g = h // (H // G)
            s = (k64[g, :p + 1] @ q[t, h].astype(np.float64)) * scale
            w = np.exp(s - s.max())
            ref[t, h] = (w / w.sum()) @ v64[g, :p + 1]
            bound[t, h] = 2.0 ** -21 * (1.0 + np.abs(s).max()) * np.abs(v64[g, :p + 1]).max()
    return ref, bound


def _attn_launch(ops, q, k, v, positions, last_row):
    """One launch over the query rows ``positions`` with every cache row after ``last_row`` set to NaN."""
    kd, vd = _gpu(k), _gpu(v)
    kd[:, last_row + 1:] = float("nan")
    vd[:, last_row + 1:] = float("nan")
    H, hs = q.shape[1], q.shape[2]
    y = ops.attention(_gpu(q), kd, vd, torch.tensor(positions, dtype=torch.int64, device=DEV), H, k.shape[0], hs,
                      1.0 / math.sqrt(hs))
    assert y.dtype == torch.float32 and y.shape == (len(positions), H * hs)
    return y.cpu().numpy().astype(np.float64).reshape(len(positions), H, hs)


@pytest.mark.parametrize("dominant", [False, True], ids=["random", "dominant-last-key"])
@pytest.mark.parametrize("H,G,hs,S,positions", ATTN_CASES, ids=_ATTN_IDS)
def test_f32_attention_matches_fp64(ops, H, G, hs, S, positions, dominant):
    """MHA, GQA and MQA (g = h / (H / G)), head sizes 32 .. 256 (HSP / phases of the P.V step; 80 leaves idle
    threads), L = 1 .. 5 (waves with no key), L across the 256-thread softmax stride, thousands of keys, and the
    largest max_seq the library states (132,096 B of dynamic LDS). The T positions are the rows of one launch, over
    a cache whose rows after the last position are NaN; then every earlier position runs once more on its own with
    NaN after ITS position, so that a read past input_pos cannot pass. In the dominant-last-key variant key p
    carries a softmax weight of 1 - O(e^-20): y must equal v[p] within the same bound, and an off-by-one in L fails
    outright instead of by 1 / L. Measured on the MI355X: error at most 0.11 of the bound (random; 0.005 in the
    32,768-row case, whose launch succeeds) and below 1e-4 of it (dominant last key)."""
    q, k, v = _attn_inputs(H, G, hs, S, positions, dominant)
    ref, bound = _attn_ref_and_bound(q, k, v, positions, 1.0 / math.sqrt(hs))
    got = _attn_launch(ops, q, k, v, positions, max(positions))
    worst = float(np.max(np.abs(got - ref) / bound))
    assert np.all(np.abs(got - ref) <= bound), worst
    for t, p in enumerate(positions):
        if p == max(positions):
            continue
        alone = _attn_launch(ops, q[t:t + 1], k, v, [p], p)
        r = float(np.max(np.abs(alone - ref[t:t + 1]) / bound[t:t + 1]))
        worst = max(worst, r)
        assert np.all(np.abs(alone - ref[t:t + 1]) <= bound[t:t + 1]), (p, r)
    print(f"f32 attention H{H} G{G} hs{hs} S{S} dominant={dominant}: max err / bound = {worst:.4f}")
    if dominant:
        qpk = H // G
        for t, p in enumerate(positions):
            vp = np.repeat(v[:, p].astype(np.float64), qpk, axis=0)  # (H, hs): head h reads group h / qpk
            assert np.all(np.abs(ref[t] - vp) <= 0.1 * bound[t]), "the construction: the reference itself is v[p]"
            assert np.all(np.abs(got[t] - vp) <= bound[t]), (p, float(np.max(np.abs(got[t] - vp) / bound[t])))


def test_f32_attention_refuses_max_seq_above_the_limit(ops):
    """One row more than the stated limit must raise before any launch and leave y alone."""
    H, G, hs, S = 2, 1, 64, F32_ATTENTION_MAX_SEQ + 1
    kc = torch.zeros(G, S, hs, dtype=torch.float32, device=DEV)
    q = torch.zeros(1, H, hs, dtype=torch.float32, device=DEV)
    y = torch.full((1, H * hs), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match=rf"max_seq must be in \[1, {F32_ATTENTION_MAX_SEQ}\]"):
        ops.attention(q, kc, kc, torch.zeros(1, dtype=torch.int64, device=DEV), H, G, hs, 0.125, out=y)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ============================================================================================= 7. lga_argmax_f32
ARGMAX_N = [1, 7, 1001, 50304, 65549, 150001]


def _argmax(ops, a: np.ndarray, off: int) -> int:
    return int(ops.argmax(_offset_view(a, off) if off else _gpu(a)).item())


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", ARGMAX_N)
def test_argmax_f32_matches_torch(ops, n, off):
    """One workgroup of 1,024 threads over n fp32 logits, from a 16-B aligned pointer and from one aligned to 4
    bytes only; against torch.argmax on the CPU."""
    r = np.random.default_rng(_seed(71, n))
    # quarter-integers in [-8, 8]: many exact ties at the maximum, the lowest index must win
    ties = (r.integers(-32, 33, n) / 4.0).astype(np.float32)
    want = int(torch.argmax(torch.from_numpy(ties)))
    assert n < 1000 or int(np.sum(ties == ties.max())) > 1
    assert _argmax(ops, ties, off) == want == int(np.flatnonzero(ties == ties.max())[0])

    if n >= 2:  # 1.0 early and 1.0 + 2^-23 later: equal in bf16, so any bf16 rounding on the way answers i
        pair = r.uniform(-4.0, 0.5, n).astype(np.float32)
        i, j = n // 3, n - 1 - n // 5
        assert i < j
        pair[i], pair[j] = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
        assert int(torch.argmax(torch.from_numpy(pair))) == j
        assert _argmax(ops, pair, off) == j

    nan = r.standard_normal(n).astype(np.float32)  # the first NaN wins, as in the bf16 kernel's test
    nan[n // 2] = nan[n - 1] = np.float32("nan")
    assert int(torch.argmax(torch.from_numpy(nan))) == n // 2
    assert _argmax(ops, nan, off) == n // 2

    assert _argmax(ops, np.full(n, -np.inf, dtype=np.float32), off) == 0  # nothing beats the start value: index 0


@pytest.mark.parametrize("n", [7, 65549])
def test_argmax_f32_bookkeeping(ops, n):
    """token_out receives the token and pos_inout advances by one (the decode graph's per-step state)."""
    a = np.random.default_rng(_seed(72, n)).standard_normal(n).astype(np.float32)
    idx = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    tok = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    pos = torch.tensor([41], dtype=torch.int64, device=DEV)
    out = ops.argmax(_gpu(a), out_idx=idx, token_out=tok, pos_inout=pos)
    want = int(np.argmax(a))
    assert out is idx and int(idx.item()) == want and int(tok.item()) == want and int(pos.item()) == 42
