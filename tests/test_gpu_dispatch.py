"""Which launches a forward takes, per weight format: the ordered entry points of one block plus the head, and for
the Linear launches whether the RMSNorm weight and the residual ride in them.

The kernels' results are checked elsewhere (test_gpu_model / test_gpu_int8 / test_gpu_kernels); nothing else pins
the format -> kernel decision of lit_gpt/quantize.py for bf16 and int8, or the norm placement of the 4-bit GEMVs
(single launch: fused while K / 32 <= 256; dual SwiGLU launch: while K / 32 <= 128). A proxy in place of the loaded
library records every ``lga_*`` call; the expected lists are written out literally.
"""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# the geometry "mha" of tests/test_gpu_model.py, and one block wide enough (K / 32 = 144) that the dual 4-bit GEMV
# no longer takes the norm while the single one still does (36 heads in 9 query groups: lga_attention_decode_fused
# takes 1, 2, 4 or 8 query heads per group, so a single group of 36 cannot run)
MHA = dict(n_layer=2, n_embd=512, n_head=4, intermediate_size=640, vocab_size=1000, padding_multiple=64,
           block_size=256)
WIDE = dict(n_layer=1, n_embd=4608, n_head=36, n_query_groups=9, intermediate_size=256, vocab_size=512,
            padding_multiple=64, block_size=256)

# entry points that launch nothing (shape queries)
QUERIES = {"lga_q4f_fits", "lga_q4f_workspace_bytes", "lga_attention_workspace_bytes"}
# Linear launches: the positions of their (norm_weight, residual) pointer arguments
NORM_RES = {
    "lga_q4_gemv": (5, 4), "lga_q4_gemv_swiglu": (5, None), "lga_q4_gemm": (None, 4), "lga_q4_gemm_fused": (None, 4),
    "lga_bf16_gemv": (4, 3), "lga_bf16_gemv_swiglu": (3, None), "lga_bf16_gemm": (None, 3),
    "lga_int8_gemv": (5, 4), "lga_int8_gemv_swiglu": (5, None), "lga_int8_gemm": (None, 8),
}
_INTS = (ctypes.c_int, ctypes.c_long, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_size_t)


class Recorder:
    """Stands in for ``ops._lib``: forwards every call and logs (symbol, arguments) for the ``lga_*`` entry points —
    an integer or float argument by value, a pointer argument as whether it is non-null."""

    def __init__(self, ops):
        self.lib, self.signatures, self.calls = ops.load_library(), ops.SIGNATURES, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        types = self.signatures.get(name)
        if types is None:
            return fn

        def call(*args):
            self.calls.append((name, [int(a) if t in _INTS else float(a) if t is ctypes.c_float else bool(a)
                                      for t, a in zip(types, args)]))
            return fn(*args)

        return call

    def launches(self):
        """The launches since the last call of this method as "symbol[+norm][+res]", in order."""
        out = []
        for name, args in self.calls:
            if name not in QUERIES:
                ni, ri = NORM_RES.get(name, (None, None))
                out.append(name + ("+norm" if ni is not None and args[ni] else "")
                           + ("+res" if ri is not None and args[ri] else ""))
        self.calls.clear()
        return out


@pytest.fixture
def rec(monkeypatch):
    from lit_gpt import ops

    r = Recorder(ops)
    monkeypatch.setattr(ops, "_lib", r)
    return r


def build(geometry, mode):
    from lit_gpt import GPT, Config
    from lit_gpt.quantize import QuantizedPrecision

    torch.manual_seed(0)
    model = GPT(Config.from_name("Llama-2-7b-hf", **geometry)).to(device=DEV, dtype=torch.bfloat16)
    if mode != "bf16":
        QuantizedPrecision(mode).convert_module(model, DEV)
    model.max_seq_length = 16
    model.set_kv_cache(1, device=DEV)
    return model.eval()


@torch.inference_mode()
def forward(model, T, pos):
    """T tokens at positions pos .. pos + T - 1 (with ``input_pos``) -> logits."""
    idx = torch.randint(0, model.config.vocab_size, (1, T), generator=torch.Generator().manual_seed(T + pos))
    return model(idx.to(DEV), torch.arange(pos, pos + T, device=DEV))


# ------------------------------------------------------------------------- expected launches (of the parent commit)
EMBED = ["lga_embedding"]
# mode -> (block, head) of an 8-token prefill; the block is [qkv, rope + KV append, attention, proj, mlp ..., proj]
_Q4F_PREFILL = (["lga_rmsnorm", "lga_q4_gemm_fused", "lga_rope_kv_append", "lga_attention", "lga_q4_gemm_fused+res",
                 "lga_rmsnorm", "lga_q4_gemm_swiglu", "lga_q4_gemm_fused+res"],
                ["lga_rmsnorm", "lga_q4_gemm_fused"])
PREFILL = {
    "int4-g128": _Q4F_PREFILL,
    "nf4": _Q4F_PREFILL,
    # group 32 is outside the fused-dequant GEMM: lga_q4_gemm, and fc_1 / fc_2 / lga_swiglu as three launches
    "int4-g32": (["lga_rmsnorm", "lga_q4_gemm", "lga_rope_kv_append", "lga_attention", "lga_q4_gemm+res",
                  "lga_rmsnorm", "lga_q4_gemm", "lga_q4_gemm", "lga_swiglu", "lga_q4_gemm+res"],
                 ["lga_rmsnorm", "lga_q4_gemm"]),
    "bf16": _Q4F_PREFILL,  # the same fused MFMA GEMMs with fmt 2 (the bf16 weight as stored)
    # one activation quantization per Linear call (fc_1 and fc_2 each), no fused SwiGLU GEMM
    "bnb.int8": (["lga_rmsnorm", "lga_int8_quantize_act", "lga_int8_gemm", "lga_rope_kv_append", "lga_attention",
                  "lga_int8_quantize_act", "lga_int8_gemm+res", "lga_rmsnorm", "lga_int8_quantize_act",
                  "lga_int8_gemm", "lga_int8_quantize_act", "lga_int8_gemm", "lga_swiglu", "lga_int8_quantize_act",
                  "lga_int8_gemm+res"],
                 ["lga_rmsnorm", "lga_int8_quantize_act", "lga_int8_gemm"]),
}
# mode -> (block, head) of one decode token: both norms ride the GEMV prologues, both residuals the epilogues
_Q4_DECODE = (["lga_q4_gemv+norm", "lga_attention_decode_fused", "lga_q4_gemv+res", "lga_q4_gemv_swiglu+norm",
               "lga_q4_gemv+res"],
              ["lga_q4_gemv+norm"])
DECODE = {
    "int4-g128": _Q4_DECODE,
    "nf4": _Q4_DECODE,
    "int4-g32": _Q4_DECODE,
    "bf16": (["lga_bf16_gemv+norm", "lga_attention_decode_fused", "lga_bf16_gemv+res", "lga_bf16_gemv_swiglu+norm",
              "lga_bf16_gemv+res"],
             ["lga_bf16_gemv+norm"]),
    "bnb.int8": (["lga_int8_gemv+norm", "lga_attention_decode_fused", "lga_int8_gemv+res",
                  "lga_int8_gemv_swiglu+norm", "lga_int8_gemv+res"],
                 ["lga_int8_gemv+norm"]),
}


@pytest.mark.parametrize("mode", ["int4-g128", "nf4", "int4-g32", "bf16", "bnb.int8"])
def test_block_and_head_launches(rec, mode):
    model = build(MHA, mode)
    rec.launches()
    forward(model, 8, 0)
    got = rec.launches()
    assert got == EMBED + PREFILL[mode][0] * 2 + PREFILL[mode][1]
    forward(model, 1, 8)
    got = rec.launches()
    assert got == EMBED + DECODE[mode][0] * 2 + DECODE[mode][1]


# mode -> the decode launches of the one wide block + head: the 4-bit dual GEMV leaves norm_2 to lga_rmsnorm
WIDE_DECODE = {
    "int4-g128": ["lga_q4_gemv+norm", "lga_attention_decode_fused", "lga_q4_gemv+res", "lga_rmsnorm",
                  "lga_q4_gemv_swiglu", "lga_q4_gemv+res", "lga_q4_gemv+norm"],
    "bf16": ["lga_bf16_gemv+norm", "lga_attention_decode_fused", "lga_bf16_gemv+res", "lga_bf16_gemv_swiglu+norm",
             "lga_bf16_gemv+res", "lga_bf16_gemv+norm"],
    "bnb.int8": ["lga_int8_gemv+norm", "lga_attention_decode_fused", "lga_int8_gemv+res",
                 "lga_int8_gemv_swiglu+norm", "lga_int8_gemv+res", "lga_int8_gemv+norm"],
}


@pytest.mark.parametrize("mode", ["int4-g128", "bf16", "bnb.int8"])
def test_norm_placement_of_the_dual_gemv_at_wide_rows(rec, mode):
    model = build(WIDE, mode)
    rec.launches()
    forward(model, 1, 0)
    got = rec.launches()
    assert got == EMBED + WIDE_DECODE[mode]


@torch.inference_mode()
def test_single_4bit_gemv_leaves_the_norm_of_a_long_row_to_rmsnorm(rec):
    """K / 32 = 260 > 256: a separate lga_rmsnorm, then the GEMV with a null norm."""
    from lit_gpt.quantize import QuantLinear

    N, K = 16, 8320
    lin = QuantLinear.from_float(torch.randn(N, K, device=DEV) * 0.02, None, "int4-g128", DEV)
    x = torch.randn(1, K, device=DEV).bfloat16()
    rec.launches()
    y = lin(x, norm_weight=torch.ones(K, dtype=torch.bfloat16, device=DEV), norm_eps=1e-5)
    assert y.shape == (1, N)
    assert rec.launches() == ["lga_rmsnorm", "lga_q4_gemv"]


@torch.inference_mode()
def test_mlp_of_two_formats_runs_the_two_linears_and_swiglu(rec):
    """fc_1 a bf16 nn.Linear, fc_2 4-bit: no dual launch, at one row or at several."""
    from lit_gpt import Config
    from lit_gpt.model import LLaMAMLP
    from lit_gpt.quantize import QuantLinear

    torch.manual_seed(0)
    mlp = LLaMAMLP(Config.from_name("Llama-2-7b-hf", **MHA)).to(device=DEV, dtype=torch.bfloat16)
    mlp.fc_2 = QuantLinear.from_float(mlp.fc_2.weight, None, "int4-g128", DEV)
    rec.launches()
    assert mlp(torch.randn(1, 1, 512, device=DEV).bfloat16()).shape == (1, 1, 512)
    assert rec.launches() == ["lga_bf16_gemv", "lga_q4_gemv", "lga_swiglu", "lga_bf16_gemv"]
    assert mlp(torch.randn(1, 8, 512, device=DEV).bfloat16()).shape == (1, 8, 512)
    assert rec.launches() == ["lga_q4_gemm_fused", "lga_q4_gemm_fused", "lga_swiglu", "lga_q4_gemm_fused"]


@torch.inference_mode()
def test_fp32_linear_refuses_a_fused_norm(rec):
    from lit_gpt.model import _lin

    lin = torch.nn.Linear(64, 32, bias=False).to(DEV)
    for M in (1, 8):
        x = torch.randn(M, 64, device=DEV)
        assert _lin(lin, x).shape == (M, 32) and rec.launches() == ["lga_f32_linear"]
        with pytest.raises(NotImplementedError, match="fp32 path"):
            _lin(lin, x, norm_weight=torch.ones(64, device=DEV))
        assert rec.launches() == []
