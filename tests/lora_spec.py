"""Specification of the LoRA path — TEST INFRASTRUCTURE ONLY (as oracle/, tests/int8_spec.py).

Three restatements, none of which runs the code under test (``lora_config`` alone imports its Config dataclass):

* ``chain`` — the arithmetic of include/litgpt_amd.h's LoRA section over the DEVICE layout (A (R, K), B (N, r) in
  output-row order, row_off), with a rounding function at every point where the kernels round to bf16:
      t = rnd(x' A^T);  u_n = rnd(sum_j B[n,j] t[off_n + j]) (0 where off_n < 0);  l = rnd(u * scaling);
      y = rnd(base + l) (or l);  y = rnd(y + residual)
* ``scatter`` — reference-layout adapter tensors (lit_gpt/lora.py of the reference: ``lora_A`` (r * enabled, K),
  ``lora_B`` (rows of the enabled q / k / v, r), ``lora_ind``) -> the device layout, with optional rank padding;
* ``LoraOracle`` — ``oracle.model.OracleGPT`` whose ``_lin`` adds the reference's unmerged LoRA forward
  (LoRALinear.forward / LoRAQKVLinear.forward: after_A, per-segment after_B, zero_pad, * scaling, + pretrained) in the
  oracle's dtype (bf16: torch rounds after every op, the reference's bf16-true rounding points).

``MODELS`` are the two fixture models of tests/golden/make_golden_lora.py (which imports them from here).
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from oracle.model import OracleGPT

MODELS = {
    # (a) the reference's generate/lora.py defaults: rank 8 on query + value
    "mha": dict(base=dict(name="Llama-2-7b-hf", n_layer=2, n_embd=256, n_head=4, intermediate_size=640,
                          vocab_size=1000, padding_multiple=64, block_size=256),
                lora=dict(r=8, alpha=16, to_query=True, to_value=True)),
    # (b) grouped queries, every target but the key, rank 4 (padded to 8 on the device)
    "gqa": dict(base=dict(name="Llama-2-70b-hf", n_layer=2, n_embd=256, n_head=4, n_query_groups=2,
                          intermediate_size=512, vocab_size=1000, padding_multiple=64, block_size=256),
                lora=dict(r=4, alpha=16, to_query=True, to_value=True, to_projection=True, to_mlp=True, to_head=True)),
}
SEED = 21  # oracle.synth seed of the base weights, the adapter's lora_B and the prompt
B_STD = 0.05
PROMPT = 12


def bf16_round(v: torch.Tensor) -> torch.Tensor:
    return v.to(torch.bfloat16).to(v.dtype)


def qkv_segments(out_features: int, n_head: int, n_query_groups: int, enable: Sequence[bool]) -> List[torch.Tensor]:
    """Output rows of the enabled q / k / v slots, in that order (concatenated: the reference's lora_ind). Row x of the
    fused qkv Linear belongs to head (x // head_size) % (q_per_kv + 2) of its group: the last two are key and value."""
    total = n_head // n_query_groups + 2
    hs = out_features // (n_query_groups * total)
    head = (np.arange(out_features) // hs) % total
    masks = (head < total - 2, head == total - 2, head == total - 1)
    return [torch.from_numpy(np.nonzero(m)[0]) for m, e in zip(masks, enable) if e]


def scatter(lora_A: torch.Tensor, lora_B: torch.Tensor, r: int, out_features: int,
            segments: Optional[List[torch.Tensor]] = None, pad_to: int = 1):
    """Reference layout -> (A, B, row_off or None) of the device layout, r padded up to a multiple of ``pad_to``."""
    rp = -(-r // pad_to) * pad_to
    K = lora_A.shape[1]
    n_seg = 1 if segments is None else len(segments)
    A = torch.zeros(rp * n_seg, K, dtype=lora_A.dtype)
    B = torch.zeros(out_features, rp, dtype=lora_B.dtype)
    for s in range(n_seg):
        A[s * rp:s * rp + r] = lora_A[s * r:(s + 1) * r]
    if segments is None:
        B[:, :r] = lora_B
        return A, B, None
    row_off = torch.full((out_features,), -1, dtype=torch.int32)
    first = 0
    for s, rows in enumerate(segments):
        B[rows, :r] = lora_B[first:first + rows.numel()]
        row_off[rows] = s * rp
        first += rows.numel()
    return A, B, row_off


def chain(x, A, B, row_off, scaling, base=None, residual=None, rnd=lambda v: v, parts: Optional[dict] = None):
    """y (M, N) of the module docstring for x' (M, K), every tensor in one float dtype; ``rnd`` rounds where the kernels
    round to bf16 (identity: exact arithmetic in that dtype). ``parts`` receives t, l and sum_j |B_nj| |t_j|."""
    r = B.shape[1]
    t = rnd(x @ A.T)
    off = torch.zeros(B.shape[0], dtype=torch.int64) if row_off is None else row_off.long()
    u = torch.zeros(x.shape[0], B.shape[0], dtype=x.dtype)
    mag = torch.zeros_like(u)
    for o in torch.unique(off[off >= 0]).tolist():
        rows = torch.nonzero(off == o).flatten()
        u[:, rows] = t[:, o:o + r] @ B[rows].T
        mag[:, rows] = t[:, o:o + r].abs() @ B[rows].abs().T
    l = rnd(rnd(u) * scaling)
    y = l if base is None else torch.where((off >= 0)[None, :], rnd(base + l), base)
    if parts is not None:
        parts.update(t=t, l=l, mag=mag, pre_residual=y)
    if residual is not None:
        y = rnd(y + residual)
    return y


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, rnd=lambda v: v) -> torch.Tensor:
    """lit_gpt/rmsnorm.py of the reference: w * (x * rsqrt(mean x^2 + eps)), one rounding."""
    return rnd(w * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)))


class LoraOracle(OracleGPT):
    """OracleGPT over a state dict that also carries the adapter under the reference's names; ``lcfg`` is a config
    with the reference's LoRA fields (r, alpha, to_query, to_key, to_value)."""

    def __init__(self, lcfg, sd: Dict[str, np.ndarray], **kw):
        super().__init__(lcfg, sd, **kw)
        self.lcfg = lcfg

    def _base_lin(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        """The pretrained Linear (a test of a quantized base whose Linear is more than a dequantized weight — LLM.int8
        quantizes the activations too — overrides this)."""
        return OracleGPT._lin(self, prefix, x)

    def _lin(self, prefix: str, x: torch.Tensor) -> torch.Tensor:
        pretrained = self._base_lin(prefix, x)
        A = self.p.get(f"{prefix}.lora_A")
        if A is None:
            return pretrained
        B, c = self.p[f"{prefix}.lora_B"], self.lcfg
        after_A = x @ A.T
        if prefix.endswith("attn.attn"):
            segments = qkv_segments(pretrained.shape[-1], c.n_head, c.n_query_groups,
                                    (c.to_query, c.to_key, c.to_value))
            lora = torch.zeros_like(pretrained)  # zero_pad
            first = 0
            for s, rows in enumerate(segments):  # the grouped conv1d: segment s of after_A against its rows of B
                lora[:, rows] = after_A[:, s * c.r:(s + 1) * c.r] @ B[first:first + rows.numel()].T
                first += rows.numel()
        else:
            lora = after_A @ B.T
        return pretrained + lora * (c.alpha / c.r)


def merged_state(lcfg, sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The state dict of the merged model: W + zero_pad((B A per segment) * scaling), adapter keys dropped (fp32)."""
    out = {k: v for k, v in sd.items() if "lora_" not in k}
    for k in sd:
        if not k.endswith(".lora_A"):
            continue
        prefix = k[:-len(".lora_A")]
        A, B = torch.from_numpy(sd[k]).float(), torch.from_numpy(sd[f"{prefix}.lora_B"]).float()
        W = torch.from_numpy(out[f"{prefix}.weight"]).float().clone()
        segments = None
        if prefix.endswith("attn.attn"):
            segments = qkv_segments(W.shape[0], lcfg.n_head, lcfg.n_query_groups,
                                    (lcfg.to_query, lcfg.to_key, lcfg.to_value))
        Ad, Bd, off = scatter(A, B, lcfg.r, W.shape[0], segments)
        offs = torch.zeros(W.shape[0], dtype=torch.int64) if off is None else off.long()
        for o in torch.unique(offs[offs >= 0]).tolist():
            rows = torch.nonzero(offs == o).flatten()
            W[rows] += (Bd[rows] @ Ad[o:o + lcfg.r]) * (lcfg.alpha / lcfg.r)
        out[f"{prefix}.weight"] = W.numpy()
    return out


def fixture_state(key: str, golden) -> Dict[str, np.ndarray]:
    """Base weights (oracle.synth, the fixture's seed) + the fixture's adapter tensors, reference names, fp32."""
    from oracle import synth

    sd = synth.state_dict(lora_config(key), seed=int(golden["seed"]))
    for name in golden.files:
        if name.startswith(f"{key}/") and "lora_" in name and not name.endswith("lora_ind"):
            sd[name[len(key) + 1:]] = golden[name]
    return sd


def lora_config(key: str):
    from lit_gpt.lora import Config

    kw = dict(MODELS[key]["base"])
    return Config.from_name(kw.pop("name"), **kw, **MODELS[key]["lora"])
