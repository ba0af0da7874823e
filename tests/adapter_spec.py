"""Specification of the LLaMA-Adapter (v1) path — TEST INFRASTRUCTURE ONLY (as oracle/, tests/lora_spec.py).

Two restatements, neither of which runs the code under test (``adapter_config`` alone imports its Config dataclass):

* ``AdapterOracle`` — ``oracle.model.OracleGPT`` whose ``_attn`` adds, in every block ``i >= adapter_start_layer``, the
  reference's gated attention over the adaption prompt (lit_gpt/adapter.py CausalSelfAttention
  .scaled_dot_product_attention) in the oracle's dtype: fp32 / float64 is exact arithmetic, bf16 rounds after every
  torch op, the reference's bf16-true rounding points;
* ``prefix_attention_spec`` — the arithmetic of ``lga_adapter_attention`` (include/litgpt_amd.h) in float64 with a bf16
  rounding at exactly the points the header names:
      q^ = bf16(rope(q));  s_j = scale * q^ . ak_j;  p = softmax(s);  ay = bf16(sum_j p_j av_j);
      t = bf16(g_h * ay);  y = bf16(y + t)

``MODELS`` are the two fixture models of tests/golden/make_golden_adapter.py (which imports them from here).
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.model import OracleGPT, apply_rope

_BASE = dict(name="Llama-2-7b-hf", n_layer=3, n_embd=256, intermediate_size=512, vocab_size=1000, padding_multiple=64,
             block_size=64)
MODELS = {
    "mha": dict(base=dict(_BASE, n_head=4, n_query_groups=4), adapter=dict(adapter_start_layer=1)),
    "gqa": dict(base=dict(_BASE, n_head=4, n_query_groups=2), adapter=dict(adapter_start_layer=1)),
}
SEED = 21  # oracle.synth seed of the base weights and the prompt; torch seed of the adapter tensors
GATING_STD = 0.5
PROMPT = 12
MIN_MOVED = 3  # positions (of PROMPT) at which the adapter must move the reference's argmax, per model


def bf16_round(v: torch.Tensor) -> torch.Tensor:
    return v.to(torch.bfloat16).to(v.dtype)


def adapter_config(key: str, **overrides):
    from lit_gpt.adapter import Config

    kw = dict(MODELS[key]["base"], **overrides)
    return Config.from_name(kw.pop("name"), **kw, **MODELS[key]["adapter"])


def wide_config(key: str, **overrides):
    """The fixture model widened to head_size 128 (n_embd 512, 4 heads): the fused decode attention's geometry, which
    the batched, shared-prefix and window routes need."""
    return adapter_config(key, n_embd=512, **overrides)


def random_adapter(cfg, seed: int = SEED, gating_std: float = GATING_STD) -> Dict[str, np.ndarray]:
    """A seeded random adapter under the reference's names (fp32 numpy): standard-normal prefix rows, gating factors of
    both signs. For tests that compare the product with itself or with ``AdapterOracle``; no fixture needed."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i in range(cfg.adapter_start_layer, cfg.n_layer):
        pre = f"transformer.h.{i}.attn"
        out[f"{pre}.adapter_wte.weight"] = torch.randn(cfg.adapter_prompt_length, cfg.n_embd, generator=g).numpy()
        out[f"{pre}.gating_factor"] = (torch.randn(1, 1, cfg.n_head, 1, generator=g) * gating_std).numpy()
    return out


def is_adapter_key(k: str) -> bool:
    return "adapter_wte" in k or "gating_factor" in k


def fixture_state(key: str, golden) -> Dict[str, np.ndarray]:
    """Base weights (oracle.synth, the fixture's seed) + the fixture's adapter tensors, reference names, fp32."""
    from oracle import synth

    sd = synth.state_dict(adapter_config(key), seed=int(golden["seed"]))
    for name in golden.files:
        if name.startswith(f"{key}/") and is_adapter_key(name):
            sd[name[len(key) + 1:]] = golden[name]
    return sd


class AdapterOracle(OracleGPT):
    """OracleGPT over a state dict that also carries ``adapter_wte.weight`` / ``gating_factor`` ((1, 1, n_head, 1))
    under the reference's names; ``cfg`` has ``adapter_prompt_length`` and ``adapter_start_layer``."""

    def _attn(self, i: int, x: torch.Tensor, cos, sin, input_pos: Optional[torch.Tensor]) -> torch.Tensor:
        c = self.cfg
        T = x.size(0)
        G, hs, H = c.n_query_groups, c.head_size, c.n_head
        qpk = H // G
        pre = f"transformer.h.{i}.attn"
        qkv = self._lin(f"{pre}.attn", x).view(T, G, qpk + 2, hs)
        q = qkv[:, :, :qpk].reshape(T, H, hs).transpose(0, 1)  # (H, T, hs)
        k = qkv[:, :, qpk].transpose(0, 1)  # (G, T, hs)
        v = qkv[:, :, qpk + 1].transpose(0, 1)
        n = c.rope_n_elem
        q = torch.cat((apply_rope(q[..., :n], cos, sin), q[..., n:]), dim=-1)
        k = torch.cat((apply_rope(k[..., :n], cos, sin), k[..., n:]), dim=-1)
        scale = 1.0 / math.sqrt(hs)
        if input_pos is not None:
            if self.cache is None:
                raise TypeError("You need to call `gpt.set_kv_cache()`")
            self.cache.write(i, input_pos, k, v)
            kk, vv = self.cache.k[i], self.cache.v[i]
            mask = torch.arange(kk.size(1))[None, :] <= input_pos[:, None]
            y = F.scaled_dot_product_attention(q[None], kk[None], vv[None], attn_mask=mask[None, None], scale=scale,
                                               enable_gqa=G != H)
        else:
            y = F.scaled_dot_product_attention(q[None], k[None], v[None], is_causal=True, scale=scale,
                                               enable_gqa=G != H)
        if i >= c.adapter_start_layer:
            # the prefix goes through the layer's own qkv Linear; its k / v slices are never roped, every one of the
            # aT keys is visible to every query; one gating factor per head
            aT = c.adapter_prompt_length
            aqkv = self._lin(f"{pre}.attn", self.p[f"{pre}.adapter_wte.weight"]).view(aT, G, qpk + 2, hs)
            ak = aqkv[:, :, qpk].transpose(0, 1)  # (G, aT, hs)
            av = aqkv[:, :, qpk + 1].transpose(0, 1)
            ay = F.scaled_dot_product_attention(q[None], ak[None], av[None], scale=scale, enable_gqa=G != H)
            y = y + self.p[f"{pre}.gating_factor"].reshape(1, H, 1, 1) * ay
        y = y[0].transpose(0, 1).reshape(T, H * hs)
        return self._lin(f"{pre}.proj", y)


def prefix_attention_spec(y, qkv, ak, av, gating, cos, sin, pos, H, G, hs, n_elem, scale, active=None,
                          parts: Optional[dict] = None) -> torch.Tensor:
    """``lga_adapter_attention`` in float64. y (T, H * hs), qkv (T, (H + 2G) * hs), ak / av (G, aT, hs), gating (H,):
    tensors holding bf16 values; cos / sin the fp32 tables; pos (T,) the rows' positions; active (T,) or None. The rope
    products are exact in float64 where the kernel's fp32 products round: the two differ before the bf16 rounding by
    fp32 steps only. ``parts`` receives ay and t (float64, (T, H, hs)). Returns y as float64 holding bf16 values."""
    T = qkv.shape[0]
    qpk = H // G
    x = qkv.double().view(T, G, qpk + 2, hs)[:, :, :qpk].reshape(T, H, hs)
    c, s = cos.double()[pos.long()], sin.double()[pos.long()]  # (T, n_elem)
    xr = x[..., :n_elem]
    half = n_elem // 2
    rot = torch.cat((-xr[..., half:], xr[..., :half]), dim=-1)
    q = torch.cat((bf16_round(xr * c[:, None] + rot * s[:, None]), x[..., n_elem:]), dim=-1)  # (T, H, hs)
    g_of = torch.arange(H) // qpk
    k, v = ak.double()[g_of], av.double()[g_of]  # (H, aT, hs)
    sc = scale * torch.einsum("thd,hjd->thj", q, k)
    p = torch.softmax(sc, dim=-1)
    ay = bf16_round(torch.einsum("thj,hjd->thd", p, v))
    t = bf16_round(gating.double().view(1, H, 1) * ay)
    y0 = y.double().view(T, H, hs)
    out = bf16_round(y0 + t)
    if active is not None:
        out = torch.where(active.view(T, 1, 1) != 0, out, y0)
    if parts is not None:
        parts.update(ay=ay, t=t)
    return out.view(T, H * hs)
