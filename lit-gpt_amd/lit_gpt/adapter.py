"""LLaMA-Adapter v1 at inference — the reference's lit_gpt/adapter.py (Config, GPT, Block, CausalSelfAttention,
adapter_filter, mark_only_adapter_as_trainable) on the MI355X kernels.

The adapter (https://arxiv.org/abs/2303.16199) touches no Linear. Every block ``i >= adapter_start_layer`` owns a learned
prefix ``adapter_wte`` (adapter_prompt_length rows of n_embd) and one ``gating_factor`` per head; after the block's
ordinary attention result ``y`` it adds

    y = y + gating_factor[h] * softmax(scale * q_roped @ ak^T) @ av

where ``ak`` / ``av`` are the k / v slices of ``attn.attn(adapter_wte.weight)``, never roped, all of them visible to every
query. They depend on the weights alone, so they are computed once per layer (one aT-row call of the layer's own qkv
Linear in whatever format it has), regrouped into (G, aT, hs) bf16 and kept until the weights change. The per-token work
is ONE ``lga_adapter_attention`` launch per adapted block (csrc/adapter.hip; include/litgpt_amd.h states its rounding
points, the reference's under bf16-true), right after the attention launch and before ``attn.proj``, in every route
that produces an attention result: the one-row decode step (fused or two launches), the prefill, the no-cache forward,
the fp8-cache forms and the batched, shared-prefix and window forms. The attention kernels and their callers are the base
classes', unchanged: the classes here call them and then ``ops.adapter_attention``. The kernel is row-wise, so every
multi-row route keeps its promise that row b has the bits of the one-sequence call.

``attach(model, state, config)`` turns an already built (and possibly quantized) ``lit_gpt.GPT`` into an adapter model,
as ``lora.attach`` does for LoRA; ``generate/adapter.py`` uses it after ``build_model``.

Refused (``NotImplementedError``, before any launch): fp32 activations (``--precision 32-true``), tensor parallelism,
``adapter_prompt_length`` > 64, and a model that also carries LoRA adapters.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn

from lit_gpt import ops
from lit_gpt.config import Config as BaseConfig
from lit_gpt.model import GPT as BaseModel
from lit_gpt.model import Block as BaseBlock
from lit_gpt.model import CausalSelfAttention as BaseCausalSelfAttention
from lit_gpt.model import _lin


@dataclass
class Config(BaseConfig):
    """lit_gpt.Config plus the reference's two adapter fields."""

    adapter_prompt_length: int = 10
    adapter_start_layer: int = 2


def check_supported(config: Config, *, precision: str = "bf16-true", world_size: int = 1) -> None:
    """What the adapter cannot run with on this build, refused before any weight is materialised."""
    aT = config.adapter_prompt_length
    if aT < 1:
        raise ValueError(f"adapter_prompt_length must be positive, got {aT}")
    if not 0 <= config.adapter_start_layer <= config.n_layer:
        raise ValueError(f"adapter_start_layer {config.adapter_start_layer} is outside the model's {config.n_layer} "
                         "layers")
    if aT > ops.ADAPTER_MAX_KEYS:
        raise NotImplementedError(f"adapter_prompt_length {aT}: the prefix-attention kernel takes at most "
                                  f"{ops.ADAPTER_MAX_KEYS} adapter keys")
    if config.head_size % 8 or config.head_size > ops.ADAPTER_MAX_HEAD_SIZE or config.rope_n_elem % 2:
        raise NotImplementedError(f"the prefix-attention kernel needs head_size % 8 == 0, head_size <= "
                                  f"{ops.ADAPTER_MAX_HEAD_SIZE} and an even rope_n_elem; got head_size "
                                  f"{config.head_size}, rope_n_elem {config.rope_n_elem}")
    if precision == "32-true":
        raise NotImplementedError("LLaMA-Adapter with --precision 32-true: the prefix-attention kernel computes on "
                                  "bf16 activations (bf16-true)")
    if world_size > 1:
        raise NotImplementedError("LLaMA-Adapter with tensor parallelism: the adapter term needs every head's gating "
                                  "factor and prefix keys on one device; run the adapter on one device")


def _check_model(model, every_module: bool = True) -> None:
    """The refusals that depend on the built model: fp32 activations, tensor-parallel hooks, LoRA adapters.
    ``every_module=False`` (each forward: an eager decode step should not walk a 7B model's module tree) looks for
    LoRA on the attention Linears and the head only; ``attach`` and ``set_kv_cache`` look everywhere."""
    from lit_gpt import comm, lora

    if model.transformer.wte.weight.dtype == torch.float32:
        raise NotImplementedError("LLaMA-Adapter with fp32 activations (--precision 32-true): the prefix-attention "
                                  "kernel computes on bf16 activations (bf16-true)")
    if comm.get_default() is not None or any(b._forward_hooks or b.attn._forward_hooks or b.mlp._forward_hooks
                                             for b in model.transformer.h):
        raise NotImplementedError("LLaMA-Adapter with forward hooks on a block (tensor parallelism): the adapter term "
                                  "runs on one device")
    if every_module:
        linears = model.modules()
    else:
        linears = [getattr(model, "lm_head", None)] + [getattr(b.attn, n, None) for b in model.transformer.h
                                                       for n in ("attn", "proj")]
    if getattr(model, "lora_adapters", None) is not None or any(
            isinstance(m, (lora.LoraLinear, lora.MultiLoraLinear)) for m in linears):
        raise NotImplementedError("LLaMA-Adapter on a model that also carries LoRA adapters: one kind of adapter at a "
                                  "time")


class GPT(BaseModel):
    """``lit_gpt.GPT`` whose blocks know their index: blocks from ``adapter_start_layer`` on add the adapter term."""

    def __init__(self, config: Config) -> None:
        nn.Module.__init__(self)  # (not the base constructor: every block is built once, as an adapter Block)
        assert config.padded_vocab_size is not None
        self.config = config
        self.lm_head = nn.Linear(config.n_embd, config.padded_vocab_size, bias=config.lm_head_bias)
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(config.padded_vocab_size, config.n_embd),
            h=nn.ModuleList(Block(config, i) for i in range(config.n_layer)),
            ln_f=config.norm_class(config.n_embd, eps=config.norm_eps),
        ))
        self.max_seq_length = self.config.block_size
        self.mask_cache: Optional[torch.Tensor] = None

    @classmethod
    def from_name(cls, name: str, **kwargs: Any) -> "GPT":
        return cls(Config.from_name(name, **kwargs))

    def _init_weights(self, module: nn.Module) -> None:
        super()._init_weights(module)
        if isinstance(module, CausalSelfAttention):
            module.reset_parameters()

    def _adapted(self):
        return [b.attn for b in self.transformer.h if getattr(b.attn, "adapted", False)]

    def drop_adapter_kv(self) -> None:
        """Forget every layer's prefix K / V (the weights they were computed from have changed)."""
        for attn in self._adapted():
            attn.adapter_kv_cache = None

    def build_adapter_kv(self) -> None:
        """Compute the prefix K / V of every adapted layer that has none (or stale ones) now: outside any graph."""
        if not self.transformer.wte.weight.is_cuda:
            return
        _check_model(self)
        check_supported(self.config)
        for attn in self._adapted():
            attn.adapter_kv()

    def set_kv_cache(self, *args: Any, **kwargs: Any) -> None:
        _check_model(self)
        super().set_kv_cache(*args, **kwargs)
        self.build_adapter_kv()

    def load_state_dict(self, *args: Any, **kwargs: Any):
        self.drop_adapter_kv()
        return super().load_state_dict(*args, **kwargs)

    def forward(self, *args: Any, **kwargs: Any) -> torch.Tensor:
        _check_model(self, every_module=False)
        return super().forward(*args, **kwargs)

    def decode_window(self, *args: Any, **kwargs: Any) -> torch.Tensor:
        _check_model(self, every_module=False)
        return super().decode_window(*args, **kwargs)


class Block(BaseBlock):
    """``lit_gpt.model.Block`` with the adapter's attention module."""

    def __init__(self, config: Config, block_idx: int) -> None:
        nn.Module.__init__(self)  # (the base constructor would build a base attention module first)
        self.norm_1 = config.norm_class(config.n_embd, eps=config.norm_eps)
        self.attn = CausalSelfAttention(config, block_idx)
        self.norm_2 = None if config.shared_attention_norm else config.norm_class(config.n_embd, eps=config.norm_eps)
        self.mlp = config.mlp_class(config)
        self.config = config


class CausalSelfAttention(BaseCausalSelfAttention):
    """``lit_gpt.model.CausalSelfAttention`` plus the gated attention over the adaption prompt."""

    def __init__(self, config: Config, block_idx: int) -> None:
        super().__init__(config)
        self.block_idx = block_idx
        if block_idx >= config.adapter_start_layer:
            self.adapter_wte = nn.Embedding(config.adapter_prompt_length, config.n_embd)
            self.gating_factor = nn.Parameter(torch.zeros(1, 1, config.n_head, 1))
        self.adapter_kv_cache: Optional[Tuple[torch.Tensor, torch.Tensor, tuple]] = None

    @property
    def adapted(self) -> bool:
        return self.block_idx >= self.config.adapter_start_layer

    def reset_parameters(self) -> None:
        if self.adapted:
            nn.init.zeros_(self.gating_factor)

    def _load_from_state_dict(self, state_dict: Dict, prefix: str, *args: Any, **kwargs: Any) -> None:
        # older checkpoints store the gating factor as (1, n_head, 1, 1)
        key = prefix + "gating_factor"
        if key in state_dict:
            state_dict[key] = _gating_layout(state_dict[key], self.config.n_head, key)
        self.adapter_kv_cache = None
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # ---- the prefix K / V
    def _weights_key(self) -> tuple:
        """What ``adapter_kv_cache`` was computed from: the qkv Linear module, and the storage and version counter of
        its tensors and of the prefix. A conversion to another weight format, a load, a move to another device or an
        in-place update (``copy_``, an optimizer step) changes it. Tensors made under ``torch.inference_mode`` (what
        the generate scripts build) keep no version counter; nothing updates those in place but ``load_state_dict``,
        which drops the cache itself."""
        lin = self.attn
        tensors = [*lin.parameters(recurse=True), *lin.buffers(recurse=True), self.adapter_wte.weight]
        return (id(lin), *((t.data_ptr(), -1 if t.is_inference() else t._version) for t in tensors))

    def adapter_kv(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(ak, av), each (G, aT, hs) bf16: the k and v slices of ``attn.attn(adapter_wte.weight)``, un-expanded, never
        roped. Computed on first use after the weights changed: one aT-row call of the layer's qkv Linear."""
        key = self._weights_key()
        kv = self.adapter_kv_cache
        if kv is not None and kv[2] == key:
            return kv[0], kv[1]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the adapter's prefix K / V are missing inside a graph capture: call set_kv_cache (or "
                               "build_adapter_kv) after the weights change and before capturing")
        c = self.config
        G, hs, aT = c.n_query_groups, c.head_size, c.adapter_prompt_length
        qpk = c.n_head // G
        prefix = self.adapter_wte.weight
        if prefix.dtype != torch.bfloat16 or tuple(prefix.shape) != (aT, c.n_embd):
            raise NotImplementedError(f"adapter_wte must be ({aT}, {c.n_embd}) bf16, got {tuple(prefix.shape)} "
                                      f"{prefix.dtype}")
        aqkv = _lin(self.attn, prefix.detach().contiguous().view(1, aT, c.n_embd)).view(aT, G, qpk + 2, hs)
        ak = aqkv[:, :, qpk].transpose(0, 1).contiguous()
        av = aqkv[:, :, qpk + 1].transpose(0, 1).contiguous()
        self.adapter_kv_cache = (ak, av, key)
        return ak, av

    # ---- the adapter term, once per attention result
    def _adapt(self, y: torch.Tensor, qkv: torch.Tensor, pos: torch.Tensor, pos_mode: str, cos: torch.Tensor,
               sin: torch.Tensor, active: Optional[torch.Tensor] = None) -> torch.Tensor:
        c = self.config
        H, G, hs = c.n_head, c.n_query_groups, c.head_size
        if qkv.dtype != torch.bfloat16:
            raise NotImplementedError(f"LLaMA-Adapter with {qkv.dtype} activations: the prefix-attention kernel takes "
                                      "bf16")
        ak, av = self.adapter_kv()
        gating = self.gating_factor.detach().reshape(-1)
        if gating.dtype != torch.bfloat16:
            raise NotImplementedError(f"gating_factor must be bf16 on the device, got {gating.dtype}")
        cos = cos.to(device=qkv.device, dtype=torch.float32).contiguous()
        sin = sin.to(device=qkv.device, dtype=torch.float32).contiguous()
        ops.adapter_attention(y.view(qkv.size(0), H * hs), qkv, ak, av, gating, pos, cos, sin, H, G, hs, c.rope_n_elem,
                              1.0 / math.sqrt(hs), pos_mode=pos_mode, active=active)
        return y

    def _attend(self, qkv, cache, pos, rope_pos, cos, sin, out=None) -> torch.Tensor:
        if not self.adapted:
            return super()._attend(qkv, cache, pos, rope_pos, cos, sin, out)
        # (the base's one-row routes go through _decode_attention: the term is added here, once, not there too)
        self._in_attend = True
        try:
            y = super()._attend(qkv, cache, pos, rope_pos, cos, sin, out)
        finally:
            self._in_attend = False
        return self._adapt(y, qkv, rope_pos, "rows", cos, sin)

    _in_attend = False

    def _decode_attention(self, form, qkv, cache, pos, rope_pos, cos, sin, active=None, out=None,
                          prefix_len=None) -> torch.Tensor:
        y = super()._decode_attention(form, qkv, cache, pos, rope_pos, cos, sin, active=active, out=out,
                                      prefix_len=prefix_len)
        if not self.adapted or self._in_attend:
            return y
        if form == "window":  # row r at pos[0] + r
            return self._adapt(y, qkv, pos, "window", cos, sin)
        if form == "shared":  # every sample at the one position pos[0]
            return self._adapt(y, qkv, pos, "one", cos, sin, active)
        return self._adapt(y, qkv, rope_pos, "rows", cos, sin, active)


def mark_only_adapter_as_trainable(model: GPT) -> None:
    """``requires_grad`` on for the adapter's parameters, off for everything else."""
    for name, param in model.named_parameters():
        param.requires_grad = adapter_filter(name, param)


def adapter_filter(key: str, value: Any) -> bool:
    return "adapter_wte" in key or "gating_factor" in key


def _gating_layout(t: torch.Tensor, n_head: int, key: str) -> torch.Tensor:
    """A checkpoint's gating factor as (1, 1, n_head, 1); the older (1, n_head, 1, 1) layout is accepted."""
    if tuple(t.shape) == (1, 1, n_head, 1):
        return t
    if tuple(t.shape) == (1, n_head, 1, 1):
        return t.permute(0, 2, 1, 3)
    raise ValueError(f"{key} has shape {tuple(t.shape)}, expected (1, 1, {n_head}, 1) or (1, {n_head}, 1, 1)")


def adapter_state(state: Dict[str, torch.Tensor], config: Config) -> Dict[str, torch.Tensor]:
    """The adapter tensors of a checkpoint under the reference's names, checked against ``config``: ``state`` may be
    nested under ``"model"`` and may carry base weights too (ignored). A missing or mis-shaped adapter tensor raises
    ``ValueError`` naming the key; gating factors come back as (1, 1, n_head, 1)."""
    state = state.get("model", state)
    out = {}
    for i in range(config.adapter_start_layer, config.n_layer):
        kw, kg = f"transformer.h.{i}.attn.adapter_wte.weight", f"transformer.h.{i}.attn.gating_factor"
        for k in (kw, kg):
            if k not in state:
                raise ValueError(f"adapter checkpoint has no {k} (adapter_start_layer {config.adapter_start_layer}, "
                                 f"{config.n_layer} layers)")
        w = state[kw]
        if tuple(w.shape) != (config.adapter_prompt_length, config.n_embd):
            raise ValueError(f"{kw} has shape {tuple(w.shape)}, expected (adapter_prompt_length "
                             f"{config.adapter_prompt_length}, n_embd {config.n_embd})")
        out[kw] = w
        out[kg] = _gating_layout(state[kg], config.n_head, kg)
    return out


def attach(model, state: Dict[str, torch.Tensor], config: Config):
    """Turn an already built ``lit_gpt.GPT`` (any weight format, bf16 activations) into an adapter model carrying the
    adapter tensors of ``state`` (``adapter_state``: the reference's key names, flat or under ``"model"``, base
    weights ignored). A bad checkpoint leaves the model as it was. Returns the model, now a ``lit_gpt.adapter.GPT``."""
    from lit_gpt import comm

    group = comm.get_default()
    wte = model.transformer.wte.weight
    check_supported(config, precision="32-true" if wte.dtype == torch.float32 else "bf16-true",
                    world_size=1 if group is None else group.world)
    _check_model(model)
    mc = model.config
    for f in ("n_layer", "n_head", "n_query_groups", "n_embd", "head_size", "rope_n_elem"):
        if getattr(mc, f) != getattr(config, f):
            raise ValueError(f"the adapter config's {f} ({getattr(config, f)}) is not the model's ({getattr(mc, f)})")
    tensors = adapter_state(state, config)
    model.__class__ = GPT
    model.config = config
    for i, block in enumerate(model.transformer.h):
        block.__class__ = Block
        attn = block.attn
        attn.__class__ = CausalSelfAttention
        block.config = attn.config = config
        attn.block_idx = i
        attn.adapter_kv_cache = None
        if i >= config.adapter_start_layer:
            pre = f"transformer.h.{i}.attn"
            w = tensors[f"{pre}.adapter_wte.weight"].detach().to(device=wte.device, dtype=wte.dtype).contiguous()
            g = tensors[f"{pre}.gating_factor"].detach().to(device=wte.device, dtype=wte.dtype).contiguous()
            attn.adapter_wte = nn.Embedding.from_pretrained(w, freeze=True)
            attn.gating_factor = nn.Parameter(g, requires_grad=False)
        else:
            for name in ("adapter_wte", "gating_factor"):
                if hasattr(attn, name):
                    delattr(attn, name)
    model.build_adapter_kv()
    return model


def random_adapter(config: Config, seed: int = 1234, gating_std: float = 0.5) -> Dict[str, torch.Tensor]:
    """A seeded random adapter in the reference's key names and shapes (``--synthetic``, tools, tests): the prefix as
    ``nn.Embedding`` initialises it (standard normal), the gating factors normal with ``gating_std`` (the reference's
    zero init would leave the model unchanged)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i in range(config.adapter_start_layer, config.n_layer):
        pre = f"transformer.h.{i}.attn"
        out[f"{pre}.adapter_wte.weight"] = torch.randn(config.adapter_prompt_length, config.n_embd, generator=g)
        out[f"{pre}.gating_factor"] = torch.randn(1, 1, config.n_head, 1, generator=g) * gating_std
    return out
