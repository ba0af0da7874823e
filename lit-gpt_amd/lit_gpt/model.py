"""GPT / Block / CausalSelfAttention / KVCache with the reference's module API and an MI355X HIP hot path.

Public surface kept from /root/reference/lit_gpt/model.py: ``GPT(config)``; ``GPT.forward(idx,
input_pos=None)`` (:499-519); ``max_seq_length`` property/setter (:462-484); ``rope_cache`` (:525-532);
``set_kv_cache`` / ``clear_kv_cache`` (:534-559); ``from_name`` (:521-523); ``_init_weights`` (:490-497);
attributes ``config, lm_head, transformer.{wte,h,ln_f}, cos, sin, mask_cache``. ``Block.forward(x, cos, sin,
mask=None, input_pos=None)`` (:572-593) with ``norm_1, attn, norm_2, mlp``; ``CausalSelfAttention.forward``
(:609-656) with ``attn`` (fused qkv Linear), ``proj``, ``kv_cache``, ``build_kv_cache``,
``scaled_dot_product_attention``; ``KVCache`` (:776-799); ``LLaMAMLP`` / ``LLaMAMoE`` / ``GptNeoxMLP`` classes
(``generate/tp.py`` isinstance-checks them); ``build_rope_cache`` / ``apply_rope`` / ``build_mask_cache``.

What runs underneath (GPU, bf16 activations, Linears converted by ``QuantizedPrecision``): every op is a HIP
kernel from ``liblitgpt_amd.so`` — embedding gather, RMSNorm fused into the qkv / fc GEMV prologue, RoPE fused
with the KV-cache append, split-sequence decode attention, the out-projections with the residual add in their
epilogue, SwiGLU fused into the dual fc_1/fc_2 GEMV, and greedy argmax. Differences from the reference that do
not change results: the KV cache holds ``n_query_groups`` heads (un-expanded GQA) and the bool mask is never
materialised on the hot path (the kernels read keys ``<= input_pos``). RoPE positions follow the reference's
default-dtype semantics (``build_rope_cache``), so ``generate.base.build_model`` reproduces the bf16 rounding of
positions > 256 that the reference's bf16 ``init_tensor`` context produces.
"""

from __future__ import annotations

import math
import os
from typing import Any, Optional, Tuple

import torch
import torch.nn as nn

from lit_gpt import comm, ops, quantize
from lit_gpt.config import Config
from lit_gpt.rmsnorm import RMSNorm, _gpu_only


def _lin(linear: nn.Module, x: torch.Tensor, *, reduce=None, **kw) -> torch.Tensor:
    """Run a Linear on the MI355X kernels (lit_gpt/quantize.py ``kernels``). ``reduce``: the TP all-reduce hook of a
    row-parallel projection (generate/tp.py) — the partial output is summed over the ranks (+ ``residual``), fused
    into the GEMV launch for one-token inputs (lit_gpt/comm.py linear_reduce)."""
    if reduce is not None:
        res = kw.pop("residual", None)
        return comm.linear_reduce(reduce, linear, x, res, lambda: quantize.kernels(linear)(x, **kw))
    return quantize.kernels(linear)(x, **kw)


class GPT(nn.Module):
    def __init__(self, config: Config) -> None:
        super().__init__()
        assert config.padded_vocab_size is not None
        self.config = config
        self.lm_head = nn.Linear(config.n_embd, config.padded_vocab_size, bias=config.lm_head_bias)
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(config.padded_vocab_size, config.n_embd),
            h=nn.ModuleList(Block(config) for _ in range(config.n_layer)),
            ln_f=config.norm_class(config.n_embd, eps=config.norm_eps),
        ))
        self.max_seq_length = self.config.block_size
        self.mask_cache: Optional[torch.Tensor] = None

    @property
    def max_seq_length(self) -> int:
        return self._max_seq_length

    @max_seq_length.setter
    def max_seq_length(self, value: int) -> None:
        if value > self.config.block_size:
            raise ValueError(f"Cannot attend to {value}, block size is only {self.config.block_size}")
        self._max_seq_length = value
        if not hasattr(self, "cos"):
            cos, sin = self.rope_cache()
            self.register_buffer("cos", cos, persistent=False)
            self.register_buffer("sin", sin, persistent=False)
        elif value != self.cos.size(0):
            self.cos, self.sin = self.rope_cache(device=self.cos.device)

    def reset_parameters(self) -> None:
        self.cos, self.sin = self.rope_cache()

    def _init_weights(self, module: nn.Module) -> None:
        if isinstance(module, nn.Linear):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if module.bias is not None:
                torch.nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)

    def _rope_tables(self) -> Tuple[torch.Tensor, torch.Tensor]:
        # model.to(bf16) would also cast the rope buffers; the kernels need the exact fp32 tables
        if self.cos.dtype != torch.float32 or self.cos.size(0) != self.max_seq_length:
            self.cos, self.sin = self.rope_cache(device=self.cos.device)
        return self.cos, self.sin

    def forward(self, idx: torch.Tensor, input_pos: Optional[torch.Tensor] = None, *,
                last_token_only: bool = False, embedded: Optional[torch.Tensor] = None,
                hidden_only: bool = False, kv_slot: int = 0, active: Optional[torch.Tensor] = None,
                shared_prefix: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B=1, T) ids -> (1, T, padded_vocab) logits; ``last_token_only`` computes only the last row (1, 1, V)
        — all that ``generate`` samples from (generate/base.py:31). ``embedded`` (T * n_embd bf16) is
        ``transformer.wte(idx)`` already gathered — by the previous decode step's ``ops.argmax_embed`` in
        ``DecodeGraph`` — and replaces the embedding launch. ``hidden_only`` stops before ln_f / lm_head and returns
        the last block's output (DecodeGraph runs the head fused with the greedy argmax). ``kv_slot``: the slot of a
        ``set_kv_cache(batch_size > 1)`` cache that a B = 1 call reads and writes.

        (B <= MAX_BATCH = 4, T) with a KV cache is the batched form (``_forward_batch``): T > 1 runs each row as the
        B = 1 prefill on slot b at the shared ``input_pos`` (T,); T = 1 is one batched decode step, ``input_pos`` (1,)
        shared or (B,) / (B, 1) one position per sequence, ``embedded`` (B * n_embd). Row b has the bits of the B = 1
        call on that sequence. ``active`` (B,) int32 on the device (batched decode step only, B >= 1): a row flagged 0 is
        idle — its cache slot is left untouched and its logits are not meaningful. ``shared_prefix`` (1,) int64 on the
        device (batched decode step only): the rows are samples of ONE prompt at one shared position, and the keys below
        that length are read from slot 0 alone (``CausalSelfAttention.decode_rows``); the logits are those of the step
        without it on caches whose every slot holds the prompt."""
        B, T = idx.shape
        if self.max_seq_length < T:
            raise ValueError(f"Cannot forward sequence of length {T}, max seq length is only {self.max_seq_length}.")
        if input_pos is not None and self.mask_cache is None:
            raise TypeError("You need to call `gpt.set_kv_cache()`")
        if not idx.is_cuda:
            _gpu_only("GPT.forward")
        if B != 1 or active is not None or shared_prefix is not None:
            # (a one-slot engine, B = 1 with ``active``, is a batched step of one row)
            return self._forward_batch(idx, input_pos, last_token_only, embedded, hidden_only, active, shared_prefix)
        cos, sin = self._rope_tables()
        if input_pos is not None:
            input_pos = input_pos.to(device=idx.device, dtype=torch.int64).contiguous()
        if embedded is not None:
            if embedded.numel() != T * self.transformer.wte.weight.shape[1] or embedded.dtype != torch.bfloat16:
                raise ValueError("embedded must hold T * n_embd bf16 values (the gathered wte rows of idx)")
            x = embedded.view(1, T, -1)
        else:
            x = ops.embedding(idx.reshape(-1).contiguous(), self.transformer.wte.weight).view(1, T, -1)
        for block in self.transformer.h:
            x = block(x, cos, sin, None, input_pos, kv_slot=kv_slot)
        if last_token_only:
            x = x[:, -1:].contiguous()
        if hidden_only:
            return x
        ln = self.transformer.ln_f
        if isinstance(ln, RMSNorm):
            return _lin(self.lm_head, x, norm_weight=ln.weight, norm_eps=ln.eps)
        return _lin(self.lm_head, ln(x))

    # Sequences per batched decode step. The rows kernels take up to ops.MAX_GEMV_ROWS = 8 rows, but measured on the
    # Llama-2-7B shapes an 8-row launch is no faster than the MFMA prefill GEMM at 8 rows, while at 2
    # and 4 rows it beats both that GEMM and M one-row launches: 4 is the largest measured batch where both hold
    MAX_BATCH = 4

    def _batch_check(self, B: int) -> None:
        """What the batched route (B > 1) covers: up to MAX_BATCH sequences, dense RMSNorm / LLaMAMLP blocks whose
        Linears are all 4-bit ``QuantLinear`` and carry no hooks. Everything else is refused here, before any launch."""
        if B > self.MAX_BATCH:
            raise NotImplementedError(f"batch size {B}: the MI355X batched decode runs at most {self.MAX_BATCH} "
                                      "sequences per step")
        self._rows_check("batch size > 1", adapters=True)

    def _rows_check(self, what: str, adapters: bool = False) -> None:
        """What every multi-row decode step (the batched step, the speculative verify window) needs of the model.
        ``adapters`` (the batched step only): a ``lora.MultiLoraLinear`` (``lora.attach_many``: one adapter per row of
        the batch) counts as its base Linear; a single-adapter ``LoraLinear`` stays refused."""
        from lit_gpt.lora import MultiLoraLinear  # (lit_gpt.lora imports this package)

        def four_bit(lin, name):
            if adapters and isinstance(lin, MultiLoraLinear) and not lin._forward_hooks:
                lin = lin.base
            if type(lin) is not quantize.QuantLinear or lin._forward_hooks:
                raise NotImplementedError(
                    f"{what} with {name} a {type(lin).__name__}: the multi-row decode GEMV streams plain "
                    f"4-bit Linears only (--quantize {quantize.ROWS_MODES}); LoRA-attached, bnb.int8, bf16 and fp32 "
                    "Linears decode one sequence at a time (a batch takes adapters attached with lora.attach_many)")

        for i, blk in enumerate(self.transformer.h):
            if blk.config.parallel_residual or not isinstance(blk.norm_1, RMSNorm):
                raise NotImplementedError(f"{what} with parallel-residual (GPT-NeoX) blocks: the batched decode "
                                          "runs RMSNorm / LLaMAMLP blocks only")
            if not isinstance(blk.mlp, LLaMAMLP):
                raise NotImplementedError(f"{what} with a {type(blk.mlp).__name__} (sparse-MoE) block: the "
                                          "routed expert kernels decode one sequence at a time")
            if blk.attn._forward_hooks or blk.mlp._forward_hooks or blk._forward_hooks:
                raise NotImplementedError(f"{what} with forward hooks on a block (tensor parallelism): the "
                                          "fused GEMV + all-reduce decodes one sequence at a time")
            for name in ("attn.attn", "attn.proj", "mlp.fc_1", "mlp.fc_2", "mlp.proj"):
                four_bit(blk.get_submodule(name), f"transformer.h.{i}.{name}")
        four_bit(self.lm_head, "lm_head")
        if not isinstance(self.transformer.ln_f, RMSNorm):
            raise NotImplementedError(f"{what} needs an RMSNorm ln_f")

    # Rows per speculative verify window (``decode_window``). The kernels take ops.MAX_WINDOW_ROWS = 8, and the cap
    # stays there: measured at M = 2, 4, 8 the window attention launch costs 0.77 / 0.53 / 0.38 of M
    # one-row launches on the Llama-2-7B geometry (0.77 / 0.55 / 0.41 with 8 query groups), so no M fails the criterion
    # that capped MAX_BATCH. (Whether a long window pays is the drafter's acceptance rate, not this cap.)
    MAX_WINDOW = 8

    def decode_window(self, idx: torch.Tensor, pos0: torch.Tensor, *, embedded: Optional[torch.Tensor] = None,
                      hidden_only: bool = False) -> torch.Tensor:
        """One verify step of greedy speculative decoding: ``idx`` (M,) are M <= MAX_WINDOW consecutive tokens of ONE
        sequence, row r at position ``pos0[0] + r`` (``pos0`` (1,) int64 on the device, read by the kernels: a
        captured graph stays valid as it advances). Returns (M, padded_vocab) logits whose row r has the bits of the
        one-row ``forward(idx[r], pos0 + r)`` after rows 0..r-1, and leaves the KV cache (slot 0) as those M steps
        would: the batched step's layer sequence on the rows GEMVs (every weight streamed once for the M rows) with
        ``ops.attention_decode_window`` once per block. Rows that a later round rejects leave stale K/V past the
        accepted position; decode attention never reads past its row's position and the next window overwrites them.
        ``embedded`` (M * n_embd bf16) replaces the embedding launch; ``hidden_only`` stops before ln_f / lm_head."""
        M = idx.numel()
        if not 1 <= M <= self.MAX_WINDOW:
            raise NotImplementedError(f"window of {M} rows: the speculative verify step runs 1..{self.MAX_WINDOW} "
                                      "rows")
        self._rows_check("a speculative verify window")
        c = self.config
        if not ops.decode_fusable(c.head_size, c.rope_n_elem) or c.n_head // c.n_query_groups not in (1, 2, 4, 8):
            raise NotImplementedError("a speculative verify window needs the fused decode attention's geometry "
                                      "(head_size == rope_n_elem == 128, 1 / 2 / 4 / 8 heads per query group)")
        if not idx.is_cuda:
            _gpu_only("GPT.decode_window")
        if self.mask_cache is None or self.transformer.h[0].attn.kv_cache is None:
            raise TypeError("You need to call `gpt.set_kv_cache()`")
        if pos0.numel() != 1 or pos0.dtype != torch.int64 or pos0.device != idx.device:
            raise ValueError("pos0 must be one int64 position on the model's device")
        return self._rows_step(idx, embedded, hidden_only,
                               lambda attn, x, cos, sin, **kw: attn.decode_window(x, cos, sin, pos0, **kw)).view(M, -1)

    def _rows_step(self, idx, embedded, hidden_only, attend) -> torch.Tensor:
        """What the batched decode step and the verify window share: R = idx.numel() rows x (R, C), gathered here or
        passed as ``embedded``; every block on the rows GEMVs with ``attend`` as its attention (``Block.decode_rows``);
        then the last block's output (``hidden_only``) or ln_f fused into the rows lm_head -> (R, padded_vocab)."""
        R, C = idx.numel(), self.transformer.wte.weight.shape[1]
        cos, sin = self._rope_tables()
        if embedded is not None:
            if embedded.numel() != R * C or embedded.dtype != torch.bfloat16:
                raise ValueError(f"embedded must hold {R} * n_embd bf16 values (the gathered wte rows of idx)")
            x = embedded.view(R, C)
        else:
            x = ops.embedding(idx.reshape(-1).contiguous(), self.transformer.wte.weight).view(R, C)
        for block in self.transformer.h:
            x = block.decode_rows(x, cos, sin, attend)
        if hidden_only:
            return x
        ln = self.transformer.ln_f
        return _lin(self.lm_head, x, norm_weight=ln.weight, norm_eps=ln.eps, rows=True)

    def _forward_batch(self, idx, input_pos, last_token_only, embedded, hidden_only, active=None,
                       shared_prefix=None) -> torch.Tensor:
        """The B > 1 forms of ``forward`` (its docstring). T = 1 per block: the rows qkv GEMV with norm_1 fused, the
        decode attention of every sequence on its own cache slot (one batch launch, ``CausalSelfAttention.decode_rows``;
        ``active`` flags idle rows), the rows out-projection + residual, the
        rows SwiGLU pair with norm_2 fused, the rows down-projection + residual; then ln_f fused into the rows
        lm_head. Every launch is serial on the current stream, so the step captures as one unbranched HIP graph."""
        B, T = idx.shape
        self._batch_check(B)
        if input_pos is None:
            raise NotImplementedError("batch size > 1 runs with a KV cache only (pass input_pos)")
        kv = self.transformer.h[0].attn.kv_cache
        if kv is None or kv.k.size(0) < B:
            raise ValueError(f"batch size {B} needs set_kv_cache(batch_size >= {B})")
        input_pos = input_pos.to(device=idx.device, dtype=torch.int64)
        if T > 1:  # the reference's shared positions: each row is the B = 1 prefill on its slot
            if embedded is not None or active is not None or shared_prefix is not None:
                raise ValueError("embedded / active / shared_prefix: one token per sequence (T = 1) only")
            return torch.cat([self.forward(idx[b:b + 1], input_pos, last_token_only=last_token_only,
                                           hidden_only=hidden_only, kv_slot=b) for b in range(B)])
        if input_pos.numel() == 1:
            pos = input_pos.reshape(1).expand(B).contiguous()
        elif input_pos.numel() == B:
            pos = input_pos.reshape(B).contiguous()
        else:
            raise ValueError(f"input_pos must hold 1 (shared) or {B} (one per sequence) positions for a batched "
                             f"decode step, got shape {tuple(input_pos.shape)}")
        if active is not None and (active.numel() != B or active.dtype != torch.int32 or active.device != idx.device):
            raise ValueError(f"active must hold {B} int32 flags on the model's device")
        if shared_prefix is not None:
            if input_pos.numel() != 1:
                raise ValueError("shared_prefix: the samples of one prompt sit at ONE position, input_pos (1,)")
            if (shared_prefix.numel() != 1 or shared_prefix.dtype != torch.int64
                    or shared_prefix.device != idx.device):
                raise ValueError("shared_prefix must be one int64 length on the model's device")
            self._shared_check()
            pos = input_pos.reshape(1).contiguous()
        return self._rows_step(idx, embedded, hidden_only,
                               lambda attn, x, cos, sin, **kw: attn.decode_rows(x, cos, sin, pos, active=active,
                                                                                shared_prefix=shared_prefix, **kw)
                               ).view(B, 1, -1)

    def _shared_check(self) -> None:
        """What a shared-prefix step (``forward(..., shared_prefix=)``) needs beyond ``_batch_check``: the bf16 cache
        and the batch launch's geometry in every block. Refused here, before any launch."""
        for blk in self.transformer.h:
            kv = blk.attn.kv_cache
            if kv is not None and kv.fp8:
                raise NotImplementedError("a shared prompt prefix over an fp8 KV cache: the shared-prefix decode "
                                          "attention reads bf16 caches only")
            if not blk.attn.batch_fusable(self.transformer.wte.weight.dtype):
                raise NotImplementedError("a shared prompt prefix needs the batched decode attention launch: head_size "
                                          "== rope_n_elem == 128, 1 / 2 / 4 / 8 heads per query group, bf16 "
                                          "activations")

    @classmethod
    def from_name(cls, name: str, **kwargs: Any) -> "GPT":
        return cls(Config.from_name(name, **kwargs))

    def rope_cache(self, device: Optional[torch.device] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        return build_rope_cache(seq_len=self.max_seq_length, n_elem=self.config.rope_n_elem, device=device,
                                condense_ratio=self.config.rope_condense_ratio, base=self.config.rope_base)

    def set_kv_cache(self, batch_size: int, rope_cache_length: Optional[int] = None,
                     device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None) -> None:
        """``dtype=torch.float8_e4m3fn`` builds the fp8 cache (``KVCache``): e4m3 codes plus one
        power-of-two scale per row, 132 B per row instead of 256. Every weight format takes it; what the fp8 attention
        kernels do not cover is refused here, before any launch."""
        if rope_cache_length is None:
            rope_cache_length = self.cos.size(-1)
        if dtype == torch.float8_e4m3fn:
            self._kv8_check()
        for block in self.transformer.h:
            block.attn.kv_cache = block.attn.build_kv_cache(batch_size, self.max_seq_length, rope_cache_length,
                                                            device, dtype)
        if dtype == torch.float8_e4m3fn:
            # the cached prefill (T > 1) expands a layer's cache into this bf16 pair for the MFMA flash kernels: one
            # pair for the model, every layer's attention is done with it before the next one fills it
            kv0 = self.transformer.h[0].attn.kv_cache
            scratch = tuple(torch.empty(kv0.k.shape[1:], dtype=torch.bfloat16, device=kv0.k.device) for _ in range(2))
            for block in self.transformer.h:
                block.attn.kv_cache.scratch = scratch
        if self.mask_cache is None or self.mask_cache.size(3) != self.max_seq_length:
            self.mask_cache = CausalMask(self.max_seq_length, device or self.transformer.wte.weight.device)

    def _kv8_check(self) -> None:
        """What the fp8 KV cache needs: the fused decode attention's geometry, bf16 activations, one device."""
        c = self.config
        if not ops.decode_fusable(c.head_size, c.rope_n_elem) or c.n_head // c.n_query_groups not in (1, 2, 4, 8):
            raise NotImplementedError("an fp8 KV cache needs the fused decode attention's geometry (head_size == "
                                      f"rope_n_elem == 128, 1 / 2 / 4 / 8 heads per query group); got head_size "
                                      f"{c.head_size}, rope_n_elem {c.rope_n_elem}, {c.n_head} heads in "
                                      f"{c.n_query_groups} groups")
        if self.transformer.wte.weight.dtype == torch.float32:
            raise NotImplementedError("an fp8 KV cache under --precision 32-true: the fp8 attention kernels take bf16 "
                                      "activations (the fp32 path keeps an fp32 cache)")
        if comm.get_default() is not None or any(comm.tp_hook(b.attn) is not None for b in self.transformer.h):
            raise NotImplementedError("an fp8 KV cache under tensor parallelism: the per-rank decode step keeps the "
                                      "bf16 cache")

    def clear_kv_cache(self) -> None:
        self.mask_cache = None
        for block in self.transformer.h:
            block.attn.kv_cache = None


class Block(nn.Module):
    def __init__(self, config: Config) -> None:
        super().__init__()
        self.norm_1 = config.norm_class(config.n_embd, eps=config.norm_eps)
        self.attn = CausalSelfAttention(config)
        self.norm_2 = None if config.shared_attention_norm else config.norm_class(config.n_embd, eps=config.norm_eps)
        self.mlp = config.mlp_class(config)
        self.config = config

    def decode_rows(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, attend) -> torch.Tensor:
        """One multi-row decode step (GPT._rows_check has checked the block): x (R, C) on the multi-row GEMVs, one token
        of each of R sequences or R consecutive tokens of one; row r has the bits of ``forward`` on that token.
        ``attend`` is the step's attention, ``CausalSelfAttention.decode_rows`` or ``.decode_window`` bound to its
        positions (``GPT._rows_step``)."""
        x = attend(self.attn, x, cos, sin, norm=self.norm_1, residual=x)
        g = quantize.swiglu(self.mlp.fc_1, self.mlp.fc_2, x, self.norm_2, rows=True)
        return _lin(self.mlp.proj, g, residual=x, rows=True)

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mask: Optional[torch.Tensor] = None,
                input_pos: Optional[torch.Tensor] = None, *, kv_slot: int = 0) -> torch.Tensor:
        c = self.config
        if c.shared_attention_norm and not c.parallel_residual:
            raise NotImplementedError("No checkpoint amongst the ones we support uses this configuration"
                                      " (non-parallel residual and shared attention norm).")
        if c.parallel_residual:
            return self._parallel_forward(x, cos, sin, mask, input_pos, kv_slot)
        if not isinstance(self.norm_1, RMSNorm) or not isinstance(self.mlp, (LLaMAMLP, LLaMAMoE)):
            raise NotImplementedError(f"{type(self.mlp).__name__} / {type(self.norm_1).__name__} blocks have no "
                                      "MI355X kernels in this build")
        if input_pos is not None and isinstance(self.mlp, LLaMAMoE) and isinstance(self.mlp.experts[0].fc_1, nn.Linear):
            # (refused at the prefill already, not at the first decode step: generation needs the 4-bit expert kernels)
            raise NotImplementedError("LLaMAMoE on the MI355X needs bias-free QuantLinear experts of one format for "
                                      "generation (the KV-cache forward); unquantized experts serve only the no-cache "
                                      "multi-row forward that scoring uses")
        # The norms ride the qkv / fc GEMV prologues and the residual adds the out-projection epilogues. Under
        # tensor parallelism (generate/tp.py's all_reduce_output hook on attn / mlp) the projections yield partial
        # sums: the module then runs without its hook and the reduction + residual add is one fused kernel
        # (lit_gpt/comm.py); any other forward hook keeps the reference's call-the-module semantics.
        ha = comm.tp_hook(self.attn)
        hm = comm.tp_hook(self.mlp)
        if ha is not None:
            x = self.attn.forward(x, cos, sin, mask, input_pos, norm=self.norm_1, residual=x, reduce=ha,
                                  kv_slot=kv_slot)
        elif not self.attn._forward_hooks:
            x = self.attn(x, cos, sin, mask, input_pos, norm=self.norm_1, residual=x, kv_slot=kv_slot)
        else:
            x = ops.add(self.attn(self.norm_1(x), cos, sin, mask, input_pos, kv_slot=kv_slot).contiguous(),
                        x.contiguous())
        if hm is not None and isinstance(self.mlp, LLaMAMLP):
            return self.mlp.forward(x, norm=self.norm_2, residual=x, reduce=hm)
        if hm is not None:
            return comm.reduce_add(hm, self.mlp, self.mlp.forward(x, norm=self.norm_2), x)
        if not self.mlp._forward_hooks:  # (a sparse-MoE block applies its experts' TP hooks itself)
            return self.mlp(x, norm=self.norm_2, residual=x)
        return ops.add(self.mlp(self.norm_2(x)).contiguous(), x)


    def _parallel_forward(self, x, cos, sin, mask, input_pos, kv_slot) -> torch.Tensor:
        """GPT-NeoX block (reference model.py:572-593, parallel_residual): n_1 = norm_1(x), h = attn(n_1),
        n_2 = n_1 if shared_attention_norm else norm_2(x), x = mlp(n_2) + h + x — the reference's association:
        bf16(mlp + h) (fused into the mlp.proj epilogue) then + x. Under tensor parallelism the attn / mlp outputs
        go through their all-reduce hooks first (generate/tp.py), as in the reference."""
        n_1 = self.norm_1(x)
        h = self.attn(n_1, cos, sin, mask, input_pos, kv_slot=kv_slot).contiguous()
        n_2 = n_1 if self.config.shared_attention_norm else self.norm_2(x)
        if self.mlp._forward_hooks:  # TP: the hook must see the mlp output alone
            m = ops.add(self.mlp(n_2).contiguous(), h)
        else:
            m = self.mlp(n_2, residual=h)
        return ops.add(m.contiguous(), x.contiguous()).view_as(x)


class CausalSelfAttention(nn.Module):
    def __init__(self, config: Config) -> None:
        super().__init__()
        shape = (config.n_head + 2 * config.n_query_groups) * config.head_size
        self.attn = nn.Linear(config.n_embd, shape, bias=config.bias)
        self.proj = nn.Linear(config.n_embd, config.n_embd, bias=config.bias)
        self.kv_cache: Optional[KVCache] = None
        self.config = config

    # decode tokens (T = 1) with full 128-dim rotary use lga_attention_decode_fused; False keeps the two-launch
    # rope_kv_append + attention path (bit-identical; tests compare the two)
    fuse_decode = True

    def forward(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mask: Optional[torch.Tensor] = None,
                input_pos: Optional[torch.Tensor] = None, *, norm: Optional["RMSNorm"] = None,
                residual: Optional[torch.Tensor] = None, reduce=None, kv_slot: int = 0) -> torch.Tensor:
        """``norm`` / ``residual`` / ``reduce`` are fusion hooks used by Block.forward: the RMSNorm runs in the qkv
        GEMV prologue, the residual add (and under TP the all-reduce hook ``reduce``) in the proj epilogue. Without
        them this is the reference forward. ``kv_slot``: the slot of a batch KV cache (``set_kv_cache(batch_size >
        1)``) this B = 1 call reads and writes."""
        B, T, C = x.size()
        c = self.config
        H, G, hs = c.n_head, c.n_query_groups, c.head_size
        qkv = _lin(self.attn, x, norm_weight=None if norm is None else norm.weight,
                   norm_eps=c.norm_eps if norm is None else norm.eps).view(T, -1)
        dev = x.device
        if input_pos is None:
            # no cache (training-style causal forward, model.py:510-513): a private cache of T rows
            pos = rope_pos = torch.arange(T, device=dev, dtype=torch.int64)
            kc = torch.empty(G, T, hs, dtype=qkv.dtype, device=dev)  # bf16, or fp32 under --precision 32-true
            cache = (kc, torch.empty_like(kc))
        else:
            if not isinstance(self.kv_cache, KVCache):
                raise TypeError("You need to call `gpt.set_kv_cache()`")
            if not 0 <= kv_slot < self.kv_cache.k.size(0):
                raise ValueError(f"kv_slot {kv_slot}: the KV cache holds {self.kv_cache.k.size(0)} sequence(s)")
            cache = self._cache(qkv.dtype, kv_slot)
            pos = input_pos
            # callers may pass the full cos/sin tables (our GPT.forward) or rows pre-selected by input_pos (the
            # reference's GPT.forward, model.py:505-506)
            rope_pos = pos if (cos.size(0) != T or T == cache[0].size(-2)) else torch.arange(T, device=dev)
        y = self._attend(qkv, cache, pos, rope_pos, cos, sin)
        out = _lin(self.proj, y.view(1, T, H * hs), residual=residual, reduce=reduce)
        return out.view(B, T, -1)

    def _cache(self, dtype: torch.dtype, slot: Optional[int] = None):
        """The KV cache as the ops take it, of sequence ``slot`` or (None) of all slots: (k, v), cast to the activation
        ``dtype`` as the reference's KVCache.forward does (:790-791), or (k codes, v codes, k scales, v scales)."""
        kv = self.kv_cache
        if kv.fp8:
            whole = (kv.k, kv.v, kv.k_scale, kv.v_scale)
        else:
            if kv.k.dtype != dtype:
                kv.k, kv.v = kv.k.to(dtype), kv.v.to(dtype)
            whole = (kv.k, kv.v)
        return whole if slot is None else tuple(t[slot] for t in whole)

    def _decode_setup(self, qkv, cache, cos, sin, split=True):
        """What every attention call on decode rows needs: the fp32 contiguous rope tables, the split count of the
        one-row step on this cache length (the bits of y depend on it) and the split workspace for qkv's row count.
        One ``AttentionWorkspace`` per row count serves every form (one row, window, batch) and both cache formats:
        all launches are serial on one stream and the last-arriving workgroup of each re-arms the counters, so a
        launch always finds them as the constructor left them."""
        c = self.config
        H, G, hs = c.n_head, c.n_query_groups, c.head_size
        rows, dev = qkv.size(0), qkv.device
        cos = cos.to(device=dev, dtype=torch.float32).contiguous()
        sin = sin.to(device=dev, dtype=torch.float32).contiguous()
        if not split:
            return cos, sin, 1, None
        n_splits = ops.decode_splits(G, H // G, hs, cache[0].size(-2))
        wss = self.__dict__.setdefault("_decode_ws", {})
        ws = wss.get(rows)
        if ws is None or ws.key != (rows, H, G, hs, n_splits) or ws.counters.device != dev:
            ws = wss[rows] = ops.AttentionWorkspace(rows, H, G, hs, n_splits, dev)
        return cos, sin, n_splits, ws

    def _decode_attention(self, form, qkv, cache, pos, rope_pos, cos, sin, active=None, out=None,
                          prefix_len=None) -> torch.Tensor:
        """RoPE + KV-append + split decode attention of the rows of ``qkv`` in one launch of the form ``form`` ("fused",
        "window", "batch" or "shared", the last behind ``prefix_len``: ``ops._attention_decode``)
        over ``cache`` (``_cache``) -> (rows, H * hs)."""
        c = self.config
        cos, sin, n_splits, ws = self._decode_setup(qkv, cache, cos, sin)
        return ops._attention_decode(form, qkv, cache, pos, rope_pos, cos, sin, c.n_head, c.n_query_groups, c.head_size,
                                     c.rope_n_elem, 1.0 / math.sqrt(c.head_size), n_splits, ws, out, active, prefix_len)

    def _attend(self, qkv, cache, pos, rope_pos, cos, sin, out=None) -> torch.Tensor:
        """RoPE + KV-append + causal attention of the T rows of ``qkv`` over one sequence's ``cache`` -> (T, H * hs)."""
        c = self.config
        H, G, hs = c.n_head, c.n_query_groups, c.head_size
        if len(cache) == 4:
            return self._attend_kv8(qkv, cache, pos, rope_pos, cos, sin, out)
        decode = qkv.size(0) == 1 and qkv.dtype == torch.bfloat16
        if decode and self.fuse_decode and ops.decode_fusable(hs, c.rope_n_elem):
            # decode token: RoPE + KV-append + attention in a single launch
            return self._decode_attention("fused", qkv, cache, pos, rope_pos, cos, sin, out=out)
        cos, sin, n_splits, ws = self._decode_setup(qkv, cache, cos, sin, split=decode)
        q = ops.rope_kv_append(qkv, *cache, pos, rope_pos, cos, sin, H, G, hs, c.rope_n_elem)
        return ops.attention(q, *cache, pos, H, G, hs, 1.0 / math.sqrt(hs), n_splits, workspace=ws, out=out)

    def _attend_kv8(self, qkv, cache, pos, rope_pos, cos, sin, out=None) -> torch.Tensor:
        """``_attend`` over one sequence's fp8 cache. Every row is scored as the cache holds it, the call's own rows
        included. T = 1: quantizing append + attention in one launch. T > 1: the quantizing append, the cache expanded
        into the model's bf16 scratch pair, then the bf16 prefill attention over that (no host read of ``pos``:
        graph-safe)."""
        c = self.config
        H, G, hs = c.n_head, c.n_query_groups, c.head_size
        if qkv.dtype != torch.bfloat16:
            raise NotImplementedError(f"an fp8 KV cache with {qkv.dtype} activations: the kernels take bf16")
        if qkv.size(0) == 1:
            return self._decode_attention("fused", qkv, cache, pos, rope_pos, cos, sin, out=out)
        dev = qkv.device
        cos, sin, _, _ = self._decode_setup(qkv, cache, cos, sin, split=False)
        q = ops.kv8_rope_append(qkv, cache, pos, rope_pos, cos, sin, H, G, hs, c.rope_n_elem)
        kv = self.kv_cache
        if kv.scratch is None or kv.scratch[0].shape != cache[0].shape or kv.scratch[0].device != dev:
            kv.scratch = tuple(torch.empty(cache[0].shape, dtype=torch.bfloat16, device=dev) for _ in range(2))
        kd, vd = ops.kv8_dequantize(cache, out=kv.scratch)
        return ops.attention(q, kd, vd, pos, H, G, hs, 1.0 / math.sqrt(hs), 1, out=out)

    def batch_fusable(self, dtype: torch.dtype) -> bool:
        """Whether ``ops.attention_decode_batch`` covers this module: the fused decode form's geometry, bf16."""
        c = self.config
        return (self.fuse_decode and ops.decode_fusable(c.head_size, c.rope_n_elem)
                and c.n_head // c.n_query_groups in (1, 2, 4, 8) and dtype == torch.bfloat16)

    def decode_rows(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, *,
                    norm: "RMSNorm", residual: torch.Tensor, active: Optional[torch.Tensor] = None,
                    shared_prefix: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Batched decode step: x (B, C), one token of each of B sequences at ``pos`` (B,). The qkv and the
        out-projection run once for all rows (multi-row GEMVs); attention cannot share anything across sequences
        (each has its own K / V): on the fused decode form's geometry it is ONE ``ops.attention_decode_batch`` launch
        whose row b is the one-sequence launch on row b of qkv and cache slot b (``batch_attention``; the split count
        is the one-sequence step's, the bits of y depend on it), otherwise the one-sequence decode attention once per
        sequence, all through the one ``AttentionWorkspace`` (serial launches; its counters re-arm). ``active`` (B,)
        int32 marks idle rows (0): their cache slot is untouched and their y is zero — the batch launch only.
        ``shared_prefix`` (1,) int64 on the device: the rows are samples of one prompt at the ONE position ``pos`` (1,),
        and attention is ONE ``ops.attention_decode_shared`` launch that reads the keys below that length from slot 0
        for all rows; bf16 cache and the batch launch's geometry only (``GPT._shared_check``)."""
        B = x.size(0)
        qkv = _lin(self.attn, x, norm_weight=norm.weight, norm_eps=norm.eps, rows=True)
        fusable = self.batch_fusable(qkv.dtype)
        if shared_prefix is not None:
            if not fusable or self.kv_cache.fp8:
                raise NotImplementedError("a shared prompt prefix needs the bf16 cache and the batched decode "
                                          "attention's geometry")
            y = self._decode_attention("shared", qkv, self._cache(qkv.dtype), pos, pos, cos, sin, active=active,
                                       prefix_len=shared_prefix)
            return _lin(self.proj, y, residual=residual, rows=True)
        if active is not None and not fusable:
            raise NotImplementedError("idle rows (active) need the batched decode attention launch: head_size == "
                                      "rope_n_elem == 128, 1 / 2 / 4 / 8 heads per query group, bf16 activations")
        if fusable and (batch_attention or active is not None):
            y = self._decode_attention("batch", qkv, self._cache(qkv.dtype), pos, pos, cos, sin, active=active)
        else:
            y = torch.empty(B, self.config.n_head * self.config.head_size, dtype=qkv.dtype, device=qkv.device)
            for b in range(B):
                p = pos[b:b + 1]
                self._attend(qkv[b:b + 1], self._cache(qkv.dtype, b), p, p, cos, sin, out=y[b:b + 1])
        return _lin(self.proj, y, residual=residual, rows=True)

    def decode_window(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos0: torch.Tensor, *,
                      norm: "RMSNorm", residual: torch.Tensor) -> torch.Tensor:
        """Speculative verify window: x (M, C), M consecutive tokens of the sequence in cache slot 0 from ``pos0``
        (1,). The qkv and the out-projection are the multi-row GEMVs; the M rows read one K / V, so attention is ONE
        ``ops.attention_decode_window`` call with the split count of the one-row step (``ops.decode_splits`` of the
        cache length: the bits of y depend on it, so the cache must be as long as the one ``generate`` would use)."""
        qkv = _lin(self.attn, x, norm_weight=norm.weight, norm_eps=norm.eps, rows=True)
        y = self._decode_attention("window", qkv, self._cache(qkv.dtype, 0), pos0, None, cos, sin)
        return _lin(self.proj, y, residual=residual, rows=True)

    def scaled_dot_product_attention(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                     mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Reference-compatible helper (model.py:658-665); the fused path uses ``ops.attention`` instead."""
        scale = 1.0 / math.sqrt(self.config.head_size)
        y = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, scale=scale,
                                                             is_causal=mask is None)
        return y.transpose(1, 2)

    def build_kv_cache(self, batch_size: int, max_seq_length: int, rope_cache_length: Optional[int] = None,
                       device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None) -> "KVCache":
        heads = self.config.n_query_groups  # un-expanded groups (the reference stores n_head, model.py:675)
        v_shape = (batch_size, heads, max_seq_length, self.config.head_size)
        if rope_cache_length is None:
            if self.config.rotary_percentage != 1.0:
                raise TypeError("Please pass the `rope_cache_length=gpt.cos.size(-1)` value")
            k_shape = v_shape
        else:
            k_shape = (batch_size, heads, max_seq_length,
                       rope_cache_length + self.config.head_size - self.config.rope_n_elem)
        if device is None:
            device = self.attn.weight.device
        return KVCache(k_shape, v_shape, device=device, dtype=dtype or torch.bfloat16)


class GptNeoxMLP(nn.Module):
    """GPT-NeoX / pythia MLP (reference model.py:691-702): fc (+bias) -> GELU -> proj (+bias). The Linears run the
    GEMV / GEMM kernels (4-bit or bf16), the activation ``lga_gelu`` (exact erf, or tanh per
    ``config.gelu_approximate``) with the reference's bf16 rounding points."""

    def __init__(self, config: Config) -> None:
        super().__init__()
        self.fc = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.proj = nn.Linear(config.intermediate_size, config.n_embd, bias=config.bias)
        self.config = config

    def forward(self, x: torch.Tensor, *, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``residual`` fuses an add into the proj epilogue (bf16(bf16(proj(x)) + residual)); Block uses it for the
        parallel residual's ``mlp(n_2) + h``."""
        if not x.is_cuda:
            _gpu_only("GptNeoxMLP")
        h = _lin(self.fc, x)
        h = ops.gelu(h.contiguous(), self.config.gelu_approximate)
        return _lin(self.proj, h, residual=residual)


class LLaMAMLP(nn.Module):
    def __init__(self, config: Config) -> None:
        super().__init__()
        self.fc_1 = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.fc_2 = nn.Linear(config.n_embd, config.intermediate_size, bias=config.bias)
        self.proj = nn.Linear(config.intermediate_size, config.n_embd, bias=config.bias)

    def forward(self, x: torch.Tensor, *, norm: Optional["RMSNorm"] = None,
                residual: Optional[torch.Tensor] = None, reduce=None) -> torch.Tensor:
        """proj(silu(fc_1 x) * fc_2 x) (model.py:712-716); ``norm``/``residual``/``reduce`` are Block fusion hooks
        (``reduce``: the TP all-reduce of the row-parallel proj, see CausalSelfAttention.forward)."""
        lead, C = x.shape[:-1], x.shape[-1]
        g = quantize.swiglu(self.fc_1, self.fc_2, x.reshape(-1, C).contiguous(), norm)
        out = _lin(self.proj, g, residual=residual, reduce=reduce)
        return out.view(*lead, -1)


# batched decode step: one ops.attention_decode_batch launch per block for all B sequences; False (LGA_BATCH_ATTN=0)
# keeps the one-sequence decode attention once per sequence (bit-identical; tools/batch_decode.py and the tests A/B
# the two). A step with idle rows (``active``) always takes the batch launch.
batch_attention = os.environ.get("LGA_BATCH_ATTN", "1") != "0"

# decode routing through the fused gate + route launch (lga_moe_gate_route); False keeps lga_q4_gemv + lga_moe_route
# (tests A/B the two)
moe_gate_route = True
# one-token sparse-MoE: the routed proj GEMVs of both slots + the combine + residual in one launch whose second-arriving
# workgroup per row block combines (lga_q4_gemv_experts_pair_combine, bit-identical to the two launches); False keeps
# lga_q4_gemv_experts + lga_moe_combine
moe_pair_combine = os.environ.get("LGA_MOE_PAIR_COMBINE", "1") != "0"


class LLaMAMoE(nn.Module):
    """Sparse MoE (lit_gpt/model.py:719-743): router gate, top-k experts per token, prob-weighted bf16 sum.

    Decode (one token) never leaves the device: ``lga_moe_route`` picks the experts, the routed GEMVs stream
    only the k selected experts' weights (``lga_q4_gemv_swiglu_experts`` with the fused norm_2, then
    ``lga_q4_gemv_experts``), ``lga_moe_combine`` adds them in ascending expert order plus the Block residual.
    Prefill (T > 1) groups the (token, slot) pairs per expert on the device (``lga_moe_group``: the reference's
    ``torch.where`` loop as a stable counting sort and a tile table) and runs all experts in two grouped MFMA GEMM
    launches (fc_1||fc_2 + SwiGLU, proj); shapes the grouped kernel does not take fall back to the per-expert loop. Forward hooks registered on the experts (``generate/tp.py`` registers the TP
    all-reduce on each expert, tp.py:58-62) are applied to the stacked (T, k, C) expert outputs: a per-element
    sum over ranks, identical to reducing every expert call separately.

    Experts are 4-bit ``QuantLinear`` modules everywhere generation goes (every kernel named above streams packed
    weights; ``Block.forward`` refuses a KV-cache forward otherwise). The one exception is scoring an unquantized model
    (lit_gpt/score.py): with ``nn.Linear`` bf16 experts a multi-row input (T > 1) takes the per-expert loop on the bf16
    GEMM kernels; a single row still raises.
    """

    def __init__(self, config: Config) -> None:
        super().__init__()
        self.gate = nn.Linear(config.n_embd, config.n_expert, bias=False)
        self.experts = nn.ModuleList(LLaMAMLP(config) for _ in range(config.n_expert))
        self.config = config
        self._stacks = None

    def _stack(self):
        """Stack the experts' packed weights per Linear ((E, N, K/2) / (E, N, K/group)) and re-point every
        expert's buffers at its slice, so the routed GEMVs and the grouped GEMMs index experts with one stride
        (done once: ``build_model`` calls it right after quantizing the block, so the first prompt does not pay the
        copy — 32 ms of Mixtral-8x7B's cold prefill in round 4)."""
        if self._stacks is not None and self._stacks[0][0].data_ptr() == self.experts[0].fc_1.qweight.data_ptr():
            return self._stacks
        out = []
        for name in ("fc_1", "fc_2", "proj"):
            lins = [getattr(e, name) for e in self.experts]
            l0 = lins[0]
            if not all(isinstance(l, quantize.QuantLinear) and l.bias is None and (l.fmt, l.group, l.qweight.shape) ==
                       (l0.fmt, l0.group, l0.qweight.shape) for l in lins):
                raise NotImplementedError("LLaMAMoE on the MI355X needs bias-free QuantLinear experts of one format")
            qw = torch.stack([l.qweight for l in lins])
            sc = torch.stack([l.scales for l in lins])
            for i, l in enumerate(lins):
                l.qweight, l.scales = qw[i], sc[i]
            out.append((qw, sc))
        self._stacks = out
        return out

    def _grouped_ok(self, C: int) -> bool:
        """The grouped prefill GEMMs take 4-bit experts whose shapes the fused MFMA kernel covers (else the loop)."""
        f1, pj = self.experts[0].fc_1, self.experts[0].proj  # (4-bit: _stack has checked)
        return bool(ops.q4f_fits(64, f1.out_features, C, f1.group, f1.fmt)
                    and ops.q4f_fits(64, pj.out_features, pj.in_features, pj.group, pj.fmt))

    def _gate_route_ok(self, C: int) -> bool:
        """One-token routing through ``lga_moe_gate_route``: a bias-free 4-bit gate without forward hooks (the
        reference's TP keeps the gate replicated and hook-free, generate/tp.py:58-62) whose shape the kernel takes."""
        g = self.gate
        return (moe_gate_route and isinstance(g, quantize.QuantLinear) and g.bias is None and not g._forward_hooks
                and g.in_features == C and ops.moe_gate_route_fits(g.out_features, C))

    def _expert_hooks(self, x: torch.Tensor, eout: torch.Tensor) -> torch.Tensor:
        hooks = [list(e._forward_hooks.values()) for e in self.experts]
        if any(len(h) != len(hooks[0]) for h in hooks):
            raise NotImplementedError("LLaMAMoE: experts carry different forward hooks")
        for hook in hooks[0]:
            r = hook(self.experts[0], (x,), eout)
            eout = eout if r is None else r
        return eout

    def forward(self, x: torch.Tensor, *, norm: Optional["RMSNorm"] = None,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``norm`` / ``residual``: Block fusion hooks (norm_2 in the gate / fc GEMV prologues, the residual in the
        combine)."""
        c = self.config
        lead, C = x.shape[:-1], x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        T, k, E = x2.size(0), c.n_expert_per_token, c.n_expert
        f1, pj = self.experts[0].fc_1, self.experts[0].proj
        # unquantized (bf16 nn.Linear) experts: multi-row inputs only, through the per-expert loop below — what
        # scoring a bf16 model needs (lit_gpt/score.py); the one-token decode kernels stream 4-bit experts
        plain = T > 1 and all(isinstance(l, nn.Linear) for ex in self.experts for l in (ex.fc_1, ex.fc_2, ex.proj))
        if not plain:
            (q1, s1), (q2, s2), (qp, sp) = self._stack()
        res = None if residual is None else residual.reshape(T, C).contiguous()
        if T == 1:
            fuse_norm = norm is not None and f1.gemv_fuses_norm(dual=True)
            xin = x2 if (norm is None or fuse_norm) else norm(x2)
            nw = norm.weight if fuse_norm else None
            eps = norm.eps if fuse_norm else 1e-5
            if self._gate_route_ok(C):  # gate GEMV + routing in one launch (same bits as the pair below)
                g = self.gate
                ids, probs = ops.moe_gate_route(xin.view(-1), g.qweight, g.scales, E, C, g.group, g.fmt, k,
                                                norm_weight=nw, eps=eps)
            else:
                router = _lin(self.gate, xin, norm_weight=nw, norm_eps=eps).view(1, E)
                ids, probs = ops.moe_route(router, k)
            act = ops.q4_gemv_swiglu_experts(xin.view(-1), q1, s1, q2, s2, ids.view(-1), f1.out_features, C,
                                             f1.group, f1.fmt, norm_weight=nw, eps=eps)
            if (moe_pair_combine and res is not None and k == 2 and not any(e._forward_hooks for e in self.experts)
                    and ops.experts_pair_supported(pj.out_features, pj.in_features, pj.group, pj.fmt)):
                pw = getattr(self, "_pair_ws", None)
                if pw is None or pw.scratch.numel() != 2 * pj.out_features or pw.scratch.device != act.device:
                    pw = self._pair_ws = ops.ExpertsPairWorkspace(pj.out_features, act.device)
                return ops.q4_gemv_experts_pair_combine(act, qp, sp, ids.view(-1), probs.view(-1), res.view(-1),
                                                        pj.out_features, pj.in_features, pj.group, pj.fmt,
                                                        pw).view(*lead, C)
            eout = ops.q4_gemv_experts(act, qp, sp, ids.view(-1), pj.out_features, pj.in_features, pj.group,
                                       pj.fmt).view(1, k, C)
        else:
            n = x2 if norm is None else norm(x2)
            router = _lin(self.gate, n)
            ids, probs = ops.moe_route(router.contiguous(), k)
            if not plain and self._grouped_ok(C):
                # the reference's per-expert token groups (model.py:740-742) as two grouped launches over a
                # device-built tile table: no torch.where host sync, no gathered / scattered copies
                rows, bm = T * k, ops.moe_grouped_bm(T * k)
                tiles, x_rows, y_rows = ops.moe_group(ids, E, bm)
                g = ops.q4_gemm_swiglu_grouped(n.contiguous(), q1, s1, q2, s2, tiles, x_rows, rows,
                                               f1.out_features, C, f1.group, f1.fmt, bm, E)
                eout = ops.q4_gemm_grouped(g, qp, sp, tiles, y_rows, rows, pj.out_features, pj.in_features,
                                           pj.group, pj.fmt, bm, E).view(T, k, C)
            else:
                eout = torch.empty(T, k, C, dtype=torch.bfloat16, device=x2.device)
                for e in range(E):  # the reference's per-expert token groups (model.py:740-742)
                    tok, slot = torch.where(ids == e)
                    if tok.numel() == 0:
                        continue
                    xe = n.index_select(0, tok)
                    ex = self.experts[e]
                    g = ops.swiglu(_lin(ex.fc_1, xe).contiguous(), _lin(ex.fc_2, xe).contiguous())
                    eout[tok, slot] = _lin(ex.proj, g)
        eout = self._expert_hooks(x2, eout)
        return ops.moe_combine(eout.contiguous(), probs, ids, residual=res).view(*lead, C)


class LayerNorm(nn.LayerNorm):
    """config.norm_class for GPT-NeoX (reference config.py:137-144: torch.nn.LayerNorm) on the ``lga_layernorm``
    kernel: same parameters (weight, bias) and state-dict names, fp32 statistics, one bf16 cast."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            _gpu_only("LayerNorm")
        dt = torch.float32 if x.dtype == torch.float32 else torch.bfloat16  # 32-true or bf16-true
        w = self.weight.to(dt) if self.weight.dtype != dt else self.weight
        b = None if self.bias is None else (self.bias.to(dt) if self.bias.dtype != dt else self.bias)
        return ops.layernorm(x.contiguous(), w, b, self.eps)


class KVCache(nn.Module):
    """``k`` / ``v`` (B, G, S, hs) in ``dtype``, or the fp8 form for ``dtype=torch.float8_e4m3fn``:
    ``k`` / ``v`` hold OCP e4m3 codes as uint8 (no torch fp8 operator runs on the device) and ``k_scale`` / ``v_scale``
    (B, G, S) fp32 one power-of-two scale per row — 132 B per row of 128 instead of 256. ``cache_dtype`` names the
    format (``k.dtype`` is uint8 for an fp8 cache)."""

    def __init__(self, k_shape: Tuple[int, int, int, int], v_shape: Tuple[int, int, int, int],
                 device: Optional[torch.device] = None, dtype: Optional[torch.dtype] = None) -> None:
        super().__init__()
        self.cache_dtype = dtype if dtype is not None else torch.get_default_dtype()
        self.scratch = None  # fp8: the bf16 (G, S, hs) pair of the cached prefill (GPT.set_kv_cache shares one)
        if self.fp8:
            if tuple(k_shape) != tuple(v_shape):
                raise NotImplementedError("an fp8 KV cache holds full-rotary keys: k and v rows of one size")
            self.register_buffer("k", torch.zeros(k_shape, device=device, dtype=torch.uint8), persistent=False)
            self.register_buffer("v", torch.zeros(v_shape, device=device, dtype=torch.uint8), persistent=False)
            self.register_buffer("k_scale", torch.ones(k_shape[:3], device=device, dtype=torch.float32),
                                 persistent=False)
            self.register_buffer("v_scale", torch.ones(v_shape[:3], device=device, dtype=torch.float32),
                                 persistent=False)
            return
        self.register_buffer("k", torch.zeros(k_shape, device=device, dtype=dtype), persistent=False)
        self.register_buffer("v", torch.zeros(v_shape, device=device, dtype=dtype), persistent=False)

    @property
    def fp8(self) -> bool:
        return self.cache_dtype == torch.float8_e4m3fn

    def slot(self, b: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """One sequence of an fp8 cache as the ops take it: (k codes, v codes, k scales, v scales)."""
        return self.k[b], self.v[b], self.k_scale[b], self.v_scale[b]

    def dequantized(self, slot: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """bf16 (k, v), each (G, S, hs), of one sequence of an fp8 cache: float(code) * scale, exact (tests, debugging)."""
        if not self.fp8:
            raise TypeError("dequantized() reads an fp8 KV cache")
        if self.k.is_cuda:
            return ops.kv8_dequantize(self.slot(slot))
        kc, vc, ks, vs = self.slot(slot)
        return tuple((c.view(torch.float8_e4m3fn).float() * s.unsqueeze(-1)).to(torch.bfloat16)
                     for c, s in ((kc, ks), (vc, vs)))

    def forward(self, input_pos: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Reference API (model.py:788-795); the fused path writes the cache inside ``lga_rope_kv_append``."""
        if self.fp8:
            raise NotImplementedError("an fp8 KV cache is written by the quantizing kernels (ops.kv8_rope_append, "
                                      "ops.attention_decode_fused_kv8), not through the reference's index_copy_")
        self.k = self.k.to(k.dtype)
        self.v = self.v.to(v.dtype)
        return self.k.index_copy_(2, input_pos, k), self.v.index_copy_(2, input_pos, v)

    def reset_parameters(self) -> None:
        torch.nn.init.zeros_(self.k)
        torch.nn.init.zeros_(self.v)
        if self.fp8:
            torch.nn.init.ones_(self.k_scale)
            torch.nn.init.ones_(self.v_scale)


def build_rope_cache(seq_len: int, n_elem: int, device: Optional[torch.device] = None, base: int = 10000,
                     condense_ratio: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin tables (seq_len, n_elem) in fp32 (model.py:746-764).

    The positions are a true division of an integer range, so (as in the reference) they take the DEFAULT dtype:
    under a bf16 default — the reference's ``fabric.init_tensor()`` with bf16-true / bnb precision around
    ``model.max_seq_length = ...`` (generate/base.py:153-157, generate/tp.py) — positions above 256 round to bf16
    before the fp32 outer product. ``generate.base.build_model(rope_positions=...)`` chooses that context.

    The tables are computed on the CPU (as the reference's CPU run computes them) and then moved to ``device``: the
    GPU's fp32 cos / sin of angles in the thousands of radians differ from the CPU's by up to ~1.6e-3 (measured at
    the 4k-32k rows of tests/golden/g5_rope_long.npz), the CPU's are the reference's values bit for bit."""
    inv_freq = torch.arange(0, n_elem, 2).float().div(n_elem)
    theta = 1.0 / torch.pow(float(base), inv_freq)
    positions = torch.arange(seq_len).div(condense_ratio)  # default dtype, see above
    angles = torch.outer(positions, theta).repeat(1, 2)
    cos, sin = torch.cos(angles), torch.sin(angles)
    return (cos, sin) if device is None else (cos.to(device), sin.to(device))


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Reference helper (model.py:767-773); the hot path applies RoPE inside ``lga_rope_kv_append``."""
    half = x.size(-1) // 2
    rotated = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    return ((x * cos) + (rotated * sin)).to(dtype=x.dtype)


def build_mask_cache(max_seq_length: int, device: Optional[torch.device] = None) -> torch.Tensor:
    ones = torch.ones((max_seq_length, max_seq_length), device=device, dtype=torch.bool)
    return torch.tril(ones).unsqueeze(0).unsqueeze(0)


class CausalMask:
    """``GPT.mask_cache`` without the (1, 1, S, S) bool tensor (reference model.py:551-554,802-804 build it in
    ``set_kv_cache``): no kernel reads it — attention derives the mask row from ``input_pos`` — and at Mixtral's
    S = 32768 it would hold 1 GiB of HBM per rank. It keeps the reference's shape for ``size()`` / ``shape`` and
    materialises the tril tensor only if a caller indexes it (``mask_cache.index_select(2, input_pos)`` style)."""

    def __init__(self, max_seq_length: int, device: Optional[torch.device] = None) -> None:
        self.max_seq_length = max_seq_length
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self._t: Optional[torch.Tensor] = None

    @property
    def shape(self) -> torch.Size:
        return torch.Size((1, 1, self.max_seq_length, self.max_seq_length))

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self.shape[dim]

    def tensor(self) -> torch.Tensor:
        if self._t is None:
            self._t = build_mask_cache(self.max_seq_length, self.device)
        return self._t

    def __getitem__(self, item):
        return self.tensor()[item]

    def index_select(self, dim: int, index: torch.Tensor) -> torch.Tensor:
        return self.tensor().index_select(dim, index)
