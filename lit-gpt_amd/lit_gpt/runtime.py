"""Decode-step executor: one HIP graph per decode step (greedy, or top-k sampling at temperature > 0).

The reference gets launch-overhead relief from ``torch.compile(next_token, mode="reduce-overhead")``
(generate/base.py:161-166), i.e. CUDA graphs over Inductor/Triton kernels. Here the step is already a short
chain of hand-written HIP kernels (per layer: fused RMSNorm+qkv GEMV, RoPE+KV append, split attention +
combine, proj GEMV+residual, fused RMSNorm+SwiGLU GEMV, down GEMV+residual; then RMSNorm+lm_head GEMV and
argmax). ``DecodeGraph`` captures that chain once with static input buffers — the token id and ``input_pos``
live on the device, the argmax kernel writes the next token, advances ``input_pos`` and gathers the token's
embedding row for the next step (so the step has no embedding launch) — so a decode step is a single
``hipGraphLaunch`` with no host<->device synchronisation (or, with ``chunk``, several steps are).
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from lit_gpt import ops, quantize


def _sampling_ok(temperature: float, top_k: Optional[int], top_p: float) -> bool:
    """The device samplers' settings: top_k in [1, 1024] (ops.sample_topk), or, with 0 < top_p < 1, top_k in
    [1, 1024] or None (ops.sample_nucleus)."""
    if not 0.0 < top_p <= 1.0:
        return False
    if top_k is None:
        return top_p < 1.0
    return 1 <= top_k <= ops.MAX_TOP_K

class DecodeGraph:
    def __init__(self, model, first_token: torch.Tensor, first_pos: int, chunk: int = 1, *,
                 temperature: float = 0.0, top_k: Optional[int] = None, rng=None, top_p: float = 1.0) -> None:
        """Runs one real decode step eagerly (token ``first_token`` at position ``first_pos``) to warm up, then
        captures the step. Afterwards ``self.token`` holds the newest token and ``self.pos`` its position.
        ``chunk`` > 1 also captures ``chunk`` consecutive steps as one graph (``steps()``): the argmax of step i
        writes its token into ``self.history[i]`` as well, and one launch replaces ``chunk`` (≈9 us of
        graph-launch gap per step on MI355X, profiles/r02b_*). ``temperature`` > 0 replaces the argmax with the
        fused top-k sampler (ops.sample_topk, ``top_k`` 1..1024, RNG state ``rng``: generate.base.SamplerRNG), or,
        with ``top_p`` < 1, with the nucleus sampler (ops.sample_nucleus, ``top_k`` 1..1024 or None)."""
        dev = first_token.device
        self.model = model
        self.temperature, self.top_k, self.rng, self.top_p = float(temperature), top_k, rng, float(top_p)
        if self.temperature > 0.0 and (rng is None or not _sampling_ok(self.temperature, top_k, self.top_p)):
            raise ValueError("DecodeGraph: sampling needs top_k in [1, 1024] and an rng (generate.base.SamplerRNG)"
                             "; top_k may be None only with 0 < top_p < 1")
        self.token = first_token.reshape(1, 1).to(torch.int32).clone()
        self.pos = torch.tensor([first_pos], dtype=torch.int64, device=dev)
        self.chunk = max(1, int(chunk))
        self.history = torch.zeros(self.chunk, dtype=torch.int64, device=dev)
        # the argmax launch also gathers the new token's embedding row (ops.argmax_embed) into x_emb, which the
        # next step's forward takes instead of running its own embedding launch
        wte = model.transformer.wte.weight
        self.fuse_embedding = (wte.is_cuda and wte.dtype == torch.bfloat16 and wte.is_contiguous()
                               and wte.shape[1] % 8 == 0)
        self.x_emb = torch.empty(wte.shape[1], dtype=torch.bfloat16, device=dev) if self.fuse_embedding else None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.chunk_graph: Optional[torch.cuda.CUDAGraph] = None
        self._step_eager()
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_body()
        self.graph = g
        if self.chunk > 1:
            gc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc):
                for i in range(self.chunk):
                    self._step_body(self.history[i:i + 1])
            self.chunk_graph = gc

    # greedy steps run ln_f + lm_head + argmax + the next embedding row as ONE launch (ops.q4_gemv_argmax_embed)
    # where the head is a 4-bit Linear it covers; False keeps lm_head GEMV + argmax_embed (bit-identical)
    fuse_head = os.environ.get("LGA_FUSE_HEAD", "1") != "0"

    def _step_body(self, idx_out: Optional[torch.Tensor] = None, embedded: bool = True) -> None:
        fuse = self.fuse_embedding
        model = self.model
        ln = model.transformer.ln_f
        if (self.temperature == 0.0 and fuse and self.fuse_head and quantize.head_argmax_supported(model.lm_head)
                and type(ln).__name__ == "RMSNorm" and not model.lm_head._forward_hooks):
            h = model(self.token, self.pos, last_token_only=True, embedded=self.x_emb if embedded else None,
                      hidden_only=True).reshape(-1)
            if getattr(self, "_head_ws", None) is None:
                self._head_ws = ops.HeadWorkspace(model.lm_head.out_features, model.lm_head.in_features, h.device)
                self.logits = torch.empty(model.lm_head.out_features, dtype=torch.bfloat16, device=h.device)
            ops.q4_gemv_argmax_embed(h, model.lm_head, self._head_ws, norm_weight=ln.weight, eps=ln.eps,
                                     table=model.transformer.wte.weight, emb_out=self.x_emb, logits=self.logits,
                                     out_idx=idx_out, token_out=self.token.view(-1), pos_inout=self.pos)
            return
        logits = model(self.token, self.pos, last_token_only=True,
                       embedded=self.x_emb if (fuse and embedded) else None).reshape(-1)
        table = model.transformer.wte.weight if fuse else None
        if self.temperature > 0.0 and self.top_p < 1.0:
            ops.sample_nucleus(logits, self.top_k, self.top_p, self.temperature, seed=self.rng.seed,
                               counter=self.rng.counter, out_idx=idx_out, token_out=self.token.view(-1),
                               pos_inout=self.pos, table=table, emb_out=self.x_emb)
        elif self.temperature > 0.0:
            ops.sample_topk(logits, self.top_k, self.temperature, seed=self.rng.seed, counter=self.rng.counter,
                            out_idx=idx_out, token_out=self.token.view(-1), pos_inout=self.pos, table=table,
                            emb_out=self.x_emb)
        elif fuse:
            ops.argmax_embed(logits, table, self.x_emb, out_idx=idx_out, token_out=self.token.view(-1),
                             pos_inout=self.pos)
        else:
            ops.argmax(logits, out_idx=idx_out, token_out=self.token.view(-1), pos_inout=self.pos)

    def _step_eager(self) -> None:
        self._step_body(embedded=False)  # embeds first_token itself; its argmax leaves x_emb for the graphs

    def step(self) -> torch.Tensor:
        """One decode step; returns the (device) token buffer holding the new token."""
        self.graph.replay()
        return self.token

    def steps(self) -> torch.Tensor:
        """``chunk`` decode steps in one graph launch; returns the (device, int64) buffer of their tokens."""
        if self.chunk_graph is None:
            raise RuntimeError("DecodeGraph was built with chunk=1")
        self.chunk_graph.replay()
        return self.history

    def reset(self, token, pos: int) -> None:
        """Re-point the captured step at another (token, position): the next ``step()`` runs ``token`` (an int or a
        one-element tensor) at ``pos`` over whatever the KV cache holds below ``pos``. The static buffers are
        rewritten in place — the token, the position and the ``x_emb`` row the step reads instead of embedding — so
        the graphs stay valid. A speculative draft model is re-pointed this way after a rejection."""
        if torch.is_tensor(token):
            self.token.view(-1).copy_(token.reshape(1))
        else:
            self.token.fill_(int(token))
        self.pos.fill_(int(pos))
        if self.fuse_embedding:
            ops.embedding(self.token.view(-1), self.model.transformer.wte.weight, out=self.x_emb)


class WindowDecodeGraph:
    """The verify step of speculative decoding (generate/speculative.py) for one sequence: device-resident
    ``window`` (MAX_WINDOW,) int32 — ``window[0]`` the last emitted token, ``window[1:M]`` the drafts — and ``pos``
    (1,), the position of ``window[0]``. A step over M = 1 + len(drafts) rows is embedding -> ``GPT.decode_window`` ->
    ``ops.spec_accept``, every launch on one stream: one unbranched HIP graph per M in use, captured lazily (the first
    step at an M runs eagerly and is then captured; the last windows of a run are shorter). ``spec_accept`` leaves
    the accepted count and the emitted tokens in ``out``, writes the last of them to ``window[0]`` and advances
    ``pos``, so the host reads ``out`` once per round and nothing per token. ``use_graph=False`` keeps every step
    eager (tests A/B the two). ``temperature`` > 0 ends the step in ``ops.spec_accept_sample`` instead (``top_k``
    1..1024, RNG state ``rng``: generate.base.SamplerRNG, whose counter is the number of tokens sampled so far): row r
    is sampled with draw number counter + r and a draft is accepted iff it is that sample. ``top_p`` < 1 samples the
    rows with ``ops.spec_accept_sample_nucleus`` (``top_k`` 1..1024 or None)."""

    def __init__(self, model, first_token, first_pos: int, *, use_graph: bool = True, temperature: float = 0.0,
                 top_k: Optional[int] = None, rng=None, top_p: float = 1.0) -> None:
        wte = model.transformer.wte.weight
        dev = wte.device
        if not (wte.is_cuda and wte.dtype == torch.bfloat16 and wte.is_contiguous() and wte.shape[1] % 8 == 0):
            raise NotImplementedError("speculative decoding needs a contiguous bf16 embedding table on the GPU with "
                                      "n_embd % 8 == 0")
        model._rows_check("a speculative verify window")  # refuse before any launch
        self.temperature, self.top_k, self.rng, self.top_p = float(temperature), top_k, rng, float(top_p)
        if self.temperature > 0.0 and (rng is None or not _sampling_ok(self.temperature, top_k, self.top_p)):
            raise ValueError("WindowDecodeGraph: sampling needs top_k in [1, 1024] and an rng "
                             "(generate.base.SamplerRNG); top_k may be None only with 0 < top_p < 1")
        self.model, self.use_graph = model, use_graph
        self.max_rows = model.MAX_WINDOW
        self.window = torch.zeros(self.max_rows, dtype=torch.int32, device=dev)
        self.window[:1].copy_(torch.as_tensor(first_token).reshape(1))
        self.pos = torch.tensor([first_pos], dtype=torch.int64, device=dev)
        self.out = torch.zeros(self.max_rows + 1, dtype=torch.int32, device=dev)
        self.x_emb = torch.empty(self.max_rows, wte.shape[1], dtype=torch.bfloat16, device=dev)
        # the row samples, between spec_accept_sample's two launches
        self.sampled = torch.zeros(self.max_rows, dtype=torch.int32, device=dev) if self.temperature > 0.0 else None
        self.graphs = {}

    def _step_body(self, M: int) -> None:
        model, w = self.model, self.window[:M]
        x = ops.embedding(w, model.transformer.wte.weight, out=self.x_emb[:M])
        logits = model.decode_window(w, self.pos, embedded=x)
        if self.temperature > 0.0 and self.top_p < 1.0:
            ops.spec_accept_sample_nucleus(logits, w, self.top_k, self.top_p, self.temperature, seed=self.rng.seed,
                                           counter=self.rng.counter, out=self.out[:M + 1],
                                           token_inout=self.window[:1], pos_inout=self.pos, sampled=self.sampled)
        elif self.temperature > 0.0:
            ops.spec_accept_sample(logits, w, self.top_k, self.temperature, seed=self.rng.seed,
                                   counter=self.rng.counter, out=self.out[:M + 1], token_inout=self.window[:1],
                                   pos_inout=self.pos, sampled=self.sampled)
        else:
            ops.spec_accept(logits, w, out=self.out[:M + 1], token_inout=self.window[:1], pos_inout=self.pos)

    def step(self, drafts=()):
        """Verify ``drafts`` (a sequence of ints, or an int32 device tensor; at most MAX_WINDOW - 1 of them) after the
        last emitted token. Returns (a, tokens): the number of accepted drafts and the a + 1 tokens this round emits."""
        k = len(drafts)
        M = k + 1
        if M > self.max_rows:
            raise ValueError(f"{k} drafts: a verify window holds at most {self.max_rows - 1}")
        if k:
            d = drafts if torch.is_tensor(drafts) else torch.tensor(list(drafts), dtype=torch.int32)
            self.window[1:M].copy_(d)
        g = self.graphs.get(M)
        if g is not None:
            g.replay()
        else:
            self._step_body(M)
            if self.use_graph:
                torch.cuda.synchronize(self.window.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._step_body(M)
                self.graphs[M] = g
        res = self.out[:M + 1].tolist()  # the round's one device -> host read
        return res[0], res[1:res[0] + 2]


def _assign_adapters(model, adapters, B: int) -> None:
    """Write the adapter ids of the B rows of a batched step (``adapters`` None: no row runs one)."""
    aset = getattr(model, "lora_adapters", None)
    if aset is None:
        if adapters is not None:
            raise ValueError("adapters given, but the model carries no adapter set (lora.attach_many)")
        return
    if adapters is not None and len(adapters) != B:
        raise ValueError(f"{len(adapters)} adapters for {B} sequences")
    for b in range(B):
        aset.assign(b, None if adapters is None else adapters[b])


class BatchDecodeGraph:
    """``DecodeGraph`` for B <= GPT.MAX_BATCH (4) sequences that decode in lock step (generate.base.generate_batch):
    one graph per step over device-resident ``token`` (B,), ``pos`` (B,) and ``x_emb`` (B, C). The step is the batched forward
    (GPT._forward_batch: every weight streamed once for all B rows), then per sequence the same head bookkeeping as
    the single path — ``ops.argmax_embed`` (or ``ops.sample_topk`` with that sequence's RNG) on row b of the logits,
    writing ``token[b]``, advancing ``pos[b]`` and gathering ``x_emb[b]``. Every launch is on one stream, so the
    captured graph is a chain without branches; a step has no host synchronisation. ``chunk`` > 1 also captures
    ``chunk`` steps as one graph whose tokens land in ``history`` (chunk, B)."""

    def __init__(self, model, first_tokens: torch.Tensor, first_pos, chunk: int = 1, *, temperature: float = 0.0,
                 top_k: Optional[int] = None, rngs=None, use_graph: bool = True, top_p: float = 1.0,
                 adapters=None, shared_prefix: Optional[torch.Tensor] = None) -> None:
        """``first_tokens`` (B,): each sequence's newest token; ``first_pos``: its position per sequence. Runs one
        real step eagerly, then captures. ``use_graph=False`` keeps every step eager (tests A/B the two).
        ``shared_prefix`` (1,) int64 on the device: the sequences are samples of one prompt at one position whose keys
        below that length only cache slot 0 holds (``GPT.forward(..., shared_prefix=)``); the step reads ``pos[0]``.
        ``adapters``: per sequence the index of its LoRA adapter in ``model.lora_adapters`` (lora.attach_many) or None,
        written to the set's device-resident row ids before the first step."""
        dev = first_tokens.device
        B = first_tokens.numel()
        _assign_adapters(model, adapters, B)
        self.model, self.B, self.shared_prefix = model, B, shared_prefix
        self.temperature, self.top_k, self.rngs, self.top_p = float(temperature), top_k, rngs, float(top_p)
        if self.temperature > 0.0 and (rngs is None or len(rngs) != B
                                       or not _sampling_ok(self.temperature, top_k, self.top_p)):
            raise ValueError("BatchDecodeGraph: sampling needs top_k in [1, 1024] and one rng per sequence; top_k "
                             "may be None only with 0 < top_p < 1")
        wte = model.transformer.wte.weight
        if not (wte.is_cuda and wte.dtype == torch.bfloat16 and wte.is_contiguous() and wte.shape[1] % 8 == 0):
            raise NotImplementedError("batched decode needs a contiguous bf16 embedding table with n_embd % 8 == 0")
        self.token = first_tokens.reshape(B).to(torch.int32).clone()
        self.pos = torch.as_tensor(first_pos, dtype=torch.int64, device=dev).reshape(B).clone()
        self.x_emb = torch.empty(B, wte.shape[1], dtype=torch.bfloat16, device=dev)
        self.chunk = max(1, int(chunk))
        self.history = torch.zeros(self.chunk, B, dtype=torch.int64, device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.chunk_graph: Optional[torch.cuda.CUDAGraph] = None
        self._step_body(embedded=False)  # embeds first_tokens itself; its head calls leave x_emb for the graphs
        if not use_graph:
            return
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_body()
        self.graph = g
        if self.chunk > 1:
            gc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc):
                for i in range(self.chunk):
                    self._step_body(self.history[i])
            self.chunk_graph = gc

    def _step_body(self, idx_out: Optional[torch.Tensor] = None, embedded: bool = True) -> None:
        model, B = self.model, self.B
        if self.shared_prefix is None:
            logits = model(self.token.view(B, 1), self.pos, embedded=self.x_emb if embedded else None).view(B, -1)
        else:  # the samples advance in lock step: every pos[b] is pos[0]
            logits = model(self.token.view(B, 1), self.pos[:1], embedded=self.x_emb if embedded else None,
                           shared_prefix=self.shared_prefix).view(B, -1)
        table = model.transformer.wte.weight
        for b in range(B):
            out = None if idx_out is None else idx_out[b:b + 1]
            if self.temperature > 0.0 and self.top_p < 1.0:
                ops.sample_nucleus(logits[b], self.top_k, self.top_p, self.temperature, seed=self.rngs[b].seed,
                                   counter=self.rngs[b].counter, out_idx=out, token_out=self.token[b:b + 1],
                                   pos_inout=self.pos[b:b + 1], table=table, emb_out=self.x_emb[b])
            elif self.temperature > 0.0:
                ops.sample_topk(logits[b], self.top_k, self.temperature, seed=self.rngs[b].seed,
                                counter=self.rngs[b].counter, out_idx=out, token_out=self.token[b:b + 1],
                                pos_inout=self.pos[b:b + 1], table=table, emb_out=self.x_emb[b])
            else:
                ops.argmax_embed(logits[b], table, self.x_emb[b], out_idx=out, token_out=self.token[b:b + 1],
                                 pos_inout=self.pos[b:b + 1])

    def step(self) -> torch.Tensor:
        """One decode step of all B sequences; returns the (device, int32) buffer of their new tokens."""
        if self.graph is None:
            self._step_body()
        else:
            self.graph.replay()
        return self.token

    def steps(self) -> torch.Tensor:
        """``chunk`` decode steps in one graph launch; returns the (device, int64) (chunk, B) buffer of tokens."""
        if self.chunk_graph is None:
            raise RuntimeError("BatchDecodeGraph was built with chunk=1 or without graphs")
        self.chunk_graph.replay()
        return self.history


class SlotDecodeGraph:
    """The step executor of continuous batching (generate.base.generate_continuous): ``BatchDecodeGraph`` whose B rows
    are *slots* that sequences enter and leave between launches while the others' state stays on the device.
    Device-resident ``token`` (B,), ``pos`` (B,), ``x_emb`` (B, C) and ``history`` (chunk, B) as there, plus ``active``
    (B,) int32 — an idle slot's attention rows do nothing (``ops.attention_decode_batch``), its cache slot stays as it
    is — and ``uniforms`` (chunk, B) fp32: under sampling, step s samples row b with ``uniforms[s, b]``, which the
    host writes before each launch (``ops.sampler_uniform(seed_b, draws_b + s)``), so a slot's seed changes with its
    sequence without recapturing. One graph for a step and one for ``chunk`` steps, captured once after the first
    launch has run eagerly; every launch is on one stream, the graphs are chains without branches."""

    def __init__(self, model, B: int, chunk: int = 1, *, temperature: float = 0.0, top_k: Optional[int] = None,
                 use_graph: bool = True, top_p: float = 1.0) -> None:
        wte = model.transformer.wte.weight
        dev = wte.device
        if not (wte.is_cuda and wte.dtype == torch.bfloat16 and wte.is_contiguous() and wte.shape[1] % 8 == 0):
            raise NotImplementedError("batched decode needs a contiguous bf16 embedding table with n_embd % 8 == 0")
        self.temperature, self.top_k, self.top_p = float(temperature), top_k, float(top_p)
        if self.temperature > 0.0 and not _sampling_ok(self.temperature, top_k, self.top_p):
            raise ValueError("SlotDecodeGraph: sampling needs top_k in [1, 1024]; top_k may be None only with "
                             "0 < top_p < 1")
        self.model, self.B, self.use_graph = model, B, use_graph
        self.chunk = max(1, int(chunk))
        self.token = torch.zeros(B, dtype=torch.int32, device=dev)
        self.pos = torch.zeros(B, dtype=torch.int64, device=dev)
        self.x_emb = torch.zeros(B, wte.shape[1], dtype=torch.bfloat16, device=dev)
        self.history = torch.zeros(self.chunk, B, dtype=torch.int64, device=dev)
        self.active = torch.zeros(B, dtype=torch.int32, device=dev)
        self.uniforms = torch.full((self.chunk, B), 0.5, dtype=torch.float32, device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.chunk_graph: Optional[torch.cuda.CUDAGraph] = None
        self._captured = False

    def fill(self, b: int, token: torch.Tensor, pos: int, adapter: Optional[int] = None) -> None:
        """Sequence enters slot b: its newest token (a one-element device tensor) at position ``pos``. Stream-ordered
        device writes; the captured graphs read the same buffers. ``adapter``: on a ``lora.attach_many`` model the
        index of the sequence's adapter or None, written to the set's row ids (``release`` leaves it: the idle row
        keeps computing finite values nobody reads)."""
        aset = getattr(self.model, "lora_adapters", None)
        if aset is not None:
            aset.assign(b, adapter)
        elif adapter is not None:
            raise ValueError("SlotDecodeGraph.fill: adapter given, but the model carries no adapter set "
                             "(lora.attach_many)")
        self.token[b:b + 1].copy_(token.reshape(1))
        self.pos[b:b + 1].fill_(int(pos))
        ops.embedding(self.token[b:b + 1], self.model.transformer.wte.weight, out=self.x_emb[b:b + 1])
        self.active[b:b + 1].fill_(1)

    def release(self, b: int) -> None:
        """Slot b goes idle: its rows of the following steps leave its cache slot alone."""
        self.active[b:b + 1].zero_()

    def _step_body(self, s: int) -> None:
        model, B = self.model, self.B
        logits = model(self.token.view(B, 1), self.pos, embedded=self.x_emb, active=self.active).view(B, -1)
        table = model.transformer.wte.weight
        for b in range(B):
            out = self.history[s, b:b + 1]
            if self.temperature > 0.0 and self.top_p < 1.0:
                ops.sample_nucleus(logits[b], self.top_k, self.top_p, self.temperature,
                                   uniform=self.uniforms[s, b:b + 1], out_idx=out, token_out=self.token[b:b + 1],
                                   pos_inout=self.pos[b:b + 1], table=table, emb_out=self.x_emb[b])
            elif self.temperature > 0.0:
                ops.sample_topk(logits[b], self.top_k, self.temperature, uniform=self.uniforms[s, b:b + 1],
                                out_idx=out, token_out=self.token[b:b + 1], pos_inout=self.pos[b:b + 1], table=table,
                                emb_out=self.x_emb[b])
            else:
                ops.argmax_embed(logits[b], table, self.x_emb[b], out_idx=out, token_out=self.token[b:b + 1],
                                 pos_inout=self.pos[b:b + 1])

    def _capture(self) -> None:
        torch.cuda.synchronize(self.token.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step_body(0)
        self.graph = g
        if self.chunk > 1:
            gc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc):
                for s in range(self.chunk):
                    self._step_body(s)
            self.chunk_graph = gc

    def run(self, n_steps: int, uniforms=None):
        """One launch of ``n_steps`` (1 or ``chunk``) decode steps of every slot. ``uniforms``: the (n_steps, B) draws
        under sampling, written to the device ahead of the launch. Returns the launch's tokens as n_steps lists of B
        ints — the launch's one device -> host read."""
        if n_steps not in (1, self.chunk):
            raise ValueError(f"SlotDecodeGraph: a launch runs 1 or {self.chunk} steps, not {n_steps}")
        if self.temperature > 0.0:
            if uniforms is None or len(uniforms) != n_steps:
                raise ValueError("SlotDecodeGraph: sampling needs the launch's (n_steps, B) uniforms")
            self.uniforms[:n_steps].copy_(torch.tensor(uniforms, dtype=torch.float32))
        if not self._captured:  # the first launch is real and eager; then the graphs are captured
            for s in range(n_steps):
                self._step_body(s)
            if self.use_graph:
                self._capture()
            self._captured = True
        elif not self.use_graph:
            for s in range(n_steps):
                self._step_body(s)
        elif n_steps == 1:
            self.graph.replay()
        else:
            self.chunk_graph.replay()
        return self.history[:n_steps].tolist()
