"""Single-device generation on the MI355X — drop-in for the reference's generate/base.py.

Same functions and semantics as /root/reference/generate/base.py: ``multinomial_num_samples_1`` (:22-27),
``sample`` (:30-41), ``next_token`` (:44-47), ``generate`` (:50-93: prefill at ``arange(T)``, then one-token
steps at ``input_pos = T, T+1, ...``, stop on ``eos_id``, ``NotImplementedError`` when ``max_seq_length`` is too
short) and ``main`` (:96-187) with the same flags and the same stderr timing line. Differences:
  * greedy decoding (``temperature == 0``) and top-k sampling (``top_k`` <= 1024, the reference's default 200 at
    temperature 0.8) run each step as one HIP graph replay (lit_gpt/runtime.py) with the argmax / the fused
    top-k + softmax + inverse-CDF sampler on the device — the role ``--compile`` (CUDA graphs) plays in the
    reference; the sampler's uniforms come from a counter-based RNG seeded from torch's generator, so a seed
    reproduces a run but not the reference's exact torch.multinomial draws;
  * ``--top_p P`` (``top_p=P``; not in the reference) adds nucleus sampling on the device for ``0 < P < 1``, over
    the top-k set or, with ``--top_k none``, the whole vocabulary (ops.sample_nucleus; no torch fallback);
  * ``--quantize`` takes this build's formats (int4-g128, nf4 / bnb.nf4 / bnb.nf4-dq, bnb.fp4 / bnb.fp4-dq, bnb.int8);
    without it the Linears
    stay bf16 ``nn.Linear`` (BASELINE config 2) and run on the bf16 GEMV / GEMM kernels;
  * ``--synthetic NAME`` builds a random-init model of a registered config (no checkpoint, no tokenizer): the
    prompt is ``--prompt_len`` synthetic token ids.
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path
from typing import Any, List, Optional

import torch

wd = Path(__file__).parent.parent.resolve()
if str(wd) not in sys.path:
    sys.path.append(str(wd))

from lit_gpt import GPT, Config  # noqa: E402
from lit_gpt import ops  # noqa: E402


def multinomial_num_samples_1(probs: torch.Tensor) -> torch.Tensor:
    return torch.multinomial(probs, num_samples=1)


class SamplerRNG:
    """State of the fused sampler's counter-based RNG (csrc/sample.hip): a 64-bit seed drawn from torch's default
    generator, so ``torch.manual_seed`` makes a run repeatable (generate/base.py:174), and a device counter the
    kernel advances once per draw, so a captured decode step draws a fresh uniform at every replay."""

    def __init__(self, device: torch.device, seed: Optional[int] = None) -> None:
        self.seed = int(torch.randint(0, 2**62, (1,))) if seed is None else int(seed)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)


def device_sampling(temperature: float, top_k: Optional[int], dtype: torch.dtype, vocab: int = 0,
                    top_p: float = 1.0) -> bool:
    """Whether ``sample`` at this setting runs as the one-launch HIP sampler (ops.sample_topk): temperature > 0 with
    top_k in [1, 1024] over bf16 logits of at most 65536 entries — the reference's defaults (top_k 200,
    temperature 0.8) included. With 0 < top_p < 1 (ops.sample_nucleus) top_k may also be None."""
    if 0.0 < top_p < 1.0:
        return (temperature > 0.0 and (top_k is None or 1 <= top_k <= ops.MAX_TOP_K) and dtype == torch.bfloat16
                and vocab <= ops.MAX_SAMPLE_VOCAB)
    return (temperature > 0.0 and top_k is not None and 1 <= top_k <= ops.MAX_TOP_K and dtype == torch.bfloat16
            and vocab <= ops.MAX_SAMPLE_VOCAB)


def _top_p_kw(top_p: float) -> dict:
    """``top_p`` as a keyword for the callees, passed on only when it is in effect (< 1)."""
    return {"top_p": top_p} if top_p < 1.0 else {}


def check_top_p(who: str, top_p: float, temperature: float, top_k: Optional[int], dtype: torch.dtype,
                vocab: int) -> None:
    """``top_p`` must lie in (0, 1]; below 1 (and at temperature > 0) it runs on the device sampler only: there is no
    torch fallback for top-p."""
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"{who}: top_p must be in (0, 1], got {top_p}")
    if top_p < 1.0 and temperature > 0.0 and not device_sampling(temperature, top_k, dtype, vocab, top_p):
        raise NotImplementedError(f"{who}: top_p < 1 runs on the device sampler only: bf16 logits, a vocabulary of at "
                                  f"most {ops.MAX_SAMPLE_VOCAB} and top_k None or in [1, {ops.MAX_TOP_K}]")


def sample(logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None,
           rng: Optional[SamplerRNG] = None, top_p: float = 1.0) -> torch.Tensor:
    """logits (1, T, V) on the GPU -> (1,) token (generate/base.py:30-41). Greedy runs the HIP argmax (lowest index
    on ties; top-k cannot change the arg-max); temperature > 0 with top_k <= 1024 over bf16 logits runs the HIP
    top-k + softmax + inverse-CDF sampler in one launch (``rng`` carries its RNG state; a fresh one is drawn from
    torch's generator when omitted); other settings follow the reference's torch ops, softmax in the logits' dtype.
    ``top_p`` < 1 adds nucleus sampling (ops.sample_nucleus, one launch, top_k None or <= 1024 over bf16 logits; no
    torch fallback); at temperature 0 it changes nothing, the arg-max is always in the nucleus."""
    logits = logits[0, -1]
    check_top_p("sample", top_p, temperature, top_k, logits.dtype, logits.size(-1))
    if not logits.is_cuda:
        raise RuntimeError("sample: logits must be on the GPU (this build has no CPU path)")
    if temperature > 0.0:
        if top_p < 1.0:
            rng = rng if rng is not None else SamplerRNG(logits.device)
            return ops.sample_nucleus(logits.contiguous(), top_k, top_p, temperature, seed=rng.seed,
                                      counter=rng.counter)
        if device_sampling(temperature, top_k, logits.dtype, logits.size(-1)):
            rng = rng if rng is not None else SamplerRNG(logits.device)
            return ops.sample_topk(logits.contiguous(), top_k, temperature, seed=rng.seed, counter=rng.counter)
        if top_k is not None:
            v, i = torch.topk(logits, min(top_k, logits.size(-1)))
            logits = torch.full_like(logits, float("-inf")).scatter_(-1, i, v)
        probs = torch.nn.functional.softmax(logits / temperature, dim=-1)
        return multinomial_num_samples_1(probs)
    return ops.argmax((logits if logits.dtype == torch.float32 else logits.to(torch.bfloat16)).contiguous())


def next_token(model: GPT, input_pos: torch.Tensor, x: torch.Tensor, **kwargs: Any) -> torch.Tensor:
    logits = model(x, input_pos, last_token_only=True)
    return sample(logits, **kwargs).to(dtype=x.dtype)


def graph_sampling(model: GPT, temperature: float, top_k: Optional[int], top_p: float = 1.0) -> bool:
    """Whether decode steps at this setting run as captured HIP graphs (lit_gpt/runtime.py DecodeGraph): greedy, or
    the device sampler (``device_sampling``) over the model's bf16 logits."""
    wte = model.transformer.wte.weight
    return temperature == 0.0 or device_sampling(temperature, top_k, wte.dtype, model.config.padded_vocab_size, top_p)


def _check_model_top_p(who: str, model: GPT, top_p: float, temperature: float, top_k: Optional[int]) -> None:
    check_top_p(who, top_p, temperature, top_k, model.transformer.wte.weight.dtype, model.config.padded_vocab_size)


DECODE_CHUNK = 8  # greedy decode steps per graph launch (lit_gpt/runtime.py DecodeGraph.steps)


@torch.inference_mode()
def generate(model: GPT, prompt: torch.Tensor, max_returned_tokens: int, *, temperature: float = 1.0,
             top_k: Optional[int] = None, eos_id: Optional[int] = None, use_graph: bool = True,
             rng: Optional[SamplerRNG] = None, top_p: float = 1.0) -> torch.Tensor:
    """Takes a conditioning sequence (prompt, shape (T,)) and continues it; returns (T + new,) ids. ``rng``: the
    device sampler's state to draw from (a fresh one seeded from torch's generator when omitted). ``top_p`` < 1:
    nucleus sampling on the device (``sample``)."""
    T = prompt.size(0)
    assert max_returned_tokens > T
    if top_p != 1.0:
        _check_model_top_p("generate", model, top_p, temperature, top_k)
        if temperature == 0.0:
            top_p = 1.0  # greedy: top-p cannot change the arg-max
    tp = _top_p_kw(top_p)
    if model.max_seq_length < max_returned_tokens - 1:
        raise NotImplementedError(f"max_seq_length {model.max_seq_length} needs to be >= {max_returned_tokens - 1}")
    device = prompt.device
    tokens = [prompt]
    rng = (rng or SamplerRNG(device)) if temperature > 0.0 else None
    token = next_token(model, torch.arange(0, T, device=device), prompt.view(1, -1), temperature=temperature,
                       top_k=top_k, rng=rng, **tp).clone()
    tokens.append(token)
    n_steps = max_returned_tokens - T - 1
    if n_steps <= 0:
        return torch.cat(tokens)
    if use_graph and graph_sampling(model, temperature, top_k, **tp):
        from lit_gpt.runtime import DecodeGraph

        # (the prefill's token is never tested against eos: the reference's loop only tests the decoded ones,
        # generate/base.py:86-92)
        # runs the first decode step eagerly, then captures the step (and DECODE_CHUNK steps as one graph)
        dg = DecodeGraph(model, token, T, chunk=DECODE_CHUNK if n_steps > DECODE_CHUNK else 1,
                         temperature=temperature, top_k=top_k, rng=rng, **tp)
        out = torch.empty(n_steps, dtype=prompt.dtype, device=device)
        out[0] = dg.token.view(-1)[0]
        produced = 1
        if not (eos_id is not None and int(out[0]) == eos_id):
            i = 1
            while i < n_steps:
                if dg.chunk > 1 and n_steps - i >= dg.chunk:
                    out[i:i + dg.chunk] = dg.steps()
                    n = dg.chunk
                else:
                    out[i] = dg.step().view(-1)[0]
                    n = 1
                produced = i + n
                if eos_id is not None:  # one host check per launch; tokens past an eos are dropped
                    hit = (out[i:i + n] == eos_id).nonzero()
                    if hit.numel():
                        produced = i + int(hit[0]) + 1
                        break
                i += n
        tokens.append(out[:produced])
        _check_collectives()
        return torch.cat(tokens)
    input_pos = torch.tensor([T], device=device)
    for _ in range(n_steps):
        token = next_token(model, input_pos, token.view(1, -1), temperature=temperature, top_k=top_k,
                           rng=rng, **tp).clone()
        tokens.append(token)
        if eos_id is not None and int(token) == eos_id:
            break
        input_pos = input_pos.add_(1)
    _check_collectives()
    return torch.cat(tokens)


MAX_BATCH = GPT.MAX_BATCH  # sequences per batched decode step (4: lit_gpt/model.py)


def _check_adapters(who: str, model: GPT, adapters, n: int):
    """``adapters`` of a batched call: one entry per prompt, the index of its LoRA adapter in ``model.lora_adapters``
    (lit_gpt.lora.attach_many) or None. Returns (the set or None, the list); on a model with a set and no ``adapters``
    every prompt runs without one. Raises before anything is launched."""
    aset = getattr(model, "lora_adapters", None)
    if adapters is None:
        return aset, [None] * n
    if aset is None:
        raise ValueError(f"{who}: adapters given, but the model carries no adapter set (lit_gpt.lora.attach_many)")
    adapters = list(adapters)
    if len(adapters) != n:
        raise ValueError(f"{who}: {len(adapters)} adapters for {n} prompts")
    return aset, [aset.check(a, who) for a in adapters]


class _selected:
    """``with _selected(aset, i)``: one-sequence calls run adapter i of the set (None: the base model); the set's
    earlier selection returns on exit. Without a set it does nothing."""

    def __init__(self, aset, i) -> None:
        self.aset, self.i = aset, i

    def __enter__(self):
        if self.aset is not None:
            self.before = self.aset.selected
            self.aset.select(self.i)

    def __exit__(self, *exc) -> None:
        if self.aset is not None:
            self.aset.select(self.before)


def _batch_steps(dg, n_steps: int, eos_id: Optional[int]):
    """Drive a batched step executor (lit_gpt.runtime.BatchDecodeGraph: ``B``, ``token`` (B,) holding the first
    step's tokens, ``chunk``, ``step()``, ``steps()``) for ``n_steps`` steps in all. Returns the (n_steps, B) token
    buffer and, per sequence, how many of its tokens count: up to and including its first ``eos_id``. A sequence
    that met it stops collecting; the batch keeps stepping until every sequence has, one host read per launch."""
    B = dg.B
    out = torch.empty(n_steps, B, dtype=torch.int64, device=dg.token.device)
    out[0] = dg.token.view(-1)
    lengths: List[Optional[int]] = [None] * B

    def scan(i: int, n: int) -> bool:  # rows i .. i + n are new: note each open sequence's first eos among them
        if eos_id is None:
            return False
        hit = (out[i:i + n] == eos_id).cpu()  # the launch's one device -> host read
        for b in range(B):
            if lengths[b] is None and bool(hit[:, b].any()):
                lengths[b] = i + int(hit[:, b].nonzero()[0]) + 1
        return all(n_b is not None for n_b in lengths)

    i = 1
    done = scan(0, 1)
    while i < n_steps and not done:
        if dg.chunk > 1 and n_steps - i >= dg.chunk:
            out[i:i + dg.chunk] = dg.steps()
            n = dg.chunk
        else:
            out[i] = dg.step().view(-1)
            n = 1
        done = scan(i, n)
        i += n
    return out, [i if n_b is None else n_b for n_b in lengths]


@torch.inference_mode()
def generate_batch(model: GPT, prompts: List[torch.Tensor], max_new_tokens: int, *, temperature: float = 1.0,
                   top_k: Optional[int] = None, eos_id: Optional[int] = None, seeds: Optional[List[int]] = None,
                   use_graph: bool = True, top_p: float = 1.0, adapters=None) -> List[torch.Tensor]:
    """Continue up to MAX_BATCH = 4 prompts (each (T_b,), lengths may differ) by ``max_new_tokens`` tokens each,
    decoding them together: every decode step streams the weights once for all sequences (the multi-row GEMVs; attention runs per
    sequence). Sequence b gets exactly the tokens ``generate`` returns for ``prompts[b]`` alone (under sampling: with
    ``SamplerRNG(seed=seeds[b])``). Each prompt is prefilled alone into slot b of the KV cache, which is rebuilt for
    ``len(prompts)`` sequences when it holds fewer. A sequence that meets ``eos_id`` stops collecting tokens; the
    batch steps on until all have or ``max_new_tokens`` is reached. Returns the (T_b + new_b,) ids per sequence.
    ``adapters`` (a ``lit_gpt.lora.attach_many`` model): per prompt the index of its LoRA adapter or None; sequence b
    then gets the tokens of ``generate`` under ``model.lora_adapters.select(adapters[b])``."""
    B = len(prompts)
    if B == 0:
        raise ValueError("generate_batch: no prompts")
    aset, adapters = _check_adapters("generate_batch", model, adapters, B)
    if top_p != 1.0:
        _check_model_top_p("generate_batch", model, top_p, temperature, top_k)
        if temperature == 0.0:
            top_p = 1.0
    tp = _top_p_kw(top_p)
    if B > MAX_BATCH:
        raise NotImplementedError(f"generate_batch: {B} prompts; the MI355X batched decode runs at most {MAX_BATCH} "
                                  "sequences per step")
    if max_new_tokens < 1:
        raise ValueError("generate_batch: max_new_tokens must be at least 1")
    if seeds is not None and len(seeds) != B:
        raise ValueError(f"generate_batch: {len(seeds)} seeds for {B} prompts")
    longest = max(p.size(0) for p in prompts)
    if model.max_seq_length < longest + max_new_tokens - 1:
        raise NotImplementedError(f"max_seq_length {model.max_seq_length} needs to be >= "
                                  f"{longest + max_new_tokens - 1}")
    if B > 1 and temperature > 0.0 and not graph_sampling(model, temperature, top_k, **tp):
        raise NotImplementedError("generate_batch: sampling a batch runs on the device sampler only (temperature > 0 "
                                  f"with top_k in [1, {ops.MAX_TOP_K}] over bf16 logits)")
    device = prompts[0].device
    rngs = None
    if temperature > 0.0:
        rngs = [SamplerRNG(device, None if seeds is None else seeds[b]) for b in range(B)]
    if B == 1:
        with _selected(aset, adapters[0]):
            return [generate(model, prompts[0], prompts[0].size(0) + max_new_tokens, temperature=temperature,
                             top_k=top_k, eos_id=eos_id, use_graph=use_graph, rng=None if rngs is None else rngs[0],
                             **tp)]
    kv = model.transformer.h[0].attn.kv_cache
    if kv is None or kv.k.size(0) < B:
        model.set_kv_cache(batch_size=B, device=device, dtype=None if kv is None else kv.cache_dtype)
    firsts = []
    for b, prompt in enumerate(prompts):  # the single path's prefill (next_token), on slot b
        T = prompt.size(0)
        with _selected(aset, adapters[b]):
            logits = model(prompt.view(1, -1), torch.arange(0, T, device=device), last_token_only=True, kv_slot=b)
        firsts.append(sample(logits, temperature=temperature, top_k=top_k,
                             rng=None if rngs is None else rngs[b], **tp).to(dtype=prompt.dtype).clone())
    n_steps = max_new_tokens - 1
    if n_steps <= 0:
        return [torch.cat([p, f]) for p, f in zip(prompts, firsts)]
    from lit_gpt.runtime import BatchDecodeGraph

    dg = BatchDecodeGraph(model, torch.cat(firsts), [p.size(0) for p in prompts],
                          chunk=DECODE_CHUNK if use_graph and n_steps > DECODE_CHUNK else 1,
                          temperature=temperature, top_k=top_k, rngs=rngs, use_graph=use_graph,
                          **({} if aset is None else {"adapters": adapters}), **tp)
    out, lengths = _batch_steps(dg, n_steps, eos_id)
    return [torch.cat([p, f, out[:n_b, b].to(p.dtype)]) for b, (p, f, n_b) in enumerate(zip(prompts, firsts, lengths))]


# What ``generate_samples(share="auto")`` takes where the shared-prefix launch applies: True = that launch, False = the
# copy route. Fixed by the rule of DESIGN §4.5f: the launch is picked only if it beat the batch launch per block at B =
# 2 and B = 4 at all three measured positions by more than the runs' spread.
SHARE_AUTO = False


def _copy_prefix(model: GPT, P: int, B: int) -> None:
    """Rows [0, P) of cache slot 0 into slots 1..B-1 of every layer (codes and scales too for the fp8 cache)."""
    for block in model.transformer.h:
        kv = block.attn.kv_cache
        for t in (kv.k, kv.v) + ((kv.k_scale, kv.v_scale) if kv.fp8 else ()):
            t[1:B, :, :P].copy_(t[:1, :, :P].expand(B - 1, *t.shape[1:2], P, *t.shape[3:]))


@torch.inference_mode()
def generate_samples(model: GPT, prompt: torch.Tensor, max_new_tokens: int, num_samples: int, *,
                     temperature: float = 1.0, top_k: Optional[int] = None, top_p: float = 1.0,
                     eos_id: Optional[int] = None, seeds: Optional[List[int]] = None, use_graph: bool = True,
                     share="auto", wave: int = MAX_BATCH) -> List[torch.Tensor]:
    """``num_samples`` completions of ONE prompt ((T,)), each ``max_new_tokens`` long at most, for one prefill: the
    prompt goes into cache slot 0 once, the first token of sample i is drawn from that one logits row with
    ``SamplerRNG(device, seeds[i])`` (its draw 0), and the samples decode together in waves of at most MAX_BATCH = 4
    behind the same prefix; rows [0, T) of slot 0 are never rewritten. Sample i is exactly what ``generate(model,
    prompt, T + max_new_tokens, ..., rng=SamplerRNG(device, seeds[i]))`` returns (at temperature 0 all are equal);
    ``num_samples == 1`` is that call. ``seeds`` None: one per sample from torch's generator, in sample order.
    ``share=True``: the wave's decode attention is the shared-prefix launch (``ops.attention_decode_shared``: the
    prompt's K / V stay in slot 0 alone and every step reads them once per set of rows), ``NotImplementedError`` where
    it does not apply (fp8 cache, a geometry outside the batch launch's). ``share=False``: the prompt's rows are copied
    into the wave's other slots and the wave runs the batched step of ``generate_batch`` — everything that covers.
    ``share="auto"``: the launch where it applies and ``SHARE_AUTO`` allows it, else the copies. Refuses what
    ``generate_batch`` refuses, before any launch. ``wave``: samples per wave, 1..MAX_BATCH. A model that carries a
    LoRA adapter set (``lit_gpt.lora.attach_many``) is refused too: a prefix depends on its adapter."""
    if num_samples < 1:
        raise ValueError("generate_samples: num_samples must be at least 1")
    if not 1 <= wave <= MAX_BATCH:
        raise NotImplementedError(f"generate_samples: waves of {wave}; the MI355X batched decode runs 1..{MAX_BATCH} "
                                  "sequences per step")
    if share not in (True, False, "auto"):
        raise ValueError(f"generate_samples: share must be True, False or 'auto', got {share!r}")
    if max_new_tokens < 1:
        raise ValueError("generate_samples: max_new_tokens must be at least 1")
    if seeds is not None and len(seeds) != num_samples:
        raise ValueError(f"generate_samples: {len(seeds)} seeds for {num_samples} samples")
    if getattr(model, "lora_adapters", None) is not None:
        raise NotImplementedError("generate_samples: a model with a LoRA adapter set (a prefix depends on its adapter)")
    if top_p != 1.0:
        _check_model_top_p("generate_samples", model, top_p, temperature, top_k)
        if temperature == 0.0:
            top_p = 1.0
    tp = _top_p_kw(top_p)
    T = prompt.size(0)
    if model.max_seq_length < T + max_new_tokens - 1:
        raise NotImplementedError(f"max_seq_length {model.max_seq_length} needs to be >= {T + max_new_tokens - 1}")
    device = prompt.device
    sampling = temperature > 0.0
    B = min(num_samples, wave)
    if B > 1 and sampling and not graph_sampling(model, temperature, top_k, **tp):
        raise NotImplementedError("generate_samples: sampling several samples runs on the device sampler only "
                                  f"(temperature > 0 with top_k in [1, {ops.MAX_TOP_K}] over bf16 logits)")
    if sampling and seeds is None:
        seeds = [int(torch.randint(0, 2**62, (1,))) for _ in range(num_samples)]  # as SamplerRNG draws its own
    rngs = [SamplerRNG(device, s) for s in seeds] if sampling else None
    if num_samples == 1:
        return [generate(model, prompt, T + max_new_tokens, temperature=temperature, top_k=top_k, eos_id=eos_id,
                         use_graph=use_graph, rng=None if rngs is None else rngs[0], **tp)]
    model._batch_check(B)  # before any launch
    kv = model.transformer.h[0].attn.kv_cache
    applies = (model.transformer.h[0].attn.batch_fusable(model.transformer.wte.weight.dtype)
               and not (kv is not None and kv.fp8))
    if share is True and not applies:
        raise NotImplementedError("generate_samples(share=True): the shared-prefix decode attention needs the bf16 KV "
                                  "cache and the batched decode attention's geometry (head_size == rope_n_elem == "
                                  "128, 1 / 2 / 4 / 8 heads per query group, bf16 activations)")
    shared = applies and (share is True or (share == "auto" and SHARE_AUTO))
    if kv is None or kv.k.size(0) < B:
        model.set_kv_cache(batch_size=B, device=device, dtype=None if kv is None else kv.cache_dtype)
    logits = model(prompt.view(1, -1), torch.arange(0, T, device=device), last_token_only=True, kv_slot=0)
    firsts = [sample(logits, temperature=temperature, top_k=top_k, rng=None if rngs is None else rngs[i],
                     **tp).to(dtype=prompt.dtype).clone() for i in range(num_samples)]
    n_steps = max_new_tokens - 1
    if n_steps <= 0:
        return [torch.cat([prompt, f]) for f in firsts]
    from lit_gpt.runtime import BatchDecodeGraph

    if not shared:
        _copy_prefix(model, T, B)
    prefix = torch.tensor([T], dtype=torch.int64, device=device) if shared else None
    ys: List[torch.Tensor] = []
    for w in range(0, num_samples, B):  # a wave: up to ``wave`` samples in slots 0.. behind the one prefix
        nb = min(B, num_samples - w)
        dg = BatchDecodeGraph(model, torch.cat(firsts[w:w + nb]), [T] * nb,
                              chunk=DECODE_CHUNK if use_graph and n_steps > DECODE_CHUNK else 1,
                              temperature=temperature, top_k=top_k, rngs=None if rngs is None else rngs[w:w + nb],
                              use_graph=use_graph, **({"shared_prefix": prefix} if shared and nb > 1 else {}), **tp)
        out, lengths = _batch_steps(dg, n_steps, eos_id)
        ys += [torch.cat([prompt, firsts[w + b], out[:n_b, b].to(prompt.dtype)]) for b, n_b in enumerate(lengths)]
    return ys


@torch.inference_mode()
def generate_continuous(model: GPT, prompts: List[torch.Tensor], max_new_tokens, *, batch_size: int = MAX_BATCH,
                        temperature: float = 1.0, top_k: Optional[int] = None, eos_id: Optional[int] = None,
                        seeds: Optional[List[int]] = None, use_graph: bool = True,
                        chunk: int = DECODE_CHUNK, top_p: float = 1.0, adapters=None) -> List[torch.Tensor]:
    """Continuous batching: any number of prompts (each (T_i,)) through ``min(batch_size, len(prompts))`` slots of the
    batched decode step. ``max_new_tokens``: an int, or one per prompt. A prompt enters a free slot through the single
    path's prefill; a sequence that met ``eos_id`` or its budget leaves its slot to the next prompt of the queue while
    the other slots keep decoding, their state on the device (lit_gpt.runtime.SlotDecodeGraph; the bookkeeping is
    lit_gpt.scheduler.SlotScheduler). Returns the (T_i + new_i,) ids in prompt order; ``result[i]`` is exactly what
    ``generate(model, prompts[i], T_i + max_new_i, ..., rng=SamplerRNG(device, seeds[i]))`` returns on a cache of the
    same ``max_seq_length``. Refuses what ``generate_batch`` refuses. ``adapters`` (a ``lit_gpt.lora.attach_many``
    model): per prompt the index of its LoRA adapter or None; ``result[i]`` is then that ``generate`` under
    ``model.lora_adapters.select(adapters[i])``, and a slot takes its next sequence's adapter without a recapture."""
    from lit_gpt.scheduler import SlotScheduler

    n = len(prompts)
    if n == 0:
        raise ValueError("generate_continuous: no prompts")
    aset, adapters = _check_adapters("generate_continuous", model, adapters, n)
    if top_p != 1.0:
        _check_model_top_p("generate_continuous", model, top_p, temperature, top_k)
        if temperature == 0.0:
            top_p = 1.0
    tp = _top_p_kw(top_p)
    if batch_size < 1:
        raise ValueError("generate_continuous: batch_size must be at least 1")
    if batch_size > MAX_BATCH:
        raise NotImplementedError(f"generate_continuous: batch_size {batch_size}; the MI355X batched decode runs at "
                                  f"most {MAX_BATCH} sequences per step")
    B = min(batch_size, n)
    device = prompts[0].device
    sampling = temperature > 0.0
    if sampling and seeds is None:
        seeds = [int(torch.randint(0, 2**62, (1,))) for _ in range(n)]  # as SamplerRNG draws its own
    sched = SlotScheduler([p.size(0) for p in prompts], max_new_tokens, B, chunk=chunk, eos_id=eos_id, seeds=seeds if sampling else None, max_seq_length=model.max_seq_length)
    budgets = [s + 1 for s in sched.steps_budget]
    if B == 1:  # one slot: the single path, one prompt after the other
        out = []
        for i, (p, m) in enumerate(zip(prompts, budgets)):
            with _selected(aset, adapters[i]):
                out.append(generate(model, p, p.size(0) + m, temperature=temperature, top_k=top_k, eos_id=eos_id,
                                    use_graph=use_graph, rng=SamplerRNG(device, seeds[i]) if sampling else None, **tp))
        return out
    if sampling and not graph_sampling(model, temperature, top_k, **tp):
        raise NotImplementedError("generate_continuous: sampling runs on the device sampler only (temperature > 0 "
                                  f"with top_k in [1, {ops.MAX_TOP_K}] over bf16 logits)")
    model._batch_check(B)  # before any launch
    if not model.transformer.h[0].attn.batch_fusable(model.transformer.wte.weight.dtype):
        raise NotImplementedError("generate_continuous needs the batched decode attention launch (head_size == "
                                  "rope_n_elem == 128, 1 / 2 / 4 / 8 heads per query group, bf16 activations)")
    kv = model.transformer.h[0].attn.kv_cache
    if kv is None or kv.k.size(0) < B:
        model.set_kv_cache(batch_size=B, device=device, dtype=None if kv is None else kv.cache_dtype)
    from lit_gpt.runtime import SlotDecodeGraph

    ex = SlotDecodeGraph(model, B, chunk=sched.chunk, temperature=temperature, top_k=top_k, use_graph=use_graph,
                         **tp)
    firsts: List[Optional[torch.Tensor]] = [None] * n
    while not sched.done:
        while (fill := sched.next_fill()) is not None:  # the single path's prefill (next_token), on the free slot
            b, i = fill
            prompt, T = prompts[i], prompts[i].size(0)
            with _selected(aset, adapters[i]):
                logits = model(prompt.view(1, -1), torch.arange(0, T, device=device), last_token_only=True,
                               kv_slot=b)
            firsts[i] = sample(logits, temperature=temperature, top_k=top_k,
                               rng=SamplerRNG(device, seeds[i]) if sampling else None,
                               **tp).to(dtype=prompt.dtype).clone()
            if sched.start(b):
                ex.fill(b, firsts[i], T, **({} if aset is None else {"adapter": adapters[i]}))
        if sched.done:
            break
        n_steps = sched.next_launch()
        history = ex.run(n_steps, sched.uniforms(n_steps) if sampling else None)
        for b in sched.consume(history):
            ex.release(b)
    return [torch.cat([p, f, torch.tensor(t, dtype=p.dtype, device=device)])
            for p, f, t in zip(prompts, firsts, sched.results())]


def _check_collectives() -> None:
    """Under tensor parallelism with the xGMI all-reduce: raise (on every rank) if any decode all-reduce of this
    run gave up waiting for a peer — its logits were summed from partial data (lit_gpt/comm.py check_errors)."""
    from lit_gpt import comm

    if comm.get_default() is not None:
        comm.check_errors()


# --kv_cache choices -> GPT.set_kv_cache dtype (None: the activation dtype)
KV_CACHE_DTYPES = {"bf16": None, "fp8": torch.float8_e4m3fn}


def build_model(config: Config, *, quantize: Optional[str], device: torch.device, seed: int = 1234,
                checkpoint_path: Optional[Path] = None, max_seq_length: Optional[int] = None,
                fabric=None, rope_positions: str = "reference", prefill_rows: Optional[int] = None,
                dtype: torch.dtype = torch.bfloat16, kv_cache: str = "bf16") -> GPT:
    """Instantiate on the meta device, then materialise (load, or random-init as GPT._init_weights) the float
    weights on the GPU in the model's parameter order; with ``fabric`` (world_size / global_rank, generate/tp.py)
    every block is sharded (``tensor_parallel_block``) and quantized as soon as its weights exist, so a rank holds
    at most one unsharded block (70B TP=8: ~1.7 GB, not the whole 138 GB model). Then the rope tables and the KV
    cache. Mirrors generate/base.py:151-171 / generate/tp.py:157-190 (convert_module -> tensor_parallel ->
    to_device: the values each rank quantizes are its float shard, as there).

    ``rope_positions="reference"`` builds the rope tables under a bf16 default dtype, as the reference's
    ``with fabric.init_tensor(): model.max_seq_length = ...`` does under bf16-true / bnb precision
    (generate/base.py:153-157): positions above 256 round to bf16. ``"exact"`` keeps fp32 positions.
    ``prefill_rows`` (the prompt length about to be served) is accepted for API stability; the prefill GEMMs are
    hand-written (csrc/gemm_q4f.hip) and need no per-shape tuning or warm-up. ``dtype`` float32 is the reference's
    ``--precision 32-true`` (GPT-NeoX family, csrc/fp32.hip; no quantization, no TP). ``kv_cache="fp8"`` builds the
    e4m3 KV cache (``GPT.set_kv_cache(dtype=torch.float8_e4m3fn)``) in place of one in ``dtype``."""
    if kv_cache not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache must be one of {sorted(KV_CACHE_DTYPES)}, got {kv_cache!r}")
    if kv_cache == "fp8" and (dtype == torch.float32 or (fabric is not None and fabric.world_size > 1)):
        # (before any weight is materialised; GPT.set_kv_cache refuses the same, and the geometry, at the cache)
        raise NotImplementedError("--kv_cache fp8 runs with bf16 activations on one device (no 32-true, no tensor "
                                  "parallelism)")
    if dtype not in (torch.bfloat16, torch.float32):
        raise NotImplementedError(f"precision with dtype {dtype}: the MI355X path computes in bf16 or fp32")
    if dtype == torch.float32 and (quantize is not None or (fabric is not None and fabric.world_size > 1)):
        raise NotImplementedError("32-true runs unquantized on one device (BASELINE config 1)")
    if rope_positions not in ("reference", "exact"):
        raise ValueError(f"rope_positions must be 'reference' or 'exact', got {rope_positions!r}")
    from lit_gpt.quantize import QuantizedPrecision

    if quantize is not None:
        from lit_gpt.quantize import parse_mode

        parse_mode(quantize)  # unsupported modes fail before any weight is materialised
        if quantize == "bnb.int8":  # out of scope for the int8 kernels; refused before any weight is materialised
            if config._mlp_class == "LLaMAMoE":
                raise NotImplementedError("--quantize bnb.int8 with a sparse-MoE model: the routed expert kernels "
                                          "take 4-bit experts only (int4-g128, nf4, bnb.fp4 and their -dq forms)")
            if fabric is not None and fabric.world_size > 1:
                raise NotImplementedError("--quantize bnb.int8 with tensor parallelism: the fused GEMV + all-reduce "
                                          "takes 4-bit or bf16 shards only; run bnb.int8 on one device")
    tp = None
    if fabric is not None and fabric.world_size > 1:
        from generate import tp

        for attr in ("n_head", "n_embd", "n_query_groups"):  # fail before materialising (generate/tp.py:87-90)
            if getattr(config, attr) % fabric.world_size:
                raise ValueError(f"This {attr} value ({getattr(config, attr)}) is not evenly divisible by the world "
                                 f"size ({fabric.world_size})")
    with torch.device("meta"):
        model = GPT(config)
    state = None
    if checkpoint_path is not None:
        state = torch.load(str(checkpoint_path), mmap=True, map_location="cpu", weights_only=True)
        state = state.get("model", state)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    precision = QuantizedPrecision(quantize) if quantize is not None else None

    def finish(module: torch.nn.Module) -> None:
        """Shard (TP) and quantize one fully materialised block (or the top-level Linears)."""
        if tp is not None and hasattr(module, "attn"):
            tp.tensor_parallel_block(fabric, module)
        if precision is not None:
            precision.convert_module(module, device)
            mlp = getattr(module, "mlp", None)
            if hasattr(mlp, "_stack"):  # sparse MoE: the experts' packed weights stacked now, not in the first prompt
                mlp._stack()
        else:  # bf16-true: the Linears stay nn.Linear; TP row shards are strided views -> own contiguous storage
            for mod in module.modules():
                if isinstance(mod, torch.nn.Linear) and not mod.weight.is_contiguous():
                    mod.weight = torch.nn.Parameter(mod.weight.data.contiguous(), requires_grad=False)

    open_block = None
    for name, p in list(model.named_parameters()):
        mod_name, _, attr = name.rpartition(".")
        parts = name.split(".")
        blk = int(parts[2]) if parts[:2] == ["transformer", "h"] else None
        if open_block is not None and blk != open_block:
            finish(model.transformer.h[open_block])
        open_block = blk
        mod = model.get_submodule(mod_name)
        if state is not None:
            t = state[name].to(device=device, dtype=dtype)
        elif attr == "weight" and (isinstance(mod, (torch.nn.Linear, torch.nn.Embedding))):
            t = torch.empty(p.shape, dtype=torch.float32, device=device).normal_(0.0, 0.02, generator=gen)
            t = t.to(dtype)
        elif attr == "bias":
            t = torch.zeros(p.shape, dtype=dtype, device=device)
        else:  # norm weights
            t = torch.ones(p.shape, dtype=dtype, device=device)
        setattr(mod, attr, torch.nn.Parameter(t, requires_grad=False))
    if open_block is not None:
        finish(model.transformer.h[open_block])
    if precision is not None:  # lm_head (replicated under TP, as the reference leaves it unsharded)
        precision.convert_module(model, device)
    if tp is not None:
        tp.shard_config(fabric, model)
    torch.cuda.empty_cache()
    prev = torch.get_default_dtype()
    # (32-true: the reference's default dtype stays float32, so its positions are exact)
    torch.set_default_dtype(torch.bfloat16 if rope_positions == "reference" and dtype == torch.bfloat16
                            else torch.float32)
    try:
        model.max_seq_length = max_seq_length or config.block_size
        model.cos, model.sin = model.rope_cache(device=device)
    finally:
        torch.set_default_dtype(prev)
    model.set_kv_cache(batch_size=1, device=device, dtype=KV_CACHE_DTYPES[kv_cache] or dtype)
    ops.preload_kernels()  # the runtime would otherwise build each prefill kernel inside the first prompt
    return model.eval()


@torch.inference_mode()
def main(prompt: str = "What food do llamas eat?", *, num_samples: int = 1, max_new_tokens: int = 50,
         top_k: Optional[int] = 200, temperature: float = 0.8,
         checkpoint_dir: Path = Path("checkpoints/stabilityai/stablelm-base-alpha-3b"),
         quantize: Optional[str] = None, precision: Optional[str] = None, compile: bool = False,
         synthetic: Optional[str] = None, prompt_len: int = 16, batch_size: int = 1,
         kv_cache: str = "bf16", prompts_file: Optional[Path] = None, top_p: float = 1.0,
         share_prompt: bool = False) -> None:
    precision = precision or "bf16-true"
    if share_prompt and batch_size <= 1:
        raise ValueError("--share_prompt decodes the samples of one prompt together: it needs --batch_size > 1")
    if share_prompt and prompts_file is not None:
        raise ValueError("--share_prompt serves the samples of ONE prompt: it cannot be combined with --prompts_file")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"--top_p must be in (0, 1], got {top_p}")
    tp = _top_p_kw(top_p)
    if not 1 <= batch_size <= MAX_BATCH:
        raise NotImplementedError(f"--batch_size {batch_size}: the batched decode runs 1..{MAX_BATCH} sequences")
    if precision not in ("bf16-true", "32-true"):
        raise NotImplementedError("the MI355X path computes in bf16 (bf16-true) or fp32 (32-true)")
    dtype = torch.float32 if precision == "32-true" else torch.bfloat16
    device = torch.device("cuda", torch.cuda.current_device())
    tokenizer = None
    lines = None
    if prompts_file is not None:  # one prompt per line (--synthetic: one prompt length per line)
        lines = [ln.strip() for ln in Path(prompts_file).read_text().splitlines() if ln.strip()]
        if not lines:
            raise ValueError(f"--prompts_file {prompts_file}: no prompts")
    if synthetic is not None:
        config = Config.from_name(synthetic)
        checkpoint_path = None
        g = torch.Generator(device="cpu").manual_seed(1234)
        lens = [prompt_len] if lines is None else [int(ln) for ln in lines]
        many = [torch.randint(0, config.vocab_size, (n,), generator=g, dtype=torch.int32).to(device) for n in lens]
        encoded = many[0]
    else:
        from lit_gpt.tokenizer import Tokenizer
        from lit_gpt.utils import check_valid_checkpoint_dir

        check_valid_checkpoint_dir(checkpoint_dir)
        config = Config.from_json(checkpoint_dir / "lit_config.json")
        checkpoint_path = checkpoint_dir / "lit_model.pth"
        tokenizer = Tokenizer(checkpoint_dir)
        many = [tokenizer.encode(ln, device=device) for ln in (lines if lines is not None else [prompt])]
        encoded = many[0]
    prompt_length = encoded.size(0) if lines is None else max(e.size(0) for e in many)
    max_returned_tokens = prompt_length + max_new_tokens
    print(f"Loading model {str(checkpoint_path or synthetic)!r} with {config.__dict__}", file=sys.stderr)
    t0 = time.perf_counter()
    model = build_model(config, quantize=quantize, device=device, checkpoint_path=checkpoint_path,
                        max_seq_length=max_returned_tokens, prefill_rows=prompt_length, dtype=dtype,
                        kv_cache=kv_cache)
    print(f"Time to load the model weights: {time.perf_counter() - t0:.02f} seconds.", file=sys.stderr)
    torch.manual_seed(1234)
    eos_id = tokenizer.eos_id if tokenizer is not None else None
    if lines is not None:
        # --prompts_file: every prompt through --batch_size slots (generate_continuous), completions in file order
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys = generate_continuous(model, many, max_new_tokens, batch_size=batch_size, temperature=temperature,
                                 top_k=top_k, eos_id=eos_id, **tp)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        for y in ys:
            print(tokenizer.decode(y) if tokenizer is not None else y.tolist())
        tokens_generated = sum(y.size(0) - e.size(0) for y, e in zip(ys, many))
        print(f"Time for inference of {len(many)} prompts through {min(batch_size, len(many))} slots: {t:.02f} sec "
              f"total, {tokens_generated / t:.02f} tokens/sec", file=sys.stderr)
        print(f"Memory used: {torch.cuda.max_memory_allocated() / 1e9:.02f} GB", file=sys.stderr)
        return
    if share_prompt:
        # --share_prompt: all samples behind one prefill of the prompt (generate_samples), --batch_size at a time; the
        # seeds are drawn in the order the loop below draws them, so the samples are the same
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys = generate_samples(model, encoded, max_new_tokens, num_samples, temperature=temperature, top_k=top_k,
                              eos_id=eos_id, wave=batch_size, **tp)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        for block in model.transformer.h:
            block.attn.kv_cache.reset_parameters()
        for y in ys:
            print(tokenizer.decode(y) if tokenizer is not None else y.tolist())
        tokens_generated = sum(y.size(0) - prompt_length for y in ys)
        print(f"Time for inference of {num_samples} samples of one prompt: {t:.02f} sec total, "
              f"{tokens_generated / t:.02f} tokens/sec", file=sys.stderr)
        print(f"Memory used: {torch.cuda.max_memory_allocated() / 1e9:.02f} GB", file=sys.stderr)
        return
    for i in range(0, num_samples if batch_size > 1 else 0, batch_size):
        # --batch_size B: the samples B at a time, decoded together (generate_batch; each its own sampler seed)
        nb = min(batch_size, num_samples - i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys = generate_batch(model, [encoded] * nb, max_new_tokens, temperature=temperature, top_k=top_k, eos_id=eos_id,
                            **tp)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        for block in model.transformer.h:
            block.attn.kv_cache.reset_parameters()
        for y in ys:
            print(tokenizer.decode(y) if tokenizer is not None else y.tolist())
        tokens_generated = sum(y.size(0) - prompt_length for y in ys)
        print(f"Time for inference {i // batch_size + 1}: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec",
              file=sys.stderr)
    for i in range(num_samples if batch_size == 1 else 0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = generate(model, encoded, max_returned_tokens, temperature=temperature, top_k=top_k, eos_id=eos_id, **tp)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        for block in model.transformer.h:
            block.attn.kv_cache.reset_parameters()
        print(tokenizer.decode(y) if tokenizer is not None else y.tolist())
        tokens_generated = y.size(0) - prompt_length
        print(f"Time for inference {i + 1}: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec",
              file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_allocated() / 1e9:.02f} GB", file=sys.stderr)


def top_k_arg(text: str) -> Optional[int]:
    """--top_k: an integer, or the word ``none``."""
    return None if text.strip().lower() == "none" else int(text)


def _cli(argv=None) -> None:
    p = argparse.ArgumentParser(description="Generates text samples based on a pre-trained model and tokenizer.")
    p.add_argument("--prompt", default="What food do llamas eat?")
    p.add_argument("--num_samples", type=int, default=1)
    p.add_argument("--max_new_tokens", type=int, default=50)
    p.add_argument("--top_k", type=top_k_arg, default=200, help="an integer, or 'none' (with --top_p: the nucleus "
                   "over the whole vocabulary)")
    p.add_argument("--top_p", type=float, default=1.0, help="nucleus sampling: the smallest set of most likely "
                   "tokens whose probability reaches top_p (1.0: off)")
    p.add_argument("--temperature", type=float, default=0.8)
    p.add_argument("--checkpoint_dir", type=Path, default=Path("checkpoints/stabilityai/stablelm-base-alpha-3b"))
    p.add_argument("--quantize", default=None)
    p.add_argument("--precision", default=None)
    p.add_argument("--compile", action="store_true")
    p.add_argument("--synthetic", default=None, help="random-init model of this registered config name")
    p.add_argument("--prompt_len", type=int, default=16)
    p.add_argument("--batch_size", type=int, default=1,
                   help="decode the samples this many at a time (1..4) through generate_batch")
    p.add_argument("--prompts_file", type=Path, default=None,
                   help="one prompt per line (with --synthetic: one prompt length per line); all of them run through "
                        "--batch_size slots with continuous batching (generate_continuous)")
    p.add_argument("--kv_cache", default="bf16", choices=sorted(KV_CACHE_DTYPES),
                   help="KV cache format: fp8 = e4m3 codes + one power-of-two scale per row (0.516 x the bytes)")
    p.add_argument("--share_prompt", action="store_true",
                   help="with --batch_size > 1: prefill the prompt once for all --num_samples samples "
                        "(generate_samples) instead of once per sample")
    a = p.parse_args(argv)
    main(a.prompt, num_samples=a.num_samples, max_new_tokens=a.max_new_tokens, top_k=a.top_k,
         temperature=a.temperature, checkpoint_dir=a.checkpoint_dir, quantize=a.quantize, precision=a.precision,
         compile=a.compile, synthetic=a.synthetic, prompt_len=a.prompt_len, batch_size=a.batch_size,
         kv_cache=a.kv_cache, prompts_file=a.prompts_file, top_p=a.top_p, share_prompt=a.share_prompt)


if __name__ == "__main__":
    _cli()
