"""Log-likelihood scoring over the existing forward: the log-probability a model assigns to given tokens.

``score_tokens`` runs the no-cache causal forward (``GPT.forward(..., input_pos=None, hidden_only=True)``: the
generation KV cache is not touched), keeps the hidden rows whose predictions are asked for, runs ``ln_f`` + ``lm_head``
on them ``HEAD_ROWS`` at a time and reduces each chunk of logits on the device with ``ops.token_logprobs``
(csrc/score.hip): the live logits buffer is ``HEAD_ROWS x padded_vocab_size``, never ``T x V``, and no logit is copied
to the host. The vocabulary axis is ``padded_vocab_size``: the reference's harness (eval/lm_eval_harness.py) takes
``log_softmax`` over the model's full output.

``compare_tokens`` does the same with two models built from the same weights (say bf16 and a quantized format) and
reduces both chunks with ``ops.logits_kl``: how far the second model's next-token distribution is from the first's.

``rolling_windows`` is the host-side plan that cuts a long text into windows of at most ``max_len`` inputs so that
every token is scored exactly once (lm-eval 0.3's ``get_rolling_token_windows`` + ``make_disjoint_window``).

Batch size 1 and one device: tensor-parallel scoring is refused.
"""

from __future__ import annotations

from typing import Iterator, List, Optional, Sequence, Tuple, Union

import torch

HEAD_ROWS = 256  # rows of logits alive at a time (256 x 32000 bf16 = 16 MB)


def rolling_windows(tokens: Union[int, Sequence[int]], max_len: int, prefix_token: int,
                    min_context: int = 1) -> Iterator[Tuple[List[int], int]]:
    """Yield ``(input_ids, n_scored)``: the model input of each window and how many of its LAST rows are scored.
    Row ``i`` of a window predicts the token after ``input_ids[i]``; over all windows every token of ``tokens`` is
    predicted exactly once, in order, and no input is longer than ``max_len``.

    ``tokens`` is the id sequence, or an int ``n`` standing for the positions ``0 .. n - 1`` (to plan or to test).
    The first window's input is ``[prefix_token] + tokens[:k - 1]`` and scores ``k = min(max_len, n)`` tokens. A later
    window that scores ``tokens[a:b]`` takes as input ``tokens[b - 1 - max_len:b - 1]``, the ``max_len`` tokens that
    end just before the last scored one: right-aligned, so the final, shorter window reuses earlier tokens as extra
    context. Later windows score at most ``max_len - min_context + 1`` tokens each, so every scored token sees at least
    ``min_context`` inputs; ``min_context=1`` is lm-eval's ``context_len=1`` (disjoint, maximal windows)."""
    toks = list(range(tokens)) if isinstance(tokens, int) else list(tokens)
    n = len(toks)
    if max_len < 1:
        raise ValueError(f"rolling_windows: max_len must be >= 1, got {max_len}")
    if not 1 <= min_context <= max_len:
        raise ValueError(f"rolling_windows: min_context must be in [1, max_len={max_len}], got {min_context}")
    if n == 0:
        return
    k = min(max_len, n)
    yield [prefix_token] + toks[:k - 1], k
    step = max_len - min_context + 1
    a = k
    while a < n:
        b = min(n, a + step)
        yield toks[b - 1 - max_len:b - 1], b - a
        a = b


def _refuse_tp() -> None:
    from lit_gpt import comm

    if comm.get_default() is not None:
        raise NotImplementedError("scoring under tensor parallelism is not implemented: score on one device")


def _host_ids(tokens, vocab: int) -> torch.Tensor:
    """The ids as a CPU int64 vector, validated against [0, vocab) before anything is launched."""
    ids = torch.as_tensor(tokens).detach().to("cpu").reshape(-1)
    if ids.is_floating_point() or ids.dtype == torch.bool:
        raise TypeError(f"token ids must be integers, got {ids.dtype}")
    ids = ids.to(torch.int64)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
        raise ValueError(f"token ids must lie in [0, {vocab}): got min {int(ids.min())}, max {int(ids.max())}")
    return ids


def _plan(model, tokens, n_scored: int) -> Tuple[torch.Tensor, int]:
    _refuse_tp()
    ids = _host_ids(tokens, model.config.padded_vocab_size)
    T = ids.numel() - 1
    if not 0 <= n_scored <= max(T, 0):
        raise ValueError(f"n_scored must be in [0, {max(T, 0)}] for {ids.numel()} tokens, got {n_scored}")
    if T > model.max_seq_length:
        raise ValueError(f"Cannot score {ids.numel()} tokens: the input of {T} exceeds max_seq_length "
                         f"{model.max_seq_length}")
    return ids, T


def _hidden(model, ids: torch.Tensor, T: int, n_scored: int, cached: bool = False) -> torch.Tensor:
    """The last ``n_scored`` rows of the last block's output for the input ``ids[:-1]``: the no-cache causal forward,
    or with ``cached`` a prefill through the model's KV cache at positions 0 .. T - 1 (which it overwrites)."""
    dev = model.transformer.wte.weight.device
    pos = torch.arange(T, device=dev) if cached else None
    x = model(ids[:-1].to(dev).view(1, -1), input_pos=pos, hidden_only=True)
    return x.view(T, -1)[T - n_scored:]


def _head(model, h: torch.Tensor) -> torch.Tensor:
    """(rows, n_embd) hidden -> (rows, padded_vocab_size) logits: ln_f + lm_head as GPT.forward runs them."""
    from lit_gpt.model import _lin
    from lit_gpt.rmsnorm import RMSNorm

    rows = h.shape[0]
    x = h.contiguous().view(1, rows, -1)
    ln = model.transformer.ln_f
    if isinstance(ln, RMSNorm):
        y = _lin(model.lm_head, x, norm_weight=ln.weight, norm_eps=ln.eps)
    else:
        y = _lin(model.lm_head, ln(x))
    return y.reshape(rows, -1)


@torch.inference_mode()
def score_tokens(model, tokens, n_scored: int, *, return_hidden: bool = False, cached: bool = False):
    """``(logprobs fp32 (n_scored,), greedy int32 (n_scored,))`` on the model's device: for the last ``n_scored``
    tokens of ``tokens``, the log-probability the model gives each one after the tokens before it, and the model's
    own arg-max at that position. ``tokens[:-1]`` is the input (at most ``model.max_seq_length`` long).
    ``return_hidden`` appends the ``(n_scored, n_embd)`` hidden rows the head ran on, which ``compare_tokens`` takes
    as ``hidden_q`` so that a caller wanting both runs this model's blocks once. ``cached`` scores the window as a
    prefill through the model's KV cache (``input_pos = arange(T)``) instead of the no-cache forward, so the
    log-probabilities reflect the cache format — an fp8 cache's quantized K / V (eval/perplexity.py ``--kv_cache``)."""
    from lit_gpt import ops

    ids, T = _plan(model, tokens, n_scored)
    dev = model.transformer.wte.weight.device
    lp = torch.empty(n_scored, dtype=torch.float32, device=dev)
    greedy = torch.empty(n_scored, dtype=torch.int32, device=dev)
    h = None
    if n_scored:
        h = _hidden(model, ids, T, n_scored, cached)
        targets = ids[ids.numel() - n_scored:].to(device=dev, dtype=torch.int32)
        for a in range(0, n_scored, HEAD_ROWS):
            b = min(n_scored, a + HEAD_ROWS)
            ops.token_logprobs(_head(model, h[a:b]), targets[a:b], logprob_out=lp[a:b], argmax_out=greedy[a:b])
    return (lp, greedy, h) if return_hidden else (lp, greedy)


@torch.inference_mode()
def compare_tokens(model_p, model_q, tokens, n_scored: int, *, hidden_q: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(kl fp32 (n_scored,), agree int32 (n_scored,))``: at each of the last ``n_scored`` positions,
    KL(model_p's next-token distribution || model_q's) and whether both models' arg-max agree. Both models see
    ``tokens[:-1]``; their vocabularies must match. ``hidden_q``: model_q's hidden rows for these very ``tokens`` and
    ``n_scored`` (``score_tokens(..., return_hidden=True)``), which spares its forward."""
    from lit_gpt import ops

    ids, T = _plan(model_p, tokens, n_scored)
    _plan(model_q, ids, n_scored)
    if model_p.config.padded_vocab_size != model_q.config.padded_vocab_size:
        raise ValueError("compare_tokens: the two models' padded_vocab_size differ")
    dev = model_p.transformer.wte.weight.device
    kl = torch.empty(n_scored, dtype=torch.float32, device=dev)
    agree = torch.empty(n_scored, dtype=torch.int32, device=dev)
    if n_scored == 0:
        return kl, agree
    if hidden_q is not None and tuple(hidden_q.shape) != (n_scored, model_q.config.n_embd):
        raise ValueError(f"compare_tokens: hidden_q is {tuple(hidden_q.shape)}, expected "
                         f"({n_scored}, {model_q.config.n_embd})")
    hp = _hidden(model_p, ids, T, n_scored)
    hq = hidden_q if hidden_q is not None else _hidden(model_q, ids, T, n_scored)
    for a in range(0, n_scored, HEAD_ROWS):
        b = min(n_scored, a + HEAD_ROWS)
        ops.logits_kl(_head(model_p, hp[a:b]), _head(model_q, hq[a:b]), kl_out=kl[a:b], agree_out=agree[a:b])
    return kl, agree
