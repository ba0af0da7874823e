"""The specification of the scoring kernels and of the window plan, in float64 numpy — what csrc/score.hip and
lit_gpt/score.py are tested against (tests/test_score_host.py, tests/test_gpu_score.py)."""

from __future__ import annotations

import numpy as np

KERNEL_LP_ABS = 1e-5  # tolerance of one log-probability: KERNEL_LP_ABS + KERNEL_LP_REL * |ref|
KERNEL_LP_REL = 2.0 ** -21
KERNEL_KL_ABS = 1e-5  # tolerance of one KL: KERNEL_KL_ABS + KERNEL_KL_REL * A_r
KERNEL_KL_REL = 2.0 ** -20


def _f64(x):
    if hasattr(x, "detach"):
        x = x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def log_softmax(x):
    """Row-wise log_softmax in float64 with torch's special cases: -inf entries contribute 0; a row holding NaN or
    +inf, or all -inf, is NaN."""
    x = _f64(x)
    with np.errstate(all="ignore"):
        m = x.max(axis=-1, keepdims=True)
        out = x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))
    return out


def argmax(x):
    """torch.argmax order per row: the first NaN if any, else the lowest index among the maxima."""
    x = _f64(x)
    out = np.empty(x.shape[0], dtype=np.int64)
    for r, row in enumerate(x):
        nan = np.flatnonzero(np.isnan(row))
        out[r] = nan[0] if nan.size else int(np.argmax(row))  # np.argmax: first occurrence
    return out


def token_logprobs(x, targets):
    """(logprob float64 (rows,), argmax int64 (rows,)); a target outside [0, n) scores NaN."""
    x = _f64(x)
    ls = log_softmax(x)
    t = np.asarray(targets, dtype=np.int64)
    ok = (t >= 0) & (t < x.shape[1])
    lp = np.full(x.shape[0], np.nan)
    rows = np.arange(x.shape[0])
    lp[ok] = ls[rows[ok], t[ok]]
    return lp, argmax(x)


def logits_kl(p, q):
    """(kl (rows,), A (rows,), agree (rows,)): kl_r = sum_j P_j (log P_j - log Q_j), its magnitude term
    A_r = sum_j P_j |log P_j - log Q_j| (what the kernel's rounding scales with), and argmax agreement."""
    lp, lq = log_softmax(p), log_softmax(q)
    w = np.exp(lp)
    d = lp - lq
    return (w * d).sum(-1), (w * np.abs(d)).sum(-1), (argmax(p) == argmax(q)).astype(np.int64)


def rolling_windows_brute(n_tokens: int, max_len: int, prefix_token, min_context: int = 1):
    """The window plan built token by token over the positions 0 .. n_tokens - 1: walk the tokens in order; a token
    joins the open window while that window scores fewer than its quota (max_len for the first, max_len - min_context
    + 1 after it); a window's input is, for the first, the prefix and the tokens before its last scored one, and for
    the others the max_len tokens before its last scored one."""
    out, scored = [], []
    first = True
    for tok in range(n_tokens):
        quota = max_len if first else max_len - min_context + 1
        scored.append(tok)
        if len(scored) == quota or tok == n_tokens - 1:
            last = scored[-1]
            if first:
                inp = [prefix_token] + [t for t in range(n_tokens) if t < last]
            else:
                inp = [t for t in range(n_tokens) if last - max_len <= t < last]
            out.append((inp, len(scored)))
            scored, first = [], False
    return out
