"""The nucleus (top-p) sampler's specification in plain Python integers and numpy; not a test file.

    C       the top-k set of oracle.model.sample_topk_spec (top_k given), or every index
    p       bf16 softmax of bf16(v / temperature) over C, as sample_topk_spec computes it
    w       trunc(float(p) * 2**30), W = sum w (an integer below 2**31)
    target  clamp(ceil(double(top_p) * double(W)), 1, W), top_p held in fp32
    N       { i in C : above(i) < target }, above(i) = the weight of the candidates whose logit is greater than v_i
    tau     floor(double(u) * double(W')) + 1, W' = sum of w over N, u held in fp32
    token   the first i in N, in index order, whose inclusive prefix sum of w over N reaches tau
"""

import math

import numpy as np
import torch

from oracle import model as om

SCALE = 2 ** 30


def candidates(logits_bf16: torch.Tensor, top_k):
    """C in index order: sample_topk_spec's kept set, or every index."""
    n = logits_bf16.numel()
    if top_k:
        kept, _, _ = om.sample_topk_spec(logits_bf16, top_k, 1.0, 0.5)
        return np.asarray(kept, dtype=np.int64)
    return np.arange(n, dtype=np.int64)


def probabilities(logits_bf16: torch.Tensor, cand, temperature: float) -> np.ndarray:
    """Step 2 over C, as sample_topk_spec: fp32 values that hold bf16 numbers."""
    v = (logits_bf16.float()[torch.from_numpy(cand)] / temperature).to(torch.bfloat16).float()
    e = torch.exp(v - v.max())
    return (e / e.sum()).to(torch.bfloat16).float().numpy()


def weights(probs) -> np.ndarray:
    return np.trunc(np.asarray(probs, dtype=np.float64) * SCALE).astype(np.int64)


def nucleus_flags(values, w, top_p: float):
    """Steps 3-4 on the candidates' logit values and weights -> (flags, W, target)."""
    values = np.asarray(values, dtype=np.float64)  # (-0.0 == +0.0 as floats: one class)
    W = int(w.sum())
    target = min(max(math.ceil(float(np.float32(top_p)) * float(W)), 1), W)
    _, inv = np.unique(values, return_inverse=True)  # classes, ascending
    class_w = np.zeros(int(inv.max()) + 1, dtype=np.int64)
    np.add.at(class_w, inv, w)
    above = np.cumsum(class_w[::-1])[::-1] - class_w
    return above[inv] < target, W, target


def draw(w, flags, u: float):
    """Step 5 -> (position in C, tau, W')."""
    wn = np.where(flags, w, 0)
    Wn = int(wn.sum())
    tau = math.floor(float(np.float32(u)) * float(Wn)) + 1
    return int(np.searchsorted(np.cumsum(wn), tau, side="left")), tau, Wn


def nucleus_spec(logits_bf16: torch.Tensor, top_k, top_p: float, temperature: float, u: float, probs=None):
    """1-D bf16 logits -> (candidates, probs, flags, token). With ``probs`` given (one per candidate, index order)
    steps 3-5 are evaluated on those probabilities."""
    cand = candidates(logits_bf16, top_k)
    p = probabilities(logits_bf16, cand, temperature) if probs is None else np.asarray(probs, dtype=np.float32)
    w = weights(p)
    flags, _, _ = nucleus_flags(logits_bf16.float().numpy()[cand], w, top_p)
    j, _, _ = draw(w, flags, u)
    return cand, p, flags, int(cand[j])
