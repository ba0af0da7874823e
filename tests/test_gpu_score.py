"""Log-likelihood scoring on the MI355X: the kernels of csrc/score.hip against the float64 specification
(tests/score_spec.py) on the same stored logits, lit_gpt/score.py pinned to the reference's own logits (fixture g2)
and to the oracle on sharp synthetic models, and the entry points of eval/.

Bounds. A log-probability from the kernel: 1e-5 + 2^-21 |ref| (x - m is exact in fp32 for bf16 inputs; the sum carries
at most log2 n + 2 roundings of 2^-24 plus a few ulp per exp, about 1.2e-6 in the log; the final subtraction rounds at
2^-24 |lp|). A KL: 1e-5 + 2^-20 A_r, A_r = sum_j p_j |log p_j - log q_j|. A log-probability of a whole model against a
reference: 2 (ACC_FACTOR R_r + ACC_SLACK max|ref_r|) plus the kernel tolerance, where R_r is the reference bf16 path's
own max abs logit error on the row (tests/parity.py's constants) and 2 is the sup-norm Lipschitz constant of
x_t - logsumexp(x).
"""

from __future__ import annotations

import functools
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import score_spec as spec
from oracle import synth
from parity import ACC_FACTOR, ACC_SLACK
from test_gpu_model import CFGS, _AdoptGpuRoutes, _GpuRoutes, build_gpu_model, oracle_for

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = Path(__file__).resolve().parent.parent

NS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 32000, 50304, 65537]


def _rows_for(n):
    return [1, 2, 65, 300] if n <= 1024 else [1, 2, 65]


@functools.lru_cache(maxsize=4)
def _logits(n, dtype, scale, seed=0):
    """Seeded logits with |x| <= 32, stored in ``dtype`` (the spec sees the stored values), and seeded targets."""
    rows = _rows_for(n)[-1]
    g = torch.Generator().manual_seed(1000 * seed + n)
    x = (torch.randn(rows, n, generator=g) * scale).clamp_(-32, 32).to(dtype)
    t = torch.randint(0, n, (rows,), generator=g, dtype=torch.int32)
    return x, t


def _lp_tol(ref):
    return spec.KERNEL_LP_ABS + spec.KERNEL_LP_REL * np.abs(ref)


# ------------------------------------------------------------------------------------------------ kernels vs the spec
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", NS)
def test_token_logprobs_match_spec(n, dtype):
    from lit_gpt import ops

    for scale in (1.0, 8.0):
        x, t = _logits(n, dtype, scale)
        ref_lp, ref_am = spec.token_logprobs(x, t)
        xd, td = x.to(DEV), t.to(DEV)
        full = None
        for rows in _rows_for(n):
            lp, am = ops.token_logprobs(xd[:rows], td[:rows])
            lp, am = lp.cpu().double().numpy(), am.cpu().numpy()
            err = np.abs(lp - ref_lp[:rows])
            print(f"n={n} {dtype} scale={scale} rows={rows}: max err {err.max():.3g} at |ref| "
                  f"{np.abs(ref_lp[:rows]).max():.3g}")
            assert (err <= _lp_tol(ref_lp[:rows])).all(), (n, rows, scale, float(err.max()))
            assert np.array_equal(am, ref_am[:rows]), (n, rows, scale)
            full = (lp, am)
        # the row-wise greedy kernel picks the same token, bit for bit
        idx = torch.empty(x.shape[0], dtype=torch.int64, device=DEV)
        for r in range(x.shape[0]):
            ops.argmax(xd[r], out_idx=idx[r:r + 1])
        assert np.array_equal(idx.cpu().numpy(), full[1])


@pytest.mark.parametrize("n", NS)
def test_logits_kl_match_spec(n):
    from lit_gpt import ops

    for scale in (1.0, 8.0):
        p, _ = _logits(n, torch.bfloat16, scale)
        q, _ = _logits(n, torch.bfloat16, scale, seed=1)
        ref_kl, ref_a, ref_agree = spec.logits_kl(p, q)
        pd, qd = p.to(DEV), q.to(DEV)
        for rows in _rows_for(n):
            kl, agree = ops.logits_kl(pd[:rows], qd[:rows])
            err = np.abs(kl.cpu().double().numpy() - ref_kl[:rows])
            tol = spec.KERNEL_KL_ABS + spec.KERNEL_KL_REL * ref_a[:rows]
            print(f"kl n={n} scale={scale} rows={rows}: max err {err.max():.3g}, max A {ref_a[:rows].max():.3g}")
            assert (err <= tol).all(), (n, rows, scale, float(err.max()))
            assert np.array_equal(agree.cpu().numpy(), ref_agree[:rows])
        kl, agree = ops.logits_kl(pd, pd.clone())
        assert (kl == 0).all() and (agree == 1).all()  # kl(p, p) is exactly 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [65, 257, 1000, 65537])
def test_rows_are_independent_of_the_batch(n, dtype):
    """Any row scored alone (its own tensor: another address, another alignment for odd n) is bit-identical to the same
    row inside the 65-row batch."""
    from lit_gpt import ops

    x, t = _logits(n, dtype, 8.0)
    xd, td = x[:65].to(DEV), t[:65].to(DEV)
    lp, am = ops.token_logprobs(xd, td)
    for r in (0, 1, 2, 7, 31, 64):
        lp1, am1 = ops.token_logprobs(xd[r:r + 1].clone(), td[r:r + 1].clone())
        assert lp1.view(torch.int32).item() == lp[r].view(torch.int32).item(), (n, r)
        assert am1.item() == am[r].item()
        e = min(r + 2, 65)
        lp2, _ = ops.token_logprobs(xd[r:e], td[r:e])  # a view into the batch: for odd n a misaligned start
        assert lp2[0].view(torch.int32).item() == lp[r].view(torch.int32).item(), (n, r)
    if dtype == torch.bfloat16:
        q = _logits(n, dtype, 8.0, seed=1)[0][:65].to(DEV)
        kl, ag = ops.logits_kl(xd, q)
        for r in (0, 1, 31, 64):
            kl1, ag1 = ops.logits_kl(xd[r:r + 1].clone(), q[r:r + 1].clone())
            assert kl1.view(torch.int32).item() == kl[r].view(torch.int32).item(), (n, r)
            assert ag1.item() == ag[r].item()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [5, 257, 3000, 32000])
def test_special_rows(n, dtype):
    from lit_gpt import ops

    inf, nan = float("inf"), float("nan")
    g = torch.Generator().manual_seed(n)
    base = (torch.randn(12, n, generator=g) * 4).clamp_(-32, 32)
    t = torch.randint(0, n, (12,), generator=g, dtype=torch.int32)
    x = base.clone()
    x[0] = 1.5  # all equal: -log n, argmax 0
    x[1, n - 1] = 40.0  # the maximum at the last index
    x[2] = x[2].clamp(max=2.5)
    x[2, [n // 3, n - 2]] = 3.0  # tied maxima (at least two): the lowest index wins
    x[2, n // 5] = 3.0
    x[3] = torch.where(torch.arange(n) % 2 == 0, 3e4, -3e4)  # must not overflow
    t[3] = 1
    x[4, ::2] = -inf  # -inf entries contribute 0
    t[4] = 1 if n > 1 else 0
    x[5, : n // 2 + 1] = -inf
    t[5] = 0  # a -inf target gives -inf
    x[6, [n // 2, n - 1]] = nan  # NaN row: NaN, argmax at the first NaN
    x[7] = -inf  # all -inf: NaN (as torch.log_softmax), argmax 0
    x[8, n // 2] = inf  # +inf: NaN
    t[9] = -1  # targets outside [0, n): NaN, neighbours unaffected
    t[10] = n
    x = x.to(dtype)
    ref_lp, ref_am = spec.token_logprobs(x, t)
    lp, am = ops.token_logprobs(x.to(DEV), t.to(DEV))
    lp, am = lp.cpu().double().numpy(), am.cpu().numpy()
    assert np.array_equal(am, ref_am), (am, ref_am)
    assert am[0] == 0 and am[1] == n - 1 and am[2] == n // 5 and am[6] == n // 2 and am[7] == 0
    for r in range(12):
        if np.isnan(ref_lp[r]):
            assert np.isnan(lp[r]), (r, lp[r])
        elif np.isinf(ref_lp[r]):
            assert lp[r] == ref_lp[r], (r, lp[r])
        else:
            assert abs(lp[r] - ref_lp[r]) <= _lp_tol(ref_lp[r]), (r, lp[r], ref_lp[r])
    assert abs(lp[0] + math.log(n)) <= _lp_tol(math.log(n))
    assert all(np.isnan(lp[r]) for r in (6, 7, 8, 9, 10)) and lp[5] == -inf
    assert np.isfinite(lp[[0, 1, 2, 3, 4, 11]]).all()
    # torch agrees with the spec on the special values
    tl = torch.log_softmax(x.double(), -1)
    assert torch.isnan(tl[6]).all() and torch.isnan(tl[7]).all() and torch.isnan(tl[8]).all()


# ------------------------------------------------------------------------------------------------ models
def _bound(r, ref_logits, ref_lp):
    """Per row: 2 (ACC_FACTOR R_r + ACC_SLACK max|ref_r|) + the kernel tolerance; ``r`` is the reference bf16 path's
    own max abs logit error on the row."""
    return 2 * (ACC_FACTOR * r + ACC_SLACK * np.abs(ref_logits).max(-1)) + _lp_tol(ref_lp)


TINY = {  # the models of fixture g2 (tests/golden/make_golden.py, tests/test_oracle_golden.py)
    "llama_mha": ("Llama-2-7b-hf", dict(n_layer=2, n_embd=256, n_head=4, intermediate_size=640, vocab_size=1000,
                                         padding_multiple=64, block_size=256)),
    "llama_gqa": ("Llama-2-70b-hf", dict(n_layer=2, n_embd=256, n_head=4, n_query_groups=2, intermediate_size=512,
                                          vocab_size=1000, padding_multiple=64, block_size=256)),
    "llama_mqa": ("Llama-2-7b-hf", dict(n_layer=2, n_embd=256, n_head=4, n_query_groups=1, intermediate_size=384,
                                         vocab_size=1000, padding_multiple=64, block_size=256)),
    "mixtral": ("Mixtral-8x7B-v0.1", dict(n_layer=2, n_embd=256, n_head=4, n_query_groups=2, intermediate_size=384,
                                           n_expert=4, n_expert_per_token=2, padded_vocab_size=1024, vocab_size=1024,
                                           block_size=256)),
}


@pytest.mark.parametrize("key", list(TINY))
@torch.inference_mode()
def test_score_tokens_pinned_to_reference_logits(key, golden):
    """The reference's own fp32 no-cache logits (fixture g2, rows 23..38) give the log-probabilities of its 16 greedy
    tokens; the product in bf16 must reproduce them as closely as the reference's own bf16 run reproduces its logits."""
    from lit_gpt import Config
    from lit_gpt.score import score_tokens

    g = golden("g2_tiny_models.npz")
    name, kw = TINY[key]
    cfg = Config.from_name(name, **kw)
    model = build_gpu_model(cfg, synth.state_dict(cfg, seed=7), "bf16", 64)
    toks = np.concatenate([g[f"{key}_prompt"], g[f"{key}_fp32_tokens"]])
    lp, greedy = score_tokens(model, toks, 16)
    ref_logits = g[f"{key}_nocache_logits"][23:39].astype(np.float64)
    ref_lp, _ = spec.token_logprobs(ref_logits, toks[24:])
    r = np.abs(g[f"{key}_bf16_logits"].astype(np.float64) - g[f"{key}_fp32_logits"].astype(np.float64)).max(-1)
    bound = _bound(r, ref_logits, ref_lp)
    err = np.abs(lp.cpu().double().numpy() - ref_lp)
    print(f"{key}: lp err {err.round(4).tolist()} bound {bound.round(4).tolist()}")
    assert (err <= bound).all(), (err.max(), bound)
    top2 = np.sort(ref_logits, -1)
    clear = (top2[:, -1] - top2[:, -2]) > bound
    assert clear.sum() >= 8, clear
    assert np.array_equal(greedy.cpu().numpy()[clear], toks[24:][clear])


@functools.lru_cache(maxsize=None)
def _sharp(key, T=65):
    """A sharp synthetic model (std 0.06: per-token log-probabilities spread by more than a nat, so a shifted row or
    target cannot pass): config, float32 state dict and 65 token ids (shared: do not modify)."""
    from lit_gpt import Config

    name, kw = CFGS[key]
    cfg = Config.from_name(name, **kw)
    sd = synth.state_dict(cfg, seed=5, std=0.06)
    toks = synth.token_ids(T, cfg.vocab_size, seed=5)
    return cfg, sd, toks


def _oracle_logits(cfg, sd, mode, ids, routes=None):
    out = {}
    for dt in (torch.float64, torch.bfloat16):
        ref = oracle_for(cfg, sd, mode, dt)
        if routes:
            ref.route_override = _AdoptGpuRoutes(routes)
        out[dt] = ref.forward(torch.from_numpy(np.asarray(ids)).long()).double().numpy()
    return out[torch.float64], out[torch.bfloat16]


@pytest.mark.parametrize("key,mode", [("gqa", "bf16"), ("gqa", "int4-g128"), ("gqa", "bnb.nf4-dq"),
                                      ("moe", "int4-g128")])
@torch.inference_mode()
def test_score_tokens_match_oracle_on_sharp_logits(key, mode):
    from lit_gpt.score import score_tokens

    cfg, sd, toks = _sharp(key)
    model = build_gpu_model(cfg, sd, mode, 64)
    with _GpuRoutes() as routes:
        lp, greedy = score_tokens(model, toks, 64)
    l64, lbf = _oracle_logits(cfg, sd, mode, toks[:-1], routes.calls)
    ref_lp, ref_am = spec.token_logprobs(l64, toks[1:])
    bound = _bound(np.abs(lbf - l64).max(-1), l64, ref_lp)
    got = lp.cpu().double().numpy()
    err = np.abs(got - ref_lp)
    bf_lp, _ = spec.token_logprobs(lbf, toks[1:])
    print(f"{key} {mode}: ref lp std {ref_lp.std():.3f}; max err {err.max():.4f} (bf16 oracle's own "
          f"{np.abs(bf_lp - ref_lp).max():.4f}); min bound {bound.min():.4f} max {bound.max():.4f}")
    assert ref_lp.std() >= 1.0, ref_lp.std()  # sharp enough for an off-by-one to show
    assert (err <= bound).all(), (float(err.max()), bound.tolist())
    # control: the reference shifted by one position is NOT matched
    shifted = np.abs(got[:-1] - ref_lp[1:]) > bound[1:]
    assert shifted.sum() >= len(shifted) / 2, shifted.sum()
    top2 = np.sort(l64, -1)
    clear = (top2[:, -1] - top2[:, -2]) > bound
    assert np.array_equal(greedy.cpu().numpy()[clear], ref_am[clear])


@torch.inference_mode()
def test_chunking_and_n_scored(monkeypatch):
    from lit_gpt import score

    cfg, sd, toks = _sharp("gqa")
    model = build_gpu_model(cfg, sd, "int4-g128", 64)
    lp, greedy = score.score_tokens(model, toks, 64)
    logits = model(torch.from_numpy(toks[:-1]).long().view(1, -1).to(DEV))[0].float()
    monkeypatch.setattr(score, "HEAD_ROWS", 5)
    lp5, greedy5 = score.score_tokens(model, toks, 64)
    # a different row count may select another GEMM path: each logit may move by one bf16 rounding
    allow = 2 * 2.0 ** -8 * float(logits.abs().max())
    assert float((lp5 - lp).abs().max()) <= allow, (float((lp5 - lp).abs().max()), allow)
    monkeypatch.setattr(score, "HEAD_ROWS", 256)
    # n_scored: 0 (no launch, empty), 1, T — each a suffix of the full result
    lp0, g0 = score.score_tokens(model, toks, 0)
    assert lp0.shape == (0,) and g0.shape == (0,) and lp0.dtype == torch.float32 and g0.dtype == torch.int32
    lp1, g1 = score.score_tokens(model, toks, 1)
    assert lp1.shape == (1,) and abs(float(lp1[0] - lp[-1])) <= allow
    # against the float64 log_softmax of the product's own full logits
    ref_lp, _ = spec.token_logprobs(logits.cpu(), toks[1:])
    assert (np.abs(lp.cpu().double().numpy() - ref_lp) <= 2 * allow + _lp_tol(ref_lp)).all()


@torch.inference_mode()
def test_scoring_leaves_the_kv_cache_alone():
    from lit_gpt.score import score_tokens

    cfg, sd, toks = _sharp("gqa")
    model = build_gpu_model(cfg, sd, "bf16", 64)
    ids = torch.from_numpy(toks[:20]).long().to(DEV)
    model(ids.view(1, -1), torch.arange(20, device=DEV))  # a generation prefill fills the cache
    before = [(b.attn.kv_cache.k.clone(), b.attn.kv_cache.v.clone()) for b in model.transformer.h]
    score_tokens(model, toks, 30)
    for b, (k, v) in zip(model.transformer.h, before):
        assert torch.equal(b.attn.kv_cache.k.view(torch.int16), k.view(torch.int16))
        assert torch.equal(b.attn.kv_cache.v.view(torch.int16), v.view(torch.int16))


class _IdTokenizer:
    """Text is space-separated ids: exact round trips for any id stream."""

    def __init__(self, vocab, eos):
        self.vocab_size, self.eos_id = vocab, eos

    def encode(self, string, device=None, bos=False, eos=False):
        return torch.tensor([int(s) for s in string.split()], dtype=torch.int32)

    def decode(self, tensor):
        return "".join(f" {int(t)}" for t in tensor.tolist())


@torch.inference_mode()
def test_loglikelihood_rolling_windows_sum():
    """150 tokens at max_seq_length 64 through the harness: the sum equals the oracle's over the spec's windows."""
    from eval.lm_eval_harness import EvalHarnessBase
    from lit_gpt import Config

    name, kw = CFGS["gqa"]
    cfg = Config.from_name(name, **kw)
    sd = synth.state_dict(cfg, seed=5, std=0.06)
    toks = synth.token_ids(150, cfg.vocab_size, seed=6).tolist()
    model = build_gpu_model(cfg, sd, "int4-g128", 64)
    lm = EvalHarnessBase(model, _IdTokenizer(cfg.vocab_size, eos=2))
    (got,) = lm.loglikelihood_rolling([(" ".join(map(str, toks)),)])
    want, slack, done = 0.0, 0.0, 0
    for inp, k in spec.rolling_windows_brute(150, 64, -1):
        ids = [2 if p < 0 else toks[p] for p in inp]
        done += k
        targets = np.asarray((ids + [toks[done - 1]])[1:])
        l64, lbf = _oracle_logits(cfg, sd, "int4-g128", ids)
        ref_lp, _ = spec.token_logprobs(l64, targets)
        want += ref_lp[-k:].sum()
        slack += _bound(np.abs(lbf - l64).max(-1), l64, ref_lp)[-k:].sum()
    assert done == 150
    print(f"rolling: got {got:.4f} oracle {want:.4f} allowed {slack:.4f}")
    assert abs(got - want) <= slack


@torch.inference_mode()
def test_pythia160m_fp32_scoring(golden):
    """32-true: fp32 logits through lga_token_logprobs_f32, on the reference's greedy run (fixture g1)."""
    from lit_gpt.score import score_tokens
    from test_gpu_neox import FP32_TOL, _pythia

    g = golden("g1_pythia160m_greedy.npz")
    cfg, sd, model = _pythia("fp32")
    toks = g["tokens"]
    lp, greedy = score_tokens(model, toks, 128)
    assert lp.dtype == torch.float32
    margins, absmax = g["margins"], g["logits_absmax"]
    checked = 0
    gr = greedy.cpu().numpy()
    for i in range(128):
        if margins[i] <= 4 * FP32_TOL * absmax[i]:
            break
        assert gr[i] == toks[16 + i], f"step {i}"
        checked += 1
    assert checked >= 64, checked
    logits = model(torch.from_numpy(toks[:-1]).long().view(1, -1).to(DEV))[0]
    assert logits.dtype == torch.float32
    ref_lp, ref_am = spec.token_logprobs(logits[-128:].cpu(), toks[16:])
    err = np.abs(lp.cpu().double().numpy() - ref_lp)
    print(f"pythia fp32: max lp err vs own logits {err.max():.3g}")
    assert (err <= _lp_tol(ref_lp)).all()
    assert np.array_equal(gr, ref_am)


@torch.inference_mode()
def test_harness_on_the_gpu():
    """loglikelihood's is_greedy on an oracle-greedy continuation with clear margins (and False with one token
    replaced); greedy_until equals generate cut at the until string."""
    from eval.lm_eval_harness import EvalHarnessBase
    from generate.base import generate

    cfg, sd, toks = _sharp("gqa")
    model = build_gpu_model(cfg, sd, "int4-g128", 64)
    # an oracle-greedy continuation whose every top-1/top-2 margin is clear (4 % of the logit scale): the first of the
    # candidate prompts (12-token slices of the stream) that yields at least 3 such tokens
    ref = oracle_for(cfg, sd, "int4-g128", torch.float64)
    prompt, cont = None, []
    for start in range(0, 52, 4):
        prompt, cont = toks[start:start + 12].tolist(), []
        for _ in range(6):
            lg = ref.forward(torch.tensor(prompt + cont))[-1]
            top2 = torch.topk(lg, 2)
            if float(top2.values[0] - top2.values[1]) <= 0.04 * float(lg.abs().max()):
                break
            cont.append(int(top2.indices[0]))
        if len(cont) >= 3:
            break
    assert len(cont) >= 3, "no candidate prompt has a clear greedy continuation"

    class Small(EvalHarnessBase):
        max_gen_toks = 8

    lm = Small(model, _IdTokenizer(cfg.vocab_size, eos=2))
    text = lambda ids: " ".join(map(str, ids))  # noqa: E731
    (lp, is_greedy), = lm.loglikelihood([(text(prompt), text(cont))])
    assert is_greedy and lp < 0
    wrong = list(cont)
    wrong[len(cont) // 2] = (wrong[len(cont) // 2] + 1) % cfg.vocab_size
    (lp2, is_greedy2), = lm.loglikelihood([(text(prompt), text(wrong))])
    assert not is_greedy2 and lp2 < lp
    # greedy_until: the same tokens generate gives, decoded and cut at the until string
    y = generate(model, torch.tensor(prompt, dtype=torch.int32, device=DEV), len(prompt) + 8, temperature=0.0)
    for b in model.transformer.h:
        b.attn.kv_cache.reset_parameters()
    new = y[len(prompt):].tolist()
    stop = f" {new[3]}"
    full = "".join(f" {t}" for t in new)
    (out,) = lm.greedy_until([(text(prompt), {"until": [stop]})])
    assert out == full.split(stop)[0]


@torch.inference_mode()
def test_compare_tokens(monkeypatch):
    from lit_gpt import score

    cfg, sd, toks = _sharp("gqa")
    mb = build_gpu_model(cfg, sd, "bf16", 64)
    mq = build_gpu_model(cfg, sd, "int4-g128", 64)
    ids = torch.from_numpy(toks[:-1]).long().view(1, -1).to(DEV)
    lb, lq = mb(ids)[0].float().cpu(), mq(ids)[0].float().cpu()
    ref_kl, ref_a, ref_agree = spec.logits_kl(lb, lq)
    tol = spec.KERNEL_KL_ABS + spec.KERNEL_KL_REL * ref_a
    # one chunk of 64 rows: the head runs on the same rows as the full forward, so the logits are the same and the
    # kernel tolerance alone applies (this is the comparison with teeth: the KL is far above it on every row)
    kl, agree = score.compare_tokens(mb, mq, toks, 64)
    err = np.abs(kl.cpu().double().numpy() - ref_kl)
    print(f"compare: kl mean {ref_kl.mean():.4f} min {ref_kl.min():.4f}; max err {err.max():.3g}, max tol {tol.max():.3g}")
    assert ref_kl.min() > 100 * tol.max(), (ref_kl.min(), tol.max())  # a zero or misplaced KL cannot pass
    assert (err <= tol).all(), float(err.max())
    assert np.array_equal(agree.cpu().numpy(), ref_agree)
    # with model_q's hidden rows handed over (eval/perplexity.py: one forward per model): the same bits
    lpq, _, hq = score.score_tokens(mq, toks, 64, return_hidden=True)
    klh, agh = score.compare_tokens(mb, mq, toks, 64, hidden_q=hq)
    assert torch.equal(klh.view(torch.int32), kl.view(torch.int32)) and torch.equal(agh, agree)
    assert torch.equal(lpq.view(torch.int32), score.score_tokens(mq, toks, 64)[0].view(torch.int32))
    klt, agt = score.compare_tokens(mb, mq, toks, 7)  # the last rows only
    assert np.abs(klt.cpu().double().numpy() - ref_kl[-7:]).max() <= tol.max()
    # chunked head (5 rows at a time may select another GEMM path: each logit may move by one bf16 rounding)
    monkeypatch.setattr(score, "HEAD_ROWS", 5)
    kl5, _ = score.compare_tokens(mb, mq, toks, 64)
    allow = 2 * 2.0 ** -8 * float(max(lb.abs().max(), lq.abs().max()))
    err5 = np.abs(kl5.cpu().double().numpy() - ref_kl)
    print(f"compare, HEAD_ROWS 5: max err {err5.max():.3g}, allowance {allow:.3g}")
    assert (err5 <= tol + allow).all(), float(err5.max())
    monkeypatch.setattr(score, "HEAD_ROWS", 256)
    kl0, agree0 = score.compare_tokens(mq, mq, toks, 64)
    assert (kl0 == 0).all() and (agree0 == 1).all()


@torch.inference_mode()
def test_unquantized_moe_scores_but_does_not_generate():
    """bf16 experts serve the no-cache multi-row forward only: a KV-cache forward is refused at the prefill already
    (not at the first decode step), and a one-row no-cache forward raises too."""
    from lit_gpt import Config
    from lit_gpt.score import score_tokens

    name, kw = TINY["mixtral"]
    cfg = Config.from_name(name, **kw)
    model = build_gpu_model(cfg, synth.state_dict(cfg, seed=7), "bf16", 64)
    ids = torch.from_numpy(synth.token_ids(12, cfg.vocab_size, seed=7)).long().to(DEV)
    lp, _ = score_tokens(model, ids, 11)
    assert torch.isfinite(lp).all()
    with pytest.raises(NotImplementedError, match="QuantLinear experts"):
        model(ids.view(1, -1), torch.arange(12, device=DEV))
    with pytest.raises(NotImplementedError, match="QuantLinear experts"):
        model(ids[:1].view(1, 1))


def test_perplexity_cli():
    """eval/perplexity.py --synthetic on a small registered config (pythia-70m: head size 64): one JSON line, ppl == exp(nll / tokens); with
    --against bf16 also the KL figures."""
    cmd = [sys.executable, str(REPO / "lit-gpt_amd" / "eval" / "perplexity.py"), "--synthetic", "pythia-70m",
           "--n_tokens", "300", "--max_seq_length", "128", "--quantize", "int4-g128", "--against", "bf16"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["tokens"] == 300 and out["windows"] == 3 and out["tokens_per_s"] > 0
    assert math.isclose(out["ppl"], math.exp(out["nll"] / out["tokens"]), rel_tol=1e-9)
    assert out["mean_kl"] >= -1e-5 and out["max_kl"] >= out["mean_kl"] and 0 <= out["top1_agree"] <= 1
