"""Speculative decoding measurements: what the verify window costs and what it buys.

usage: python tools/spec_decode.py kernels [--out profiles/spec_kernels.json]
           (a) us per launch of lga_attention_decode_window at M = 2, 4, 8 against M back-to-back one-row
           lga_attention_decode_fused launches on the same cache (what a verify step without the window kernel would
           run), Llama-2-7B geometry (32 heads, 32 groups) and one GQA geometry (32 heads, 8 groups) at p = 2048 in a
           2304-row cache. One graph of 32 "layers" over distinct caches, median of 7 replays.
           (b) the whole verify step (embedding -> decode_window -> spec_accept, one graph) of synthetic Llama-2-7B
           int4-g128 at M = 1..8 against the one-row greedy step (DecodeGraph), p = 2048, median of 7 replays; and
           the same verify step under top-k sampling (spec_accept_sample in spec_accept's place) against the one-row
           sampled step.
           (s) us per call of lga_spec_accept_sample (the window sampler + the accept launch) at M = 1, 2, 4, 8
           (n = 32000, top_k = 200, temperature 0.8) against M back-to-back lga_sample_topk launches. One graph of
           32 calls over distinct logits, median of 7 replays.
       python tools/spec_decode.py e2e [--out profiles/spec_e2e.json] [--prompt_len 2048] [--steps 255]
                                       [--temperature 0.8 --top_k 200]
           (c) synthetic Llama-2-7B int4-g128, greedy, decode tokens/s (prefill timed apart) of generate and of
           generate_speculative at gamma = 1, 3, 7 with a scripted drafter forced to 0 %, ~50 % and 100 % acceptance
           (it knows generate's output), and the 100 % rows again with a 4-layer synthetic draft model's drafting
           time included. Random synthetic weights give no meaningful acceptance rate of their own: none is quoted.
           With --temperature T --top_k K: the same under sampling (generate and generate_speculative with one
           sampler seed), and in place of the 4-layer rows an nf4 twin of the target (same float weights) as
           ModelDrafter, coupled (drafts sampled with the target's uniforms) and uncoupled (greedy drafts), with the
           acceptance each reaches. That acceptance is a property of the synthetic weights (near-flat top-k
           distributions), not of trained checkpoints.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

HS = 128
LAYERS = 32


def _median_us(run, launches, reps=7):
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    return _replay_us(g, reps) / launches


def _replay_us(g, reps=7):
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e3)
    return statistics.median(times)


def attention(result, p=2048, max_seq=2304):
    from lit_gpt.model import build_rope_cache

    dev = torch.device("cuda")
    cos, sin = (t.float().contiguous() for t in build_rope_cache(max_seq, HS, device=dev))
    scale = 1.0 / math.sqrt(HS)
    for name, (H, G) in {"llama-2-7b (32 heads, 32 groups)": (32, 32), "gqa (32 heads, 8 groups)": (32, 8)}.items():
        n_splits = ops.decode_splits(G, H // G, HS, max_seq)
        caches = [(torch.randn(G, max_seq, HS, device=dev).bfloat16(), torch.randn(G, max_seq, HS, device=dev).bfloat16())
                  for _ in range(LAYERS)]
        qkv = torch.randn(8, (H + 2 * G) * HS, device=dev).bfloat16()
        pos = [torch.tensor([p + r], device=dev) for r in range(8)]
        y = torch.empty(8, H * HS, device=dev, dtype=torch.bfloat16)
        ws1 = ops.AttentionWorkspace(1, H, G, HS, n_splits, dev)
        row = {"n_splits": n_splits, "p": p, "max_seq": max_seq}

        def one_row(M):
            def run():
                for kc, vc in caches:
                    for r in range(M):
                        ops.attention_decode_fused(qkv[r:r + 1], kc, vc, pos[r], pos[r], cos, sin, H, G, HS, HS, scale,
                                                   n_splits, workspace=ws1, out=y[r:r + 1])
            return run

        def window(M):
            ws = ops.AttentionWorkspace(M, H, G, HS, n_splits, dev)

            def run():
                for kc, vc in caches:
                    ops.attention_decode_window(qkv[:M], kc, vc, pos[0], cos, sin, H, G, HS, HS, scale, n_splits,
                                                workspace=ws, out=y[:M])
            return run

        row["one_row_us"] = _median_us(one_row(1), LAYERS)
        for M in (1, 2, 4, 8):
            row[f"window_{M}_us"] = _median_us(window(M), LAYERS)  # (the append launch included)
            row[f"one_row_x{M}_us"] = _median_us(one_row(M), LAYERS)
            row[f"ok_{M}"] = bool(M == 1 or row[f"window_{M}_us"] < row[f"one_row_x{M}_us"])
        result["attention"][name] = row
        print(name, json.dumps(row), flush=True)
        del caches
        torch.cuda.empty_cache()


def _model(prompt_len, steps, quantize="int4-g128", **over):
    from generate.base import build_model
    from lit_gpt import Config

    cfg = Config.from_name("Llama-2-7b-hf", **over)
    return build_model(cfg, quantize=quantize, device=torch.device("cuda"), max_seq_length=prompt_len + steps + 1,
                       seed=4321 if over else 1234)


def sampler(result, n=32000, top_k=200, temperature=0.8, calls=32):
    dev = torch.device("cuda")
    logits = [(torch.randn(8, n, device=dev) * 3.0).bfloat16() for _ in range(calls)]
    window = torch.zeros(8, dtype=torch.int32, device=dev)
    out = torch.zeros(9, dtype=torch.int32, device=dev)
    sampled = torch.zeros(8, dtype=torch.int32, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    row = {"n": n, "top_k": top_k, "temperature": temperature}

    def one_row(M):
        def run():
            for lg in logits:
                for r in range(M):
                    ops.sample_topk(lg[r], top_k, temperature, seed=1234, counter=counter, out_idx=idx[r:r + 1])
        return run

    def entry(M):
        def run():
            for lg in logits:
                ops.spec_accept_sample(lg[:M], window[:M], top_k, temperature, seed=1234, counter=counter,
                                       out=out[:M + 1], sampled=sampled)
        return run

    for M in (1, 2, 4, 8):
        row[f"window_{M}_us"] = _median_us(entry(M), calls)  # (both launches of the entry)
        row[f"one_row_x{M}_us"] = _median_us(one_row(M), calls)
        row[f"ok_{M}"] = bool(M == 1 or row[f"window_{M}_us"] < row[f"one_row_x{M}_us"])
    result["sampler"] = row
    print("sampler", json.dumps(row), flush=True)


def _prompt(model, prompt_len):
    g = torch.Generator(device="cpu").manual_seed(1234)
    return torch.randint(0, model.config.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to("cuda")


def step(result, prompt_len=2048, top_k=200, temperature=0.8):
    from generate.base import SamplerRNG
    from lit_gpt.runtime import DecodeGraph, WindowDecodeGraph

    model = _model(prompt_len, 64)
    prompt = _prompt(model, prompt_len)
    with torch.inference_mode():
        model(prompt.view(1, -1), torch.arange(prompt_len, device="cuda"), last_token_only=True)
        first = prompt[:1].clone()
        dg = DecodeGraph(model, first, prompt_len)
        row = {"one_row_step_us": _replay_us(dg.graph)}
        ex = WindowDecodeGraph(model, first, prompt_len)
        for M in range(1, model.MAX_WINDOW + 1):
            ex.pos.fill_(prompt_len)
            ex.step([1] * (M - 1))  # eager, then captured
            ex.pos.fill_(prompt_len)
            row[f"window_step_{M}_us"] = _replay_us(ex.graphs[M])
            row[f"ratio_{M}"] = row[f"window_step_{M}_us"] / row["one_row_step_us"]
        # the same under top-k sampling: the one-row sampled step, and the window step ending in spec_accept_sample
        sdg = DecodeGraph(model, first, prompt_len, temperature=temperature, top_k=top_k,
                          rng=SamplerRNG(first.device, seed=1234))
        row["one_row_sampled_step_us"] = _replay_us(sdg.graph)
        sex = WindowDecodeGraph(model, first, prompt_len, temperature=temperature, top_k=top_k,
                                rng=SamplerRNG(first.device, seed=1234))
        for M in range(1, model.MAX_WINDOW + 1):
            sex.pos.fill_(prompt_len)
            sex.step([1] * (M - 1))
            sex.pos.fill_(prompt_len)
            row[f"window_sampled_step_{M}_us"] = _replay_us(sex.graphs[M])
            row[f"sampled_minus_greedy_{M}_us"] = row[f"window_sampled_step_{M}_us"] - row[f"window_step_{M}_us"]
    result["step"] = row
    print("step", json.dumps(row), flush=True)


def kernels(out, skip_step, skip_attention=False):
    result = {"what": "us, median of 7 graph replays; attention: per launch over 32 distinct caches, one_row_xM = M "
                      "back-to-back one-row launches on one cache; sampler: per lga_spec_accept_sample call over 32 "
                      "distinct logits, one_row_xM = M back-to-back lga_sample_topk launches; step: synthetic "
                      "Llama-2-7B int4-g128 at p = 2048",
              "library": os.environ.get("LGA_LIB", "default build"), "attention": {}}
    if not skip_attention:
        attention(result)
    sampler(result)
    if not skip_step:
        step(result)
    _write(out, result)


def e2e(out, prompt_len, steps, temperature=0.0, top_k=None):
    from generate.base import SamplerRNG, generate
    from generate.speculative import ModelDrafter, ScriptedDrafter, generate_speculative

    sampling = temperature > 0.0

    def kw():  # greedy, or sampling with one seed (a fresh counter per run)
        if not sampling:
            return dict(temperature=0.0)
        return dict(temperature=temperature, top_k=top_k, rng=SamplerRNG(torch.device("cuda"), seed=1234))

    model = _model(prompt_len, steps)
    prompt = _prompt(model, prompt_len)
    V = model.config.vocab_size
    new = steps + 1

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, y

    def measure(fn_full, fn_pre):
        fn_full()
        pre = statistics.median(timed(fn_pre)[0] for _ in range(3))
        full = [timed(fn_full)[0] for _ in range(3)]
        dec = statistics.median(full) - pre
        return {"prefill_s": pre, "decode_s": dec, "tokens_per_s": steps / dec}

    ref = generate(model, prompt, prompt_len + new, **kw()).tolist()
    mode = f"top-k sampling (temperature {temperature}, top_k {top_k}, one seed)" if sampling else "greedy"
    result = {"what": f"synthetic Llama-2-7B int4-g128, {mode}; decode time = run(steps + 1 tokens) - run(1 token), "
                      "median of 3 after a warm-up; acceptance forced by a scripted drafter"
                      + (", or reached by an nf4 twin of the target as ModelDrafter (synthetic weights: says nothing "
                         "about trained checkpoints)" if sampling else ""),
              "prompt_len": prompt_len, "steps": steps, "rows": []}
    base = measure(lambda: generate(model, prompt, prompt_len + new, **kw()),
                   lambda: generate(model, prompt, prompt_len + 1, **kw()))
    result["generate"] = base
    print("generate", json.dumps(base), flush=True)

    class Timed:  # the scripted tokens, with a draft model's drafting time spent for them
        def __init__(self, scripted, md):
            self.scripted, self.md = scripted, md

        def begin(self, prompt, first):
            self.scripted.begin(prompt, first)
            self.md.begin(prompt, first)

        def propose(self, tokens, k):
            self.md.propose(tokens, k)
            return self.scripted.propose(tokens, k)

    # greedy: a 4-layer draft model's drafting time; sampling: the target's nf4 twin as the drafter itself
    draft_model = _model(prompt_len, steps, quantize="nf4") if sampling else _model(prompt_len, steps, n_layer=4)
    for gamma in (1, 3, 7):
        half = gamma // 2
        patterns = {"0%": lambda rnd, i: True, "50%": lambda rnd, i: i == half + (rnd % 2) * (gamma % 2),
                    "100%": lambda rnd, i: False}
        extra = ([("nf4 twin, coupled", None), ("nf4 twin, uncoupled", None)] if sampling
                 else [("100% + 4-layer draft model", patterns["100%"])])
        for label, wrong in list(patterns.items()) + extra:
            def drafter():
                if wrong is None:
                    return ModelDrafter(draft_model, coupled="uncoupled" not in label)
                d = ScriptedDrafter(ref, wrong, V)
                return Timed(d, ModelDrafter(draft_model)) if "draft model" in label else d

            stats = {}
            y = generate_speculative(model, prompt, prompt_len + new, drafter(), speculate=gamma, stats=stats, **kw())
            assert y.tolist() == ref, (gamma, label)
            row = measure(lambda: generate_speculative(model, prompt, prompt_len + new, drafter(), speculate=gamma,
                                                       **kw()),
                          lambda: generate_speculative(model, prompt, prompt_len + 1, drafter(), speculate=gamma,
                                                       **kw()))
            row.update(gamma=gamma, forced=label, rounds=stats["rounds"], proposed=stats["proposed"],
                       accepted=stats["accepted"], tokens_per_pass=stats["tokens"] / stats["rounds"],
                       speedup=row["tokens_per_s"] / base["tokens_per_s"])
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
    _write(out, result)


def _write(out, result):
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("kernels", "e2e"))
    p.add_argument("--out", default=None)
    p.add_argument("--prompt_len", type=int, default=2048)
    p.add_argument("--steps", type=int, default=255)
    p.add_argument("--skip_step", action="store_true", help="kernels: the attention launches only (with LGA_LIB set "
                                                            "to a lab build, e.g. -DLGA_ATTN_WIN_NT=1: the load-hint A/B)")
    p.add_argument("--skip_attention", action="store_true", help="kernels: leave the attention table out")
    p.add_argument("--temperature", type=float, default=0.0, help="e2e: > 0 measures under top-k sampling")
    p.add_argument("--top_k", type=int, default=None, help="e2e: with --temperature, 1..1024")
    a = p.parse_args()
    if a.temperature > 0.0 and (a.top_k is None or not 1 <= a.top_k <= 1024):
        p.error("--temperature > 0 needs --top_k in 1..1024")
    if not torch.cuda.is_available():
        sys.exit("spec_decode.py measures on the GPU; there is none here")
    if a.mode == "kernels":
        kernels(a.out, a.skip_step, a.skip_attention)
    else:
        e2e(a.out, a.prompt_len, a.steps, a.temperature, a.top_k)
