"""fp8 vs bf16 KV cache, interleaved A/B in ONE process (box-to-box spread is larger than the effects).

usage: python tools/kv8_bench.py kernels [--out FILE.json]
           per-launch us of the fused decode attention, bf16 cache vs fp8 cache, at the Llama-2-7B geometry (p = 2047
           of S = 2304), the Llama-2-70B geometry (64 heads, 8 groups, p = 2303) and Mixtral's (32 heads, 8 groups,
           p = 32066 of S = 32768). Per geometry and format: 32 launches over 32 distinct caches (no launch re-reads
           what another left in the MALL) captured in one HIP graph, replayed 10 times per round; the rounds alternate
           the two formats so drift hits both. Median over the rounds, the K/V stream rate and its share of 8 TB/s.
       python tools/kv8_bench.py e2e [--prompt_len 2048] [--steps 255] [--out FILE.json]
           synthetic Llama-2-7B int4-g128 after a 2048-token prompt, greedy: decode tokens/s at B = 1 and B = 4, the
           prefill ms (the fp8 figure carries the dequantize detour) and the resident cache GB, with each cache. The
           two caches alternate run by run on one model object.
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

FP8 = torch.float8_e4m3fn
HS = 128
GEOMETRIES = {"llama-2-7b": (32, 32, 2304, 2047), "llama-2-70b": (64, 8, 2304, 2303),
              "mixtral-8x7b": (32, 8, 32768, 32066)}
LAYERS, REPLAYS, ROUNDS = 32, 10, 7


def _fp8_cache(G, S, dev):
    """Random codes below the NaN pattern with per-row scales 2^-8 .. 2^-4 (values of a few units at most)."""
    codes = [torch.randint(0, 0x7E, (G, S, HS), device=dev, dtype=torch.uint8) |
             (torch.randint(0, 2, (G, S, HS), device=dev, dtype=torch.uint8) << 7) for _ in range(2)]
    scales = [torch.exp2(-torch.randint(4, 9, (G, S), device=dev).float()) for _ in range(2)]
    return codes[0], codes[1], scales[0], scales[1]


def kernels(out):
    dev = torch.device("cuda")
    result = {"what": f"us per fused decode-attention launch: median of {ROUNDS} alternating rounds of {REPLAYS} "
                      f"replays of a graph of {LAYERS} launches over distinct caches", "geometries": {}}
    for name, (H, G, S, p) in GEOMETRIES.items():
        splits = ops.decode_splits(G, H // G, HS, S)
        qkv = torch.randn(1, (H + 2 * G) * HS, device=dev).bfloat16()
        cos, sin = torch.randn(S, HS, device=dev), torch.randn(S, HS, device=dev)
        pos = torch.tensor([p], device=dev)
        y = torch.empty(1, H * HS, device=dev, dtype=torch.bfloat16)
        bf = [(torch.randn(G, S, HS, device=dev).bfloat16(), torch.randn(G, S, HS, device=dev).bfloat16())
              for _ in range(LAYERS)]
        f8 = [_fp8_cache(G, S, dev) for _ in range(LAYERS)]
        ws = ops.AttentionWorkspace(1, H, G, HS, splits, dev)

        def run_bf16():
            for kc, vc in bf:
                ops.attention_decode_fused(qkv, kc, vc, pos, pos, cos, sin, H, G, HS, HS, 1 / math.sqrt(HS), splits,
                                           workspace=ws, out=y)

        def run_fp8():
            for cache in f8:
                ops.attention_decode_fused_kv8(qkv, cache, pos, pos, cos, sin, H, G, HS, HS, 1 / math.sqrt(HS), splits,
                                               workspace=ws, out=y)

        graphs = {}
        for fmt, run in (("bf16", run_bf16), ("fp8", run_fp8)):
            run()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run()
            g.replay()
            torch.cuda.synchronize()
            graphs[fmt] = g
        times = {"bf16": [], "fp8": []}
        for _ in range(ROUNDS):
            for fmt, g in graphs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(REPLAYS):
                    g.replay()
                e.record()
                e.synchronize()
                times[fmt].append(s.elapsed_time(e) * 1e3 / (REPLAYS * LAYERS))
        row = {"n_head": H, "n_query_groups": G, "max_seq": S, "position": p, "splits": splits}
        for fmt, row_bytes in (("bf16", 2 * HS), ("fp8", HS + 4)):
            us = statistics.median(times[fmt])
            kv_bytes = 2 * G * row_bytes * (p + 1)
            row[fmt] = {"us": us, "us_min": min(times[fmt]), "us_max": max(times[fmt]), "kv_bytes": kv_bytes,
                        "stream_GBps": kv_bytes / us / 1e3, "of_8TBps": kv_bytes / us / 1e3 / 8000}
        row["fp8_over_bf16"] = row["fp8"]["us"] / row["bf16"]["us"]
        result["geometries"][name] = row
        print(name, json.dumps(row), flush=True)
        del bf, f8
        torch.cuda.empty_cache()
    _write(out, result)


def e2e(out, prompt_len, steps):
    from generate.base import build_model, generate, generate_batch
    from lit_gpt import Config

    dev = torch.device("cuda")
    cfg = Config.from_name("Llama-2-7b-hf")
    model = build_model(cfg, quantize="int4-g128", device=dev, max_seq_length=prompt_len + steps + 1)
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompts = [torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to(dev)
               for _ in range(4)]
    new = steps + 1  # the prefill's token + `steps` decode steps

    def run(B, n_new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if B == 1:
            generate(model, prompts[0], prompt_len + n_new, temperature=0.0)
        else:
            generate_batch(model, prompts[:B], n_new, temperature=0.0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def prefill_ms():
        pos = torch.arange(prompt_len, device=dev)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        model(prompts[0].view(1, -1), pos, last_token_only=True)
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    result = {"what": "synthetic Llama-2-7B int4-g128, greedy; decode time = run(steps + 1 tokens) - run(1 token); "
                      "medians of 3 runs per cache, the caches alternating run by run after a warm-up run of each",
              "prompt_len": prompt_len, "steps": steps, "batches": {}}
    formats = (("bf16", None), ("fp8", FP8))
    for B in (1, 4):
        pre, full, pf, gb = ({k: [] for k, _ in formats} for _ in range(4))
        for rnd in range(4):  # round 0 warms up
            for fmt, dt in formats:
                model.set_kv_cache(batch_size=B, device=dev, dtype=dt)
                t1, tn, ms = run(B, 1), run(B, new), prefill_ms()
                if rnd:
                    pre[fmt].append(t1)
                    full[fmt].append(tn)
                    pf[fmt].append(ms)
                    gb[fmt] = sum(b.numel() * b.element_size() for blk in model.transformer.h
                                  for b in blk.attn.kv_cache.buffers()) / 1e9
        row = {}
        for fmt, _ in formats:
            dec = statistics.median(full[fmt]) - statistics.median(pre[fmt])
            row[fmt] = {"tokens_per_s": B * steps / dec, "decode_s": dec, "prefill_ms_one_sequence":
                        statistics.median(pf[fmt]), "cache_GB": gb[fmt]}
        row["fp8_over_bf16_tokens_per_s"] = row["fp8"]["tokens_per_s"] / row["bf16"]["tokens_per_s"]
        result["batches"][str(B)] = row
        print(B, json.dumps(row), flush=True)
    _write(out, result)


def _write(out, result):
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "e2e"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--prompt_len", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=255)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kv8_bench.py measures on the GPU; there is none here")
    if a.mode == "kernels":
        kernels(a.out)
    else:
        e2e(a.out, a.prompt_len, a.steps)
