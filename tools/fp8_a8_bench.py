"""--quantize fp8-g128-a8 measurements, the way tools/mxfp4_a8_bench.py measures mxfp4-a8.

usage: python tools/fp8_a8_bench.py gemm | e2e [--out FILE.json]
    gemm  lga_mx8_quantize + lga_fp8_a8_gemm (the pair Fp8A8Linear.gemm launches; the quantizer alone beside it) against
          lga_fp8_gemm at M = 2048 and M = 64 on the five Llama-2-7B Linears, with lga_bf16_gemm and the mxfp4-a8 pair
          in the same session: per side one graph of back-to-back launches over weight copies that together exceed the
          256 MB last-level cache (at least 8), the graphs replayed alternately, 9 times each, device events around
          each replay. us per launch: median, min, max.
    e2e   synthetic Llama-2-7B, 2048-token prompt, 255 greedy steps under graph replay: bf16, fp8-g128 and fp8-g128-a8
          models held together and run in turn, three rounds after a warm-up of each (tools/mxfp4_bench.py e2e's
          method).
"""
import argparse
import json
import statistics
import sys
import time

import torch

from batch_decode import _write, ops
from mxfp4_bench import _alternate, _capture

SHAPES = {"qkv": (12288, 4096), "attn.proj": (4096, 4096), "fc_1": (11008, 4096), "mlp.proj": (4096, 11008),
          "lm_head": (32000, 4096)}
LLC_BYTES = 256 << 20


def gemm(out):
    dev = torch.device("cuda")
    result = {"what": "us per launch: median, min, max of 9 alternated graph replays over `copies` weight copies; "
                      "a8_pair = lga_mx8_quantize + lga_fp8_a8_gemm, mxfp4_a8_pair = lga_mx8_quantize + "
                      "lga_mxfp4_a8_gemm, mx8_quantize = the quantizer alone; clears_margin: fp8_gemm median - a8_pair "
                      "median exceeds the larger of the two sides' max - min", "shapes": {}}
    for name, (N, K) in SHAPES.items():
        w = torch.randn(N, K, device=dev) * 0.02
        n = max(8, -(-LLC_BYTES // (N * K)) + 1)  # the fp8 copies alone exceed the cache
        f8 = ops.fp8_quantize(w)
        m4 = ops.mxfp4_quantize(w)
        mats = {"fp8": [tuple(t.clone() for t in f8) for _ in range(n)],
                "mxfp4": [tuple(t.clone() for t in m4) for _ in range(n)],
                "bf16": [w.bfloat16() for _ in range(n)]}
        row = {"N": N, "K": K, "copies": n}
        for M in (64, 2048):
            x = torch.randn(M, K, device=dev).bfloat16()
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            ws = ops.mx8_quantize(x)

            def parent():
                for m in mats["fp8"]:
                    ops.fp8_gemm(x, *m, out=y)

            def pair():
                for m in mats["fp8"]:
                    ops.fp8_a8_gemm(*ops.mx8_quantize(x, out=ws), *m, out=y)

            def quant():
                for _ in mats["fp8"]:
                    ops.mx8_quantize(x, out=ws)

            def bf16():
                for m in mats["bf16"]:
                    ops.bf16_gemm(x, m, out=y)

            def mx4_pair():
                for m in mats["mxfp4"]:
                    ops.mxfp4_a8_gemm(*ops.mx8_quantize(x, out=ws), *m, out=y)

            t = _alternate({"fp8_gemm": (_capture(parent), n), "a8_pair": (_capture(pair), n),
                            "mx8_quantize": (_capture(quant), n), "bf16_gemm": (_capture(bf16), n),
                            "mxfp4_a8_pair": (_capture(mx4_pair), n)})
            for k in ("fp8_gemm", "a8_pair", "bf16_gemm", "mxfp4_a8_pair"):
                t[k]["tflops"] = 2.0 * M * N * K / (t[k]["median_us"] * 1e-6) / 1e12
            t["pair_over_parent"] = t["a8_pair"]["median_us"] / t["fp8_gemm"]["median_us"]
            spread = max(t[k]["max_us"] - t[k]["min_us"] for k in ("fp8_gemm", "a8_pair"))
            t["clears_margin"] = t["fp8_gemm"]["median_us"] - t["a8_pair"]["median_us"] > spread
            row[f"M{M}"] = t
        result["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        del mats
        torch.cuda.empty_cache()
    _write(out, result)


def e2e(out, prompt_len=2048, steps=255):
    from generate.base import build_model, generate
    from lit_gpt import Config

    dev = torch.device("cuda")
    cfg = Config.from_name("Llama-2-7b-hf")
    models = {str(q or "bf16"): build_model(cfg, quantize=q, device=dev, max_seq_length=prompt_len + steps + 1)
              for q in (None, "fp8-g128", "fp8-g128-a8")}
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompt = torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to(dev)

    def run(model, n_new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = generate(model, prompt, prompt_len + n_new, temperature=0.0)
        torch.cuda.synchronize()
        assert y.numel() == prompt_len + n_new
        return time.perf_counter() - t0

    pre, full = {k: [] for k in models}, {k: [] for k in models}
    for m in models.values():
        m.set_kv_cache(batch_size=1, device=dev)
        run(m, steps + 1)
    for _ in range(3):
        for k, m in models.items():
            pre[k].append(run(m, 1))
            full[k].append(run(m, steps + 1))
    result = {"what": f"synthetic Llama-2-7B, {prompt_len}-token prompt, {steps} greedy steps, graph replay; three "
                      "models in turn, 3 rounds after a warm-up; decode = whole call - prefill-only call", "modes": {}}
    for k in models:
        dec = [f - p for f, p in zip(full[k], pre[k])]
        result["modes"][k] = {"decode_tokens_per_s": steps / statistics.median(dec),
                              "decode_tokens_per_s_runs": [steps / d for d in dec],
                              "prefill_ms": statistics.median(pre[k]) * 1e3,
                              "prefill_ms_runs": [p * 1e3 for p in pre[k]]}
        print(k, json.dumps(result["modes"][k]), flush=True)
    _write(out, result)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("gemm", "e2e"))
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_a8_bench.py measures on the GPU; there is none here")
    {"gemm": gemm, "e2e": e2e}[a.mode](a.out)
