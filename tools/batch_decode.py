"""Batched decode measurements: what a second, fourth or eighth sequence costs.

usage: python tools/batch_decode.py kernels [--out FILE.json]
           per-Linear launch times of the Llama-2-7B int4-g128 decode Linears (qkv, attn.proj, fc_1||fc_2, mlp.proj,
           lm_head): the one-row lga_q4_gemv*, the rows launch at M = 2, 4, 8, and the MFMA prefill GEMM
           (q4_gemm_fused / q4_gemm_swiglu, with the separate RMSNorm it needs) at the same M. Each figure is the
           median over 7 replays of one graph of back-to-back launches over distinct weight copies (> 1 GB per
           graph, so no copy is served from the MALL), in one process. Prints the two criteria per shape and M:
           rows(M) < M x one-row and rows(M) < GEMM(M).
       python tools/batch_decode.py e2e [--batches 1,2,4] [--prompt_len 2048] [--steps 255] [--out FILE.json]
           synthetic Llama-2-7B int4-g128, greedy: aggregate decode tokens/s of generate (B = 1) and generate_batch
           (B > 1), the prefill excluded (timed apart), median of 3 runs after one warm-up run per B.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

# name: (N, K, dual, fused norm, residual)
SHAPES = {"qkv": (12288, 4096, False, True, False), "attn.proj": (4096, 4096, False, False, True),
          "fc_1||fc_2": (11008, 4096, True, True, False), "mlp.proj": (4096, 11008, False, False, True),
          "lm_head": (32000, 4096, False, True, False)}
ROWS = (2, 4, 8)
GROUP, FMT = 128, 0


def _median_us(run, launches, reps=7):
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e3 / launches)
    return statistics.median(times)


def kernels(out):
    dev = torch.device("cuda")
    result = {"what": "us per launch, median of 7 graph replays over distinct weight copies", "shapes": {}}
    ok = True
    for name, (N, K, dual, norm, res) in SHAPES.items():
        copies = max(4, int(1.0e9 // (N * K // 2 * (2 if dual else 1))))
        mats = [tuple(ops.quantize(torch.randn(N, K, device=dev) * 0.02, FMT, GROUP) for _ in range(2 if dual else 1))
                for _ in range(copies)]
        x = torch.randn(max(ROWS), K, device=dev).bfloat16()
        nw = torch.ones(K, device=dev).bfloat16() if norm else None
        r = torch.randn(max(ROWS), N, device=dev).bfloat16() if res else None
        y = torch.empty(max(ROWS), N, device=dev, dtype=torch.bfloat16)

        def one_row():
            for m in mats:
                if dual:
                    ops.q4_gemv_swiglu(x[0], *m[0], *m[1], N, K, GROUP, FMT, norm_weight=nw, out=y[0])
                else:
                    ops.q4_gemv(x[0], *m[0], N, K, GROUP, FMT, norm_weight=nw, residual=None if r is None else r[0],
                                out=y[0])

        def rows(M):
            def run():
                for m in mats:
                    if dual:
                        ops.q4_gemv_swiglu_rows(x[:M], *m[0], *m[1], N, K, GROUP, FMT, norm_weight=nw, out=y[:M])
                    else:
                        ops.q4_gemv_rows(x[:M], *m[0], N, K, GROUP, FMT, norm_weight=nw,
                                         residual=None if r is None else r[:M], out=y[:M])
            return run

        def gemm(M):
            fits = ops.q4f_fits(M, N, K, GROUP, FMT)
            if dual and not fits:
                return None
            one = ops.q4_gemm_fused if fits else ops.q4_gemm  # QuantLinear.gemm's choice

            def run():  # what today's multi-row route costs: the RMSNorm apart, then the MFMA GEMM
                for m in mats:
                    xin = x[:M] if nw is None else ops.rmsnorm(x[:M], nw, 1e-5)
                    if dual:
                        ops.q4_gemm_swiglu(xin, *m[0], *m[1], N, K, GROUP, FMT, out=y[:M])
                    else:
                        one(xin, *m[0], N, K, GROUP, FMT, residual=None if r is None else r[:M], out=y[:M])
            return run

        row = {"N": N, "K": K, "dual": dual, "copies": copies, "one_row_us": _median_us(one_row, copies)}
        for M in ROWS:
            row[f"rows_{M}_us"] = _median_us(rows(M), copies)
            g = gemm(M)
            row[f"gemm_{M}_us"] = None if g is None else _median_us(g, copies)
            c1 = row[f"rows_{M}_us"] < M * row["one_row_us"]
            c2 = row[f"gemm_{M}_us"] is None or row[f"rows_{M}_us"] < row[f"gemm_{M}_us"]
            row[f"ok_{M}"] = bool(c1 and c2)
            ok = ok and c1 and c2
        result["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        del mats
        torch.cuda.empty_cache()
    result["all_criteria_hold"] = bool(ok)
    _write(out, result)


def e2e(out, batches, prompt_len, steps):
    from generate.base import build_model, generate, generate_batch
    from lit_gpt import Config

    dev = torch.device("cuda")
    cfg = Config.from_name("Llama-2-7b-hf")
    model = build_model(cfg, quantize="int4-g128", device=dev, max_seq_length=prompt_len + steps + 1)
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompts = [torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to(dev)
               for _ in range(max(batches))]
    new = steps + 1  # the prefill's token + `steps` decode steps

    def run(B, n_new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if B == 1:
            ys = [generate(model, prompts[0], prompt_len + n_new, temperature=0.0)]
        else:
            ys = generate_batch(model, prompts[:B], n_new, temperature=0.0)
        torch.cuda.synchronize()
        assert all(y.numel() == prompt_len + n_new for y in ys)
        return time.perf_counter() - t0

    result = {"what": "synthetic Llama-2-7B int4-g128, greedy; decode time = run(steps + 1 tokens) - run(1 token), "
                      "median of 3 after a warm-up run", "prompt_len": prompt_len, "steps": steps, "batches": {}}
    for B in batches:
        model.set_kv_cache(batch_size=B, device=dev)
        run(B, new)
        pre = statistics.median(run(B, 1) for _ in range(3))
        full = [run(B, new) for _ in range(3)]
        dec = [t - pre for t in full]
        row = {"prefill_s": pre, "decode_s": statistics.median(dec), "decode_s_runs": dec,
               "tokens_per_s": B * steps / statistics.median(dec),
               "tokens_per_s_with_prefill": B * new / statistics.median(full)}
        result["batches"][str(B)] = row
        print(B, json.dumps(row), flush=True)
    rates = [result["batches"][str(B)]["tokens_per_s"] for B in batches]
    result["rises_with_B"] = all(b > a for a, b in zip(rates, rates[1:]))
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
    p.add_argument("--batches", default="1,2,4")
    p.add_argument("--prompt_len", type=int, default=2048)
    p.add_argument("--steps", type=int, default=255)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("batch_decode.py measures on the GPU; there is none here")
    if a.mode == "kernels":
        kernels(a.out)
    else:
        e2e(a.out, [int(b) for b in a.batches.split(",")], a.prompt_len, a.steps)
