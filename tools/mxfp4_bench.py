"""MXFP4 weight measurements.

usage: python tools/mxfp4_bench.py gemv | gemm | e2e [--out FILE.json]
    gemv  us per launch of the five Llama-2-7B decode Linears (tools/batch_decode.py's SHAPES, with their fused norm /
          residual): lga_mxfp4_gemv(_swiglu) beside lga_q4_gemv(_swiglu) at int4-g32 and lga_fp8_gemv(_swiglu). Per
          format one graph of back-to-back launches over distinct weight copies (> 1 GB, so none is served from the
          last-level cache); the graphs are replayed alternately, 9 times each, device events around each replay.
          Reported: median, min..max, and the format's own weight bytes over the median as a fraction of 8 TB/s.
    gemm  lga_mxfp4_gemm beside lga_fp8_gemm and the fused int4-g128 GEMM (lga_q4_gemm_fused) at M = 64 and 2048 on
          qkv, attn.proj, fc_1 and mlp.proj, the same way over 8 weight copies.
    e2e   synthetic Llama-2-7B, 2048-token prompt, 255 greedy steps under graph replay: bf16, fp8-g128, int4-g128 and
          mxfp4 models held together and run in turn, three rounds after a warm-up of each; decode rate = 255 / (whole
          call - prefill-only call), medians; Linear + embedding weight bytes.
"""
import argparse
import json
import statistics
import sys
import time

import torch

from batch_decode import SHAPES, _write, ops

PEAK = 8.0e12  # HBM bytes / s


def _alternate(graphs, reps=9):
    """graphs: name -> (graph, launches per replay). Replayed in turn; us per launch: median, min, max."""
    times = {k: [] for k in graphs}
    for g, _ in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, (g, n) in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e3 / n)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


def _capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def _formats(w):
    """One weight in the three formats: name -> (tensors, bytes)."""
    out = {"mxfp4": ops.mxfp4_quantize(w), "int4-g32": ops.quantize(w, 0, 32), "fp8-g128": ops.fp8_quantize(w)}
    return {k: (v, sum(t.numel() * t.element_size() for t in v)) for k, v in out.items()}


def gemv(out):
    dev = torch.device("cuda")
    result = {"what": "us per launch: median, min, max of 9 alternated graph replays over distinct weight copies; "
                      "of_peak = the format's weight bytes / median / 8 TB/s", "shapes": {}}
    for name, (N, K, dual, norm, res) in SHAPES.items():
        nm = 2 if dual else 1
        fm = _formats(torch.randn(N, K, device=dev) * 0.02)
        x = torch.randn(K, device=dev).bfloat16()
        nw = torch.ones(K, device=dev).bfloat16() if norm else None
        r = torch.randn(N, device=dev).bfloat16() if res else None
        y = torch.empty(N, device=dev, dtype=torch.bfloat16)
        graphs, nbytes, keep = {}, {}, []  # keep: every format's copies live as long as the graphs that read them
        for fmt, (ts, b) in fm.items():
            copies = max(4, int(1.0e9 // (b * nm)))
            mats = [tuple(t.clone() for _ in range(nm) for t in ts) for _ in range(copies)]
            keep.append(mats)
            one = {"mxfp4": (ops.mxfp4_gemv_swiglu, ops.mxfp4_gemv), "fp8-g128": (ops.fp8_gemv_swiglu, ops.fp8_gemv)}

            def run(mats=mats, fmt=fmt):
                for m in mats:
                    if fmt == "int4-g32" and dual:
                        ops.q4_gemv_swiglu(x, *m, N, K, 32, 0, norm_weight=nw, out=y)
                    elif fmt == "int4-g32":
                        ops.q4_gemv(x, *m, N, K, 32, 0, norm_weight=nw, residual=r, out=y)
                    elif dual:
                        one[fmt][0](x, *m, norm_weight=nw, out=y)
                    else:
                        one[fmt][1](x, *m, norm_weight=nw, residual=r, out=y)

            graphs[fmt], nbytes[fmt] = (_capture(run), copies), b * nm
        t = _alternate(graphs)
        for fmt in t:
            t[fmt]["weight_bytes"] = nbytes[fmt]
            t[fmt]["of_peak"] = nbytes[fmt] / (t[fmt]["median_us"] * 1e-6) / PEAK
        t["mxfp4_over_int4_g32"] = t["mxfp4"]["median_us"] / t["int4-g32"]["median_us"]
        result["shapes"][name] = dict(N=N, K=K, dual=dual, **t)
        print(name, json.dumps(result["shapes"][name]), flush=True)
        del graphs, mats, keep
        torch.cuda.empty_cache()
    _write(out, result)


def gemm(out):
    dev = torch.device("cuda")
    shapes = {"qkv": (12288, 4096), "attn.proj": (4096, 4096), "fc_1": (11008, 4096), "mlp.proj": (4096, 11008)}
    result = {"what": "us per launch and TFLOP/s: median (min, max) of 9 alternated graph replays over 8 weight copies",
              "shapes": {}}
    for name, (N, K) in shapes.items():
        w = torch.randn(N, K, device=dev) * 0.02
        fm = {"mxfp4": ops.mxfp4_quantize(w), "fp8-g128": ops.fp8_quantize(w), "int4-g128": ops.quantize(w, 0, 128)}
        row = {"N": N, "K": K}
        for M in (64, 2048):
            x = torch.randn(M, K, device=dev).bfloat16()
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            assert ops.q4f_fits(M, N, K, 128, 0)
            graphs, keep = {}, []  # keep: the copies live as long as the graphs that read them
            for fmt, ts in fm.items():
                mats = [tuple(t.clone() for t in ts) for _ in range(8)]
                keep.append(mats)

                def run(mats=mats, fmt=fmt):
                    for m in mats:
                        if fmt == "int4-g128":
                            ops.q4_gemm_fused(x, *m, N, K, 128, 0, out=y)
                        else:
                            (ops.mxfp4_gemm if fmt == "mxfp4" else ops.fp8_gemm)(x, *m, out=y)

                graphs[fmt] = (_capture(run), 8)
            t = _alternate(graphs)
            for fmt in t:
                t[fmt]["tflops"] = 2.0 * M * N * K / (t[fmt]["median_us"] * 1e-6) / 1e12
            row[f"M{M}"] = t
            del graphs, keep
        result["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    _write(out, result)


def e2e(out, prompt_len=2048, steps=255, modes=(None, "fp8-g128", "int4-g128", "mxfp4")):
    from generate.base import build_model, generate
    from lit_gpt import Config

    dev = torch.device("cuda")
    cfg = Config.from_name("Llama-2-7b-hf")
    models = {str(q or "bf16"): build_model(cfg, quantize=q, device=dev, max_seq_length=prompt_len + steps + 1)
              for q in modes}
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
    for k, m in models.items():
        m.set_kv_cache(batch_size=1, device=dev)
        run(m, steps + 1)
    for _ in range(3):
        for k, m in models.items():
            pre[k].append(run(m, 1))
            full[k].append(run(m, steps + 1))
    result = {"what": f"synthetic Llama-2-7B, {prompt_len}-token prompt, {steps} greedy steps, graph replay; the "
                      "models in turn, 3 rounds after a warm-up; decode = whole call - prefill-only call", "modes": {}}
    for k, m in models.items():
        dec = [f - p for f, p in zip(full[k], pre[k])]
        held = {id(t): t.numel() * t.element_size() for t in list(m.parameters()) + list(m.buffers())
                if t.ndim == 2 and t.shape[0] >= 4096}  # Linear weights / codes / scales and the embedding
        result["modes"][k] = {"decode_tokens_per_s": steps / statistics.median(dec),
                              "decode_tokens_per_s_runs": [steps / d for d in dec],
                              "prefill_ms": statistics.median(pre[k]) * 1e3,
                              "prefill_ms_runs": [p * 1e3 for p in pre[k]],
                              "weight_GB": sum(held.values()) / 1e9}
        print(k, json.dumps(result["modes"][k]), flush=True)
    _write(out, result)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("gemv", "gemm", "e2e"))
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp4_bench.py measures on the GPU; there is none here")
    {"gemv": gemv, "gemm": gemm, "e2e": e2e}[a.mode](a.out)
