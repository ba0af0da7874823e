"""MXFP6 weight measurements, the way tools/mxfp4_bench.py measures mxfp4.

usage: python tools/mxfp6_bench.py gemv | gemm | e2e [--out FILE.json]
    gemv  us per launch of the five Llama-2-7B decode Linears (with their fused norm / residual):
          lga_mxfp6_gemv(_swiglu) beside lga_fp8_gemv(_swiglu) and lga_mxfp4_gemv(_swiglu). Per format one graph of
          back-to-back launches over distinct weight copies (> 1 GB), replayed alternately 9 times; median, min..max,
          and the format's own weight bytes over the median as a fraction of 8 TB/s.
    gemm  lga_mxfp6_gemm beside lga_mxfp4_gemm and lga_fp8_gemm at M = 64 and 2048 on qkv, attn.proj, fc_1 and
          mlp.proj, the same way over 8 weight copies.
    e2e   synthetic Llama-2-7B, 2048-token prompt, 255 greedy steps under graph replay: bf16, fp8-g128, int4-g128,
          mxfp4 and mxfp6 models held together and run in turn (mxfp4_bench.e2e with the fifth mode).
"""
import argparse
import json
import sys

import torch

import mxfp4_bench
from batch_decode import SHAPES, _write, ops
from mxfp4_bench import PEAK, _alternate, _capture

GEMV = {"mxfp6": (ops.mxfp6_quantize, ops.mxfp6_gemv_swiglu, ops.mxfp6_gemv),
        "fp8-g128": (ops.fp8_quantize, ops.fp8_gemv_swiglu, ops.fp8_gemv),
        "mxfp4": (ops.mxfp4_quantize, ops.mxfp4_gemv_swiglu, ops.mxfp4_gemv)}
GEMM = {"mxfp6": (ops.mxfp6_quantize, ops.mxfp6_gemm), "mxfp4": (ops.mxfp4_quantize, ops.mxfp4_gemm),
        "fp8-g128": (ops.fp8_quantize, ops.fp8_gemm)}


def gemv(out):
    dev = torch.device("cuda")
    result = {"what": "us per launch: median, min, max of 9 alternated graph replays over distinct weight copies; "
                      "of_peak = the format's weight bytes / median / 8 TB/s", "shapes": {}}
    for name, (N, K, dual, norm, res) in SHAPES.items():
        nm = 2 if dual else 1
        w = torch.randn(N, K, device=dev) * 0.02
        x = torch.randn(K, device=dev).bfloat16()
        nw = torch.ones(K, device=dev).bfloat16() if norm else None
        r = torch.randn(N, device=dev).bfloat16() if res else None
        y = torch.empty(N, device=dev, dtype=torch.bfloat16)
        graphs, nbytes, keep = {}, {}, []  # keep: every format's copies live as long as the graphs that read them
        for fmt, (quantize, pair, one) in GEMV.items():
            ts = quantize(w)
            b = sum(t.numel() * t.element_size() for t in ts) * nm
            copies = max(4, int(1.0e9 // b))
            mats = [tuple(t.clone() for _ in range(nm) for t in ts) for _ in range(copies)]
            keep.append(mats)

            def run(mats=mats, pair=pair, one=one):
                for m in mats:
                    if dual:
                        pair(x, *m, norm_weight=nw, out=y)
                    else:
                        one(x, *m, norm_weight=nw, residual=r, out=y)

            graphs[fmt], nbytes[fmt] = (_capture(run), copies), b
        t = _alternate(graphs)
        for fmt in t:
            t[fmt]["weight_bytes"] = nbytes[fmt]
            t[fmt]["of_peak"] = nbytes[fmt] / (t[fmt]["median_us"] * 1e-6) / PEAK
        t["mxfp6_over_fp8_g128"] = t["mxfp6"]["median_us"] / t["fp8-g128"]["median_us"]
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
        row = {"N": N, "K": K}
        for M in (64, 2048):
            x = torch.randn(M, K, device=dev).bfloat16()
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            graphs, keep = {}, []
            for fmt, (quantize, fn) in GEMM.items():
                ts = quantize(w)
                mats = [tuple(t.clone() for t in ts) for _ in range(8)]
                keep.append(mats)

                def run(mats=mats, fn=fn):
                    for m in mats:
                        fn(x, *m, out=y)

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


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("gemv", "gemm", "e2e"))
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp6_bench.py measures on the GPU; there is none here")
    if a.mode == "e2e":
        mxfp4_bench.e2e(a.out, modes=(None, "fp8-g128", "int4-g128", "mxfp4", "mxfp6"))
    else:
        {"gemv": gemv, "gemm": gemm}[a.mode](a.out)
