"""fp8-g128 multi-row decode GEMV measurements.

usage: python tools/fp8_rows_decode.py [--out FILE.json]
    us per launch on the five Llama-2-7B decode Linears (tools/batch_decode.py's SHAPES) at M = 2, 4, 8: ONE
    lga_fp8_gemv(_swiglu)_rows launch, M one-row lga_fp8_gemv(_swiglu) launches, and lga_fp8_gemm at M rows with the
    lga_rmsnorm it needs (fc_1 || fc_2: two GEMMs and lga_swiglu, what Fp8Linear runs for several rows). Per shape and
    M one graph per variant of back-to-back launches over distinct weight copies (> 1 GB, so none is served from the
    last-level cache); the three graphs are replayed alternately, 9 times each, device events around each replay;
    median and min..max are reported, and whether rows(M) is below each of the others beyond the spread.
    (End to end: python tools/batch_decode.py e2e --quantize fp8-g128.)
"""
import argparse
import json
import sys

import torch

from batch_decode import ROWS, SHAPES, _alternate_us, _write, ops


def kernels(out):
    dev = torch.device("cuda")
    result = {"what": "us per unit (one rows launch / M one-row launches / GEMM + norm at M rows): median, min, max of "
                      "9 alternated graph replays over distinct weight copies", "shapes": {}}
    for name, (N, K, dual, norm, res) in SHAPES.items():
        copies = max(4, int(1.0e9 // (N * K * (2 if dual else 1))))
        mats = [tuple(t for _ in range(2 if dual else 1) for t in ops.fp8_quantize(torch.randn(N, K, device=dev) * 0.02))
                for _ in range(copies)]
        x = torch.randn(max(ROWS), K, device=dev).bfloat16()
        nw = torch.ones(K, device=dev).bfloat16() if norm else None
        r = torch.randn(max(ROWS), N, device=dev).bfloat16() if res else None
        y = torch.empty(max(ROWS), N, device=dev, dtype=torch.bfloat16)
        y2 = torch.empty(max(ROWS), N, device=dev, dtype=torch.bfloat16)
        row = {"N": N, "K": K, "dual": dual, "copies": copies}
        for M in ROWS:
            def rows():
                for m in mats:
                    if dual:
                        ops.fp8_gemv_swiglu_rows(x[:M], *m, norm_weight=nw, out=y[:M])
                    else:
                        ops.fp8_gemv_rows(x[:M], *m, norm_weight=nw, residual=None if r is None else r[:M], out=y[:M])

            def one_row():
                for m in mats:
                    for i in range(M):
                        if dual:
                            ops.fp8_gemv_swiglu(x[i], *m, norm_weight=nw, out=y[i])
                        else:
                            ops.fp8_gemv(x[i], *m, norm_weight=nw, residual=None if r is None else r[i], out=y[i])

            def gemm():
                for m in mats:
                    xin = x[:M] if nw is None else ops.rmsnorm(x[:M], nw, 1e-5)
                    if dual:
                        ops.swiglu(ops.fp8_gemm(xin, m[0], m[1], out=y[:M]), ops.fp8_gemm(xin, m[2], m[3], out=y2[:M]))
                    else:
                        ops.fp8_gemm(xin, *m, residual=None if r is None else r[:M], out=y[:M])

            graphs = {}
            for k, fn in (("rows", rows), ("one_row_x_M", one_row), ("gemm", gemm)):
                fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                graphs[k] = g
            t = _alternate_us(graphs, copies)
            t["rows_below_one_row_x_M"] = bool(t["rows"]["max_us"] < t["one_row_x_M"]["min_us"])
            t["rows_below_gemm"] = bool(t["rows"]["max_us"] < t["gemm"]["min_us"])
            row[f"M{M}"] = t
            del graphs
        result["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        del mats
        torch.cuda.empty_cache()
    result["criterion_M2_M4_all_shapes"] = bool(all(s[f"M{M}"]["rows_below_one_row_x_M"]
                                                    for s in result["shapes"].values() for M in (2, 4)))
    _write(out, result)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_rows_decode.py measures on the GPU; there is none here")
    kernels(a.out)
