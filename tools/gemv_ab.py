"""A/B of builds of the one-shot weight-stream decode GEMVs (bf16, int8 and mxfp4 on csrc/gemv_pass.h; fp8-g128 and the
fp8 rows kernels in csrc/gemv_fp8.hip) in ONE process. For a change that must not move a bit or a microsecond: build
the parent beside the tree (`git archive <rev> lit-gpt_amd include`, `make OUT=...`) and compare the two.

usage: AB_LIBS=parent.so,tree.so python tools/gemv_ab.py bits
           Every entry point — lga_bf16_gemv(_swiglu), lga_int8_gemv(_swiglu), lga_fp8_gemv(_swiglu)(_rows),
           lga_mxfp4_gemv(_swiglu) — on identical seeded inputs through each library, the raw 16-bit output patterns
           compared with torch.equal (the output buffer carries 8 sentinel rows past N, compared too). Exit status 1
           names the first differing case; a library against itself is the tool's own sanity check. The shapes are the
           smallest that reach every branch: N = 1, 5, 77 (rows past N in a wave at 1, 2, 4 and 8 rows per wave); K =
           the format's minimum (one chunk, every other lane clamped), 4096 (exactly one pass), 4096 + the format's K
           step (a second pass that is nearly all clamp), 11008 (three passes, the last partial), 12288 (the largest
           norm-fused K of fp8 and mxfp4), 16384 and 32768 (int8: 8192, its 8-chunk one-pass class, and 16384, its
           largest); epilogues none / norm / bias / residual / norm + bias + residual and SwiGLU with and without the
           norm, the norm wherever the class fuses it; int8 at threshold 0, threshold 6 with no outlier, 3 planted
           outlier columns and all columns outliers; the rows kernels at M = 1, 2, 3, 5, 8. A few seconds on one MI355X.
       AB_LIBS=parent.so,parent_copy.so,tree.so python tools/gemv_ab.py time [--out FILE.txt]
           The five Llama-2-7B decode Linears (tools/batch_decode.py's SHAPES with their fused norm / residual) in
           bf16, int8, fp8-g128 and mxfp4, and the fp8 rows kernels at M = 4 and 8. Per case and library one captured
           graph of back-to-back launches over distinct weight copies (> 1 GB, so none is served from the last-level
           cache); the three graphs are replayed alternately for 9 rounds, device events around each replay.
           parent_copy.so is a byte copy of parent.so: the largest relative gap between their medians over the cases
           is the noise floor of the session, and no case's tree median may exceed its parent median by more than
           that (exit status 1 lists the cases that do).
"""
import argparse
import os
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO), str(REPO / "tools")]

from lit_gpt import ops  # noqa: E402

NS = (1, 5, 77)
# format: (K step = minimum K, the Ks, largest K whose norm fuses)
KS = {"bf16": (8, (8, 4096, 4104, 11008, 12288, 16384, 32768), 32768),
      "int8": (16, (16, 4096, 4112, 8192, 11008, 12288, 16384), 16384),
      "fp8": (128, (128, 4096, 4224, 11008, 12288, 16384, 32768), 12288),
      "mxfp4": (32, (32, 4096, 4128, 11008, 12288, 16384, 32768), 12288)}
# (norm, bias, residual)
EPILOGUES = ((False, False, False), (True, False, False), (False, True, False), (False, False, True),
             (True, True, True))
ROWS_M = (1, 2, 3, 5, 8)
SENTINEL = 0x7B7B  # bf16 bits the kernels never leave behind by accident


def _quantize(fmt, w):
    if fmt == "bf16":
        return (w.bfloat16(),)
    return {"int8": ops.int8_quantize, "fp8": ops.fp8_quantize, "mxfp4": ops.mxfp4_quantize}[fmt](w)


def _gemv(fmt, x, wt, out, **kw):
    return {"bf16": ops.bf16_gemv, "int8": ops.int8_gemv, "fp8": ops.fp8_gemv, "mxfp4": ops.mxfp4_gemv}[fmt](
        x, *wt, out=out, **kw)


def _swiglu(fmt, x, w1, w2, out, **kw):
    return {"bf16": ops.bf16_gemv_swiglu, "int8": ops.int8_gemv_swiglu, "fp8": ops.fp8_gemv_swiglu,
            "mxfp4": ops.mxfp4_gemv_swiglu}[fmt](x, *w1, *w2, out=out, **kw)


def _int8_inputs(x, K, gen):
    """(name, x, threshold): no outlier test, none found, 3 planted columns, every column."""
    calm = x.clamp(-4.0, 4.0)
    planted = calm.clone()
    planted[..., torch.randperm(K, device=x.device, generator=gen)[:3]] = 8.0
    loud = torch.where(x >= 0, 7.0 + x.abs(), -7.0 - x.abs()).bfloat16()
    return (("thr=0", x, 0.0), ("thr=6 none", calm, 6.0), ("thr=6 3 columns", planted, 6.0), ("thr=6 all", loud, 6.0))


def bits():
    libs = os.environ["AB_LIBS"].split(",")
    if len(libs) != 2:
        sys.exit("AB_LIBS names two libraries")
    dev = torch.device("cuda")
    loaded = [ops.load_library(Path(p), strict=False) for p in libs]
    names, flags = [], []

    def both(name, run, rows, N):
        """run(out) through each library into a sentinel-filled (rows, N) + 8 buffer ((N,) + 8 for rows = None); the raw
        bits compared"""
        outs = []
        for lib in loaded:
            ops._lib = lib
            buf = torch.full(((rows or 1) * N + 8,), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)
            run(buf[:N] if rows is None else buf[:rows * N].view(rows, N))
            outs.append(buf.view(torch.int16))
        flags.append(torch.equal(outs[0], outs[1]))
        names.append(name)

    for fmt, (_, ks, norm_max) in KS.items():
        for K in ks:
            gen = torch.Generator(device=dev).manual_seed(K)
            ops._lib = loaded[0]  # (the quantizers are not under test: one set of weights for both libraries)
            w1, w2 = (_quantize(fmt, torch.randn(NS[-1], K, device=dev, generator=gen) * 0.05) for _ in range(2))
            x = torch.randn(8, K, device=dev, generator=gen).bfloat16()
            nw = (1.0 + 0.1 * torch.randn(K, device=dev, generator=gen)).bfloat16()
            bias = torch.randn(NS[-1], device=dev, generator=gen).bfloat16()
            resid = torch.randn(8, NS[-1], device=dev, generator=gen).bfloat16()
            variants = _int8_inputs(x, K, gen) if fmt == "int8" else (("", x, None),)
            for N in NS:
                a1, a2 = tuple(t[:N] for t in w1), tuple(t[:N] for t in w2)
                for tag, xv, thr in variants:
                    kw = {} if thr is None else {"threshold": thr}
                    for norm, b, r in EPILOGUES:
                        if norm and K > norm_max:
                            continue
                        both(f"{fmt} gemv N={N} K={K} norm={norm} bias={b} residual={r} {tag}",
                             lambda out: _gemv(fmt, xv[0], a1, out, norm_weight=nw if norm else None,
                                               bias=bias[:N] if b else None,
                                               residual=resid[0, :N] if r else None, **kw),
                             None, N)
                    for norm in (False, True):
                        if norm and K > norm_max:
                            continue
                        both(f"{fmt} gemv_swiglu N={N} K={K} norm={norm} {tag}",
                             lambda out: _swiglu(fmt, xv[0], a1, a2, out, norm_weight=nw if norm else None, **kw),
                             None, N)
                if fmt != "fp8":
                    continue
                for M in ROWS_M:
                    rs = resid[:M, :N].contiguous()
                    for norm, b, r in EPILOGUES:
                        if norm and K > norm_max:
                            continue
                        both(f"fp8 gemv_rows M={M} N={N} K={K} norm={norm} bias={b} residual={r}",
                             lambda out: ops.fp8_gemv_rows(x[:M], *a1, norm_weight=nw if norm else None,
                                                           bias=bias[:N] if b else None, residual=rs if r else None,
                                                           out=out), M, N)
                    for norm in (False, True):
                        if norm and K > norm_max:
                            continue
                        both(f"fp8 gemv_swiglu_rows M={M} N={N} K={K} norm={norm}",
                             lambda out: ops.fp8_gemv_swiglu_rows(x[:M], *a1, *a2, norm_weight=nw if norm else None,
                                                                  out=out), M, N)
        bad = [i for i, same in enumerate(flags) if not same]
        if bad:
            print(f"DIFFERENT BITS: {names[bad[0]]} ({len(bad)} of {len(flags)} cases so far differ)", flush=True)
            sys.exit(1)
        print(f"{fmt}: {len(flags)} cases so far, same bits", flush=True)
    print(f"{len(flags)} cases, {Path(libs[0]).name} == {Path(libs[1]).name} bit for bit")


def _alternate(graphs, reps=9):
    """graphs: name -> (graph, launches per replay). Replayed in turn; us per launch of every replay."""
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
    return times


def _capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def time_(out):
    from batch_decode import SHAPES

    libs = os.environ["AB_LIBS"].split(",")
    if len(libs) != 3:
        sys.exit("AB_LIBS names three libraries: parent, a byte copy of it, tree")
    dev = torch.device("cuda")
    loaded = dict(zip(("parent", "parent_copy", "tree"), (ops.load_library(Path(p), strict=False) for p in libs)))
    lines, rel_floor, results = [], 0.0, []
    for fmt, M in [(f, 1) for f in KS] + [("fp8", 4), ("fp8", 8)]:
        for name, (N, K, dual, norm, res) in SHAPES.items():
            nm = 2 if dual else 1
            ops._lib = loaded["parent"]
            ts = _quantize(fmt, torch.randn(N, K, device=dev) * 0.02)
            nbytes = sum(t.numel() * t.element_size() for t in ts) * nm
            copies = max(4, int(1.0e9 // nbytes) + 1)
            mats = [tuple(t.clone() for _ in range(nm) for t in ts) for _ in range(copies)]
            x = torch.randn(M, K, device=dev).bfloat16()
            x = x[0] if M == 1 else x
            nw = torch.ones(K, device=dev).bfloat16() if norm else None
            r = torch.randn(M, N, device=dev).bfloat16() if res else None
            r = r[0] if res and M == 1 else r
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            y = y[0] if M == 1 else y

            def run():
                for m in mats:
                    if M > 1 and dual:
                        ops.fp8_gemv_swiglu_rows(x, *m, norm_weight=nw, out=y)
                    elif M > 1:
                        ops.fp8_gemv_rows(x, *m, norm_weight=nw, residual=r, out=y)
                    elif dual:
                        _swiglu(fmt, x, m[:len(ts)], m[len(ts):], y, norm_weight=nw)
                    else:
                        _gemv(fmt, x, m, y, norm_weight=nw, residual=r)

            graphs = {}
            for k, lib in loaded.items():
                ops._lib = lib
                graphs[k] = (_capture(run), copies)
            t = _alternate(graphs)
            med = {k: statistics.median(v) for k, v in t.items()}
            rel_floor = max(rel_floor, abs(med["parent_copy"] - med["parent"]) / med["parent"])
            case = f"{fmt}{'' if M == 1 else f' rows M={M}'} {name}"
            results.append((case, med["parent"], med["tree"]))
            lines.append(f"{case:<28}" + "".join(
                f"  {k} {med[k]:8.2f} ({min(t[k]):.2f}..{max(t[k]):.2f})" for k in t))
            print(lines[-1], flush=True)
            del graphs, mats
            torch.cuda.empty_cache()
    over = [(c, p, tr) for c, p, tr in results if tr > p * (1.0 + rel_floor)]
    lines.append(f"noise floor (largest |parent_copy - parent| / parent over the cases): {100 * rel_floor:.2f} %")
    lines += [f"OVER THE FLOOR: {c}: tree {tr:.2f} us vs parent {p:.2f} us (+{100 * (tr / p - 1):.2f} %)"
              for c, p, tr in over] or ["no case's tree median exceeds its parent median by more than the floor"]
    print("\n".join(lines[-1 - max(1, len(over)):]))
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text("us per launch: median (min..max) of 9 alternated graph replays over distinct weight "
                             "copies (> 1 GB per graph)\n" + "\n".join(lines) + "\n")
    sys.exit(1 if over else 0)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("bits", "time"))
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gemv_ab.py runs on the GPU; there is none here")
    bits() if a.mode == "bits" else time_(a.out)
