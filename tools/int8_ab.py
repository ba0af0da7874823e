"""A/B of the bnb.int8 kernels at the Llama-2-7B shapes (the bnb.int8 section; output under profiles/).

Decode: per-launch time of ops.int8_gemv against ops.bf16_gemv (the yardstick: int8 reads half its bytes) and
ops.q4_gemv (int4-g128), each with the fusions its place in the decode step uses (qkv / lm_head: RMSNorm prologue,
attn.proj / mlp.proj: residual, fc: the dual SwiGLU form with the RMSNorm prologue).
Prefill: ops.int8_quantize_act + ops.int8_gemm against ops.q4_gemm_fused (int4-g128) at M = 2048 and M = 64.

Method: every kind runs as one captured graph of back-to-back launches over distinct weight copies (about 1 GB per
graph, so no launch finds its weights in the 256 MB last-level cache); the kinds alternate inside each of ROUNDS
rounds, timed with device events; reported per launch: median over the rounds, and the minimum.

usage: python tools/int8_ab.py [--rounds 7] [--no-prefill] [--shapes qkv,lm_head]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

# name: (N, K, dual, fusion)
SHAPES = {"qkv": (12288, 4096, False, "norm"), "attn.proj": (4096, 4096, False, "res"),
          "fc dual": (11008, 4096, True, "norm"), "mlp.proj": (4096, 11008, False, "res"),
          "lm_head": (32000, 4096, False, "norm")}
GROUP = 128


REPLAYS = 8  # graph replays per timed window (a few ms of device work)


def timed(graph):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPLAYS):
        graph.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / REPLAYS  # us per replay


def capture(run):
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g


def weights(kind, N, K, dev):
    if kind == "bf16":
        return (torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02,)
    if kind == "int8":
        return (torch.randint(-127, 128, (N, K), device=dev, dtype=torch.int8),
                torch.rand(N, device=dev, dtype=torch.float32) * 0.1 + 0.01)
    return (torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8),
            (torch.rand(N, K // GROUP, device=dev) * 0.01 + 0.001).bfloat16())


def decode(rounds, dev, only=None):
    print("decode GEMV, us per launch: median (min) over %d alternating rounds" % rounds)
    print(f"{'shape':10s} {'N x K':>14s} {'bf16':>16s} {'int8':>16s} {'int4-g128':>16s}  int8/bf16")
    for name, (N, K, dual, fusion) in SHAPES.items():
        if only and name not in only:
            continue
        x = torch.randn(K, device=dev).bfloat16()
        nw = torch.ones(K, device=dev).bfloat16()
        res = torch.randn(N, device=dev).bfloat16()
        y = torch.empty(N, device=dev, dtype=torch.bfloat16)
        # every captured launch reads its weights by address: the tensors must outlive the graphs (entering
        # torch.cuda.graph empties the allocator's cache, so weights that were garbage by then would be unmapped)
        graphs, copies, alive = {}, {}, []
        for kind, bpw in (("bf16", 2.0), ("int8", 1.0), ("q4", 0.5)):
            n = max(4, int(1.0e9 // (N * K * bpw * (2 if dual else 1))))
            mats = [(weights(kind, N, K, dev), weights(kind, N, K, dev) if dual else None) for _ in range(n)]
            kw = {"norm_weight": nw} if fusion == "norm" else {"residual": res}

            def run(kind=kind, mats=mats, kw=kw):
                for a, b in mats:
                    if kind == "bf16" and dual:
                        ops.bf16_gemv_swiglu(x, a[0], b[0], norm_weight=nw, out=y)
                    elif kind == "bf16":
                        ops.bf16_gemv(x, a[0], out=y, **kw)
                    elif kind == "int8" and dual:
                        ops.int8_gemv_swiglu(x, a[0], a[1], b[0], b[1], norm_weight=nw, out=y)
                    elif kind == "int8":
                        ops.int8_gemv(x, a[0], a[1], out=y, **kw)
                    elif dual:
                        ops.q4_gemv_swiglu(x, a[0], a[1], b[0], b[1], N, K, GROUP, 0, norm_weight=nw, out=y)
                    else:
                        ops.q4_gemv(x, a[0], a[1], N, K, GROUP, 0, out=y, **kw)

            alive.append(mats)
            graphs[kind], copies[kind] = capture(run), n
        t = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, g in graphs.items():
                t[k].append(timed(g) / copies[k])
        med = {k: statistics.median(v) for k, v in t.items()}
        cells = "".join(f" {med[k]:8.2f} ({min(t[k]):5.2f})" for k in ("bf16", "int8", "q4"))
        print(f"{name:10s} {N:>7d}x{K:<6d}{cells}  {med['int8'] / med['bf16']:.3f}", flush=True)
        del graphs, mats, alive
        torch.cuda.empty_cache()


def prefill(rounds, dev):
    print("prefill, us per Linear: median (min); int8 = int8_quantize_act + int8_gemm, int4 = q4_gemm_fused")
    print(f"{'shape':10s} {'M':>5s} {'N x K':>14s} {'int8':>20s} {'int4-g128':>20s}")
    for M in (2048, 64):
        for name, (N, K, dual, _) in SHAPES.items():
            x = torch.randn(M, K, device=dev).bfloat16()
            qw, sw = weights("int8", N, K, dev)
            q4, s4 = weights("q4", N, K, dev)
            reps = 4 if M == 2048 else 16

            def run8():
                for _ in range(reps):
                    xq, sx, cols, count, _f = ops.int8_quantize_act(x)
                    ops.int8_gemm(x, xq, sx, cols, count, qw, sw)

            def run4():
                for _ in range(reps):
                    ops.q4_gemm_fused(x, q4, s4, N, K, GROUP, 0)

            graphs = {"int8": capture(run8)}
            if ops.q4f_fits(M, N, K, GROUP, 0):
                graphs["q4"] = capture(run4)
            t = {k: [] for k in graphs}
            for _ in range(rounds):
                for k, g in graphs.items():
                    t[k].append(timed(g) / reps)
            cells = "".join(f" {statistics.median(t[k]):11.1f} ({min(t[k]):8.1f})" if k in t else f"{'-':>21s}"
                            for k in ("int8", "q4"))
            label = name.replace(" dual", " (one)")
            print(f"{label:10s} {M:>5d} {N:>7d}x{K:<6d}{cells}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-prefill", action="store_true")
    ap.add_argument("--shapes", default=None, help="comma-separated decode shapes (default: all)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("int8_ab.py measures on the GPU; no device found")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    ops.load_library()
    print(torch.cuda.get_device_name(0))
    decode(a.rounds, dev, a.shapes.split(",") if a.shapes else None)
    if not a.no_prefill:
        prefill(a.rounds, dev)
