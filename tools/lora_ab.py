"""A/B of the LoRA kernels at the Llama-2-7B shapes (the LoRA section; output kept as profiles/lora_ab.txt).

Decode: an adapted Linear is the base GEMV (int4-g128, lga_q4_gemv) followed by ONE lga_lora_gemv. Timed per Linear:
the base GEMV alone with its fusions (qkv: RMSNorm prologue; mlp.proj: residual epilogue), the base GEMV + lga_lora_gemv
(the norm / residual then ride the adapter launch), and the base GEMV + the adapter as four torch ops (two matmuls, a
multiply, an add; the norm / residual stay in the base launch, which favours this side). The adapter's cost is the
difference to the base alone. ``--groups`` sweeps the rows a workgroup of lga_lora_gemv owns (LGA_LORA_GROUPS).
Prefill: lga_q4_gemm_fused alone against + lga_lora_down + lga_lora_up at 2048 rows.
Model: decode tokens/s of the synthetic Llama-2-7B in int4-g128 with and without a q + v adapter of rank 8.

Method (as tools/int8_ab.py): every kind runs as one captured graph of back-to-back Linears over distinct weight copies
(about 1 GB per graph, so no launch finds its weights in the 256 MB last-level cache); the kinds alternate inside each
of ROUNDS rounds, timed with device events; reported per Linear: median over the rounds, and the minimum.

``--rows`` (several adapters per batch, profiles/lora_rows_ab.txt) replaces the above by two measurements. Per launch:
one lga_lora_gemv_rows at M = 1, 2, 4 rows (every row another adapter of a stacked set of four) against the M one-row
lga_lora_gemv launches it replaces, by the same method: graphs of 32 back-to-back launches over distinct adapter sets
(one per layer of the model, all L2-resident as in a decode step), the kinds alternating. End to end: the synthetic
Llama-2-7B in int4-g128, four 512-token prompts with four different rank-8 q + v adapters, 256 new tokens each —
generate_batch at B = 4 against the same four requests served one after another on the single path (select(i) +
generate), interleaved over three repetitions, and the adapter-free B = 4 rate of the same session.

usage: python tools/lora_ab.py [--rounds 7] [--groups 32,64,128,256] [--no-prefill] [--no-model]
       python tools/lora_ab.py --rows [--rounds 7] [--no-model]
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

# name: (N, K, r, segments, fusion of the base launch)
SHAPES = {"qkv r8": (12288, 4096, 8, 2, "norm"), "qkv r64": (12288, 4096, 64, 2, "norm"),
          "mlp.proj r8": (4096, 11008, 8, 1, "res")}
GROUP = 128
REPLAYS = 8


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


def q4_weight(N, K, dev):
    return (torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8),
            (torch.rand(N, K // GROUP, device=dev) * 0.01 + 0.001).bfloat16())


def adapter(N, K, r, segs, dev):
    """(A, B, row_off, dense B (N, R) for the torch composition): qkv rows dealt q, k (no adapter), v per 128-row head."""
    A = (torch.randn(r * segs, K, device=dev) * K ** -0.5).bfloat16()
    B = (torch.randn(N, r, device=dev) * 0.05).bfloat16()
    if segs == 1:
        return A, B, None, B
    head = (torch.arange(N, device=dev) // 128) % 3
    off = torch.where(head == 0, 0, torch.where(head == 2, r, -1)).to(torch.int32)
    dense = torch.zeros(N, r * segs, device=dev, dtype=torch.bfloat16)
    for s, h in enumerate((0, 2)):
        dense[head == h, s * r:(s + 1) * r] = B[head == h]
    return A, B, off, dense


def report(title, t, copies, order):
    med = {k: statistics.median(v) for k, v in t.items()}
    cells = "".join(f" {med[k]:8.2f} ({min(t[k]):6.2f})" for k in order)
    extra = "".join(f" {med[k] - med[order[0]]:+8.2f}" for k in order[1:])
    print(f"{title}{cells}  |{extra}", flush=True)


def decode(rounds, dev, groups):
    print("decode, us per Linear: median (min) over %d alternating rounds | adapter cost = difference to the base" % rounds)
    kinds = ["base"] + [f"lora g{g}" if g else "lora" for g in groups] + ["torch x4"]
    print(f"{'shape':12s} {'N x K':>14s}" + "".join(f" {k:>17s}" for k in kinds))
    for name, (N, K, r, segs, fusion) in SHAPES.items():
        x = torch.randn(K, device=dev).bfloat16()
        nw = torch.ones(K, device=dev).bfloat16()
        res = torch.randn(N, device=dev).bfloat16()
        y = torch.empty(N, device=dev, dtype=torch.bfloat16)
        A, B, off, dense = adapter(N, K, r, segs, dev)
        scaling = 16.0 / r
        n = max(4, int(1.0e9 // (N * K * 0.5)))
        mats = [q4_weight(N, K, dev) for _ in range(n)]
        fused = {"norm_weight": nw} if fusion == "norm" else {"residual": res}

        def base():
            for qw, sc in mats:
                ops.q4_gemv(x, qw, sc, N, K, GROUP, 0, out=y, **fused)

        def lora():
            for qw, sc in mats:
                ops.q4_gemv(x, qw, sc, N, K, GROUP, 0, out=y, norm_weight=fused.get("norm_weight"))
                ops.lora_gemv(x, A, B, off, scaling, base=y, out=y, **fused)

        xn = ops.rmsnorm(x.view(1, -1), nw, 1e-5).view(-1) if fusion == "norm" else x

        def torch4():
            for qw, sc in mats:
                ops.q4_gemv(x, qw, sc, N, K, GROUP, 0, out=y, **fused)
                y.add_(((xn @ A.T) @ dense.T) * scaling)

        graphs = {"base": capture(base)}
        for g in groups:
            if g:
                os.environ["LGA_LORA_GROUPS"] = str(g)
            graphs[f"lora g{g}" if g else "lora"] = capture(lora)  # the grid is fixed at capture
            os.environ.pop("LGA_LORA_GROUPS", None)
        graphs["torch x4"] = capture(torch4)
        t = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, g in graphs.items():
                t[k].append(timed(g) / n)
        report(f"{name:12s} {N:>7d}x{K:<6d}", t, n, kinds)
        del graphs, mats
        torch.cuda.empty_cache()


def prefill(rounds, dev, M=2048):
    print(f"prefill at {M} rows, us per Linear: median (min) | adapter cost")
    print(f"{'shape':12s} {'N x K':>14s} {'q4_gemm_fused':>17s} {'+ down + up':>17s}")
    for name, (N, K, r, segs, _) in SHAPES.items():
        x = torch.randn(M, K, device=dev).bfloat16()
        res = torch.randn(M, N, device=dev).bfloat16()
        qw, sc = q4_weight(N, K, dev)
        A, B, off, _ = adapter(N, K, r, segs, dev)
        y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        t_buf = torch.empty(M, r * segs, device=dev, dtype=torch.bfloat16)
        reps = 4

        def base():
            for _ in range(reps):
                ops.q4_gemm_fused(x, qw, sc, N, K, GROUP, 0, residual=res, out=y)

        def lora():
            for _ in range(reps):
                ops.q4_gemm_fused(x, qw, sc, N, K, GROUP, 0, out=y)
                ops.lora_down(x, A, out=t_buf)
                ops.lora_up(t_buf, B, off, 16.0 / r, base=y, residual=res, out=y)

        graphs = {"base": capture(base), "lora": capture(lora)}
        t = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, g in graphs.items():
                t[k].append(timed(g) / reps)
        report(f"{name:12s} {N:>7d}x{K:<6d}", t, reps, ["base", "lora"])


@torch.inference_mode()
def model(dev, steps=256):
    from generate.base import build_model
    from lit_gpt import lora
    from lit_gpt.runtime import DecodeGraph

    cfg = lora.Config.from_name("Llama-2-7b-hf", r=8, alpha=16, to_query=True, to_value=True)
    T = 16
    m = build_model(cfg, quantize="int4-g128", device=dev, max_seq_length=T + steps + 64)
    prompt = torch.randint(0, cfg.vocab_size, (1, T), device=dev, dtype=torch.int32)

    def rate():
        for b in m.transformer.h:
            b.attn.kv_cache.reset_parameters()
        logits = m(prompt, torch.arange(T, device=dev), last_token_only=True)
        dg = DecodeGraph(m, logits.reshape(-1).argmax().view(1), T, chunk=8)
        out = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps // 8):
                dg.steps()
            torch.cuda.synchronize()
            out.append(steps / (time.perf_counter() - t0))
        return out

    plain = rate()
    lora.attach(m, lora.random_adapter(cfg), cfg)
    adapted = rate()
    n = sum(isinstance(x, lora.LoraLinear) for x in m.modules())
    ms = [1e3 / statistics.median(v) for v in (plain, adapted)]
    print(f"Llama-2-7B int4-g128 decode, {steps} steps x 3, tokens/s: without adapter "
          f"{statistics.median(plain):.1f} ({ms[0]:.3f} ms/step), with a q + v rank-8 adapter on {n} Linears "
          f"{statistics.median(adapted):.1f} ({ms[1]:.3f} ms/step): +{(ms[1] - ms[0]) * 1e3 / n:.2f} us per adapted Linear")


def rows_launch(rounds, dev, layers=32, n_adapters=4):
    print("several adapters per batch, us per launch site: median (min) over %d alternating rounds | rows - M x one-row"
          % rounds)
    print(f"{'shape':12s} {'N x K':>14s} {'M':>2s} {'M x lora_gemv':>17s} {'lora_gemv_rows':>17s}")
    for name in ("qkv r8", "mlp.proj r8"):
        N, K, r, segs, fusion = SHAPES[name]
        nw = torch.ones(K, device=dev).bfloat16()
        sets = []
        for _ in range(layers):
            parts = [adapter(N, K, r, segs, dev) for _ in range(n_adapters)]
            sets.append((torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), parts[0][2]))
        scaling = 16.0 / r
        for M in (1, 2, 4):
            x = torch.randn(M, K, device=dev).bfloat16()
            res = torch.randn(M, N, device=dev).bfloat16()
            y = torch.randn(M, N, device=dev).bfloat16()
            ids = torch.arange(M, device=dev, dtype=torch.int32)
            fused = {"norm_weight": nw} if fusion == "norm" else {"residual": res}

            def one_row():
                for A, B, off in sets:
                    for m in range(M):
                        kw = {"norm_weight": nw} if fusion == "norm" else {"residual": res[m]}
                        ops.lora_gemv(x[m], A[m], B[m], off, scaling, base=y[m], out=y[m], **kw)

            def rows():
                for A, B, off in sets:
                    ops.lora_gemv_rows(x, A, B, off, ids, scaling, base=y, out=y, **fused)

            graphs = {"one-row": capture(one_row), "rows": capture(rows)}
            t = {k: [] for k in graphs}
            for _ in range(rounds):
                for k, g in graphs.items():
                    t[k].append(timed(g) / layers)
            report(f"{name:12s} {N:>7d}x{K:<6d} {M:>2d}", t, layers, ["one-row", "rows"])
            spread = {k: (max(v) - min(v)) for k, v in t.items()}
            print(f"{'':32s}run-to-run spread (max - min): one-row {spread['one-row']:.2f}, rows {spread['rows']:.2f}")
        del sets
        torch.cuda.empty_cache()


@torch.inference_mode()
def rows_model(dev, T=512, new=256, reps=3):
    from generate.base import build_model, generate, generate_batch
    from lit_gpt import lora

    cfg = lora.Config.from_name("Llama-2-7b-hf", r=8, alpha=16, to_query=True, to_value=True)
    m = build_model(cfg, quantize="int4-g128", device=dev, max_seq_length=T + new)
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, cfg.vocab_size, (T,), generator=g, dtype=torch.int32).to(dev) for _ in range(4)]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def batch(adapters, n):
        m.set_kv_cache(batch_size=4, device=dev)
        generate_batch(m, prompts, n, temperature=0.0, **({} if adapters is None else {"adapters": adapters}))

    def sequential(n):
        m.set_kv_cache(batch_size=1, device=dev)
        for i, p in enumerate(prompts):
            m.lora_adapters.select(i)
            generate(m, p, T + n, temperature=0.0)
        m.lora_adapters.select(None)

    def decode_rate(fn):  # decode tokens/s: the call's time beyond the same call stopped after the prefill's token
        return 4 * (new - 1) / (wall(lambda: fn(new)) - wall(lambda: fn(1)))

    batch(None, 8)  # warm-up
    plain = [decode_rate(lambda n: batch(None, n)) for _ in range(reps)]
    lora.attach_many(m, [lora.random_adapter(cfg, seed=1234 + i) for i in range(4)], cfg)
    batch([0, 1, 2, 3], 8)
    sequential(8)
    rates = {"batch": [], "sequential": [], "batch, no row adapted": []}
    for _ in range(reps):
        rates["batch"].append(decode_rate(lambda n: batch([0, 1, 2, 3], n)))
        rates["sequential"].append(decode_rate(sequential))
        rates["batch, no row adapted"].append(decode_rate(lambda n: batch([None] * 4, n)))
    print(f"Llama-2-7B int4-g128, 4 x {T}-token prompts, {new} new tokens each, four rank-8 q + v adapters; aggregate "
          f"decode tokens/s, {reps} interleaved repetitions: median (min .. max)")
    rows = [("adapter-free model, generate_batch B = 4", plain),
            ("four adapters, generate_batch B = 4", rates["batch"]),
            ("four adapters, one after another (select + generate)", rates["sequential"]),
            ("adapter set attached, B = 4, every row without adapter", rates["batch, no row adapted"])]
    for title, v in rows:
        print(f"  {title:56s} {statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--groups", default="0", help="comma-separated LGA_LORA_GROUPS values to sweep (0: the heuristic)")
    ap.add_argument("--no-prefill", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--rows", action="store_true", help="several adapters per batch: lga_lora_gemv_rows against M "
                                                        "one-row launches, and generate_batch against sequential service")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lora_ab.py measures on the GPU; no device found")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    ops.load_library()
    print(torch.cuda.get_device_name(0))
    if a.rows:
        rows_launch(a.rounds, dev)
        if not a.no_model:
            rows_model(dev)
        sys.exit(0)
    decode(a.rounds, dev, [int(g) for g in a.groups.split(",")])
    if not a.no_prefill:
        prefill(a.rounds, dev)
    if not a.no_model:
        model(dev)
