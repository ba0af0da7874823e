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
           --attn both: every B > 1 twice in the same process, alternated run by run — the one-launch batch attention
           (lit_gpt.model.batch_attention) and the per-sequence loop (LGA_BATCH_ATTN=0, the previous behaviour).
       python tools/batch_decode.py attn [--out FILE.json]
           DESIGN §4.5e (a): us per block of ONE lga_attention_decode_batch launch at B = 2, 4, 8 against B
           per-sequence lga_attention_decode_fused launches, Llama-2-7B (H = G = 32, S = 2304, p around 2047) and
           Mixtral (H = 32, G = 8, S = 32768, p around 32066) geometries, bf16 and fp8 caches. One graph of 32 launches
           (32 x B for the loop) over distinct cache copies per form, so K / V comes from HBM; the two graphs are
           replayed alternately, 9 times each, device events around each replay; median and min..max are reported.
       python tools/batch_decode.py attn --shared [--out FILE.json]
           DESIGN §4.5f: us per block of ONE lga_attention_decode_shared launch against ONE lga_attention_decode_batch
           launch, B = 2, 4 samples behind a 2048-token prefix at p = 2048, 2175, 2302 (S = 2304), Llama-2-7B (H = G =
           32) and one GQA geometry (H = 32, G = 8). Same method: graphs of 32 launches over distinct cache copies,
           replayed alternately 9 times each. Prints the rule for generate_samples(share="auto").
       python tools/batch_decode.py samples [--samples 4] [--prompt_len 2048] [--steps 255] [--out FILE.json]
           DESIGN §4.5f: N samples of one prompt end to end, synthetic Llama-2-7B int4-g128, greedy: generate_samples
           with share=True, with share=False, and generate_batch([prompt] * N) (one prefill per sample), alternated run
           by run, 3 runs each after a warm-up of each. Wall time with the prefill, and decode tokens/s with the
           prefill-only run of each route subtracted.
       python tools/batch_decode.py continuous [--out FILE.json]
           DESIGN §4.5e (c): 16 synthetic requests (Llama-2-7B int4-g128, 512-token prompts, budgets from a fixed list
           spanning 32..256) through 4 slots with generate_continuous against the same requests through
           generate_batch in waves of 4 in arrival order (a wave runs to its longest budget). Prefill included; the
           two are alternated, 3 runs each after a warm-up of each.
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


def _alternate_us(graphs, per_replay, reps=9):
    """Replay the graphs in turn, ``reps`` rounds, device events around each replay: per graph the us per unit."""
    times = {k: [] for k in graphs}
    for k, g in graphs.items():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e3 / per_replay)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


ATTN_GEOMS = {"llama-2-7b": (32, 32, 2304, 2047), "mixtral": (32, 8, 32768, 32066)}  # H, G, S, position of row 0
ATTN_BLOCKS = 32  # launches (blocks) per graph replay


def attn(out):
    import math

    dev = torch.device("cuda")
    hs, slots = 128, 8
    result = {"what": "us per block: one lga_attention_decode_batch launch vs B per-sequence "
                      "lga_attention_decode_fused launches; graphs of 32 blocks over distinct cache copies, replayed "
                      "alternately 9 times each, device events around each replay", "cases": {}}
    for gname, (H, G, S, p0) in ATTN_GEOMS.items():
        n_splits = ops.decode_splits(G, H // G, hs, S)
        cos = torch.randn(S, hs, device=dev)
        sin = torch.randn(S, hs, device=dev)
        qkv = torch.randn(slots, (H + 2 * G) * hs, device=dev).bfloat16()
        for fp8 in (False, True):
            one = slots * G * S * hs * (1 if fp8 else 2) * 2  # bytes of one (k, v) copy of all slots
            copies = max(2, min(ATTN_BLOCKS, int(3.0e9 // one)))
            caches = []
            for _ in range(copies):
                if fp8:
                    kc, vc = (torch.randint(0, 0x78, (slots, G, S, hs), device=dev, dtype=torch.uint8) for _ in "kv")
                    caches.append((kc, vc, torch.ones(slots, G, S, device=dev), torch.ones(slots, G, S, device=dev)))
                else:
                    caches.append(tuple(torch.randn(slots, G, S, hs, device=dev).bfloat16() for _ in "kv"))
            ws1 = ops.AttentionWorkspace(1, H, G, hs, n_splits, dev)
            for B in ROWS:
                pos = torch.tensor([p0 - 37 * b for b in range(B)], device=dev)  # positions differ per sequence
                posv = [pos[b:b + 1] for b in range(B)]
                wsB = ops.AttentionWorkspace(B, H, G, hs, n_splits, dev)
                y = torch.empty(B, H * hs, device=dev, dtype=torch.bfloat16)
                q = qkv[:B].contiguous()
                rows = [q[b:b + 1] for b in range(B)]
                sc = 1.0 / math.sqrt(hs)

                def batch():
                    for i in range(ATTN_BLOCKS):
                        c = caches[i % copies]
                        if fp8:
                            ops.attention_decode_batch_kv8(q, c, pos, cos, sin, H, G, hs, hs, sc, n_splits,
                                                           workspace=wsB, out=y)
                        else:
                            ops.attention_decode_batch(q, c[0], c[1], pos, cos, sin, H, G, hs, hs, sc, n_splits,
                                                       workspace=wsB, out=y)

                def loop():
                    for i in range(ATTN_BLOCKS):
                        c = caches[i % copies]
                        for b in range(B):
                            if fp8:
                                ops.attention_decode_fused_kv8(rows[b], tuple(t[b] for t in c), posv[b], posv[b], cos,
                                                               sin, H, G, hs, hs, sc, n_splits, workspace=ws1,
                                                               out=y[b:b + 1])
                            else:
                                ops.attention_decode_fused(rows[b], c[0][b], c[1][b], posv[b], posv[b], cos, sin, H, G,
                                                           hs, hs, sc, n_splits, workspace=ws1, out=y[b:b + 1])

                graphs = {}
                for name, fn in (("batch", batch), ("loop", loop)):
                    fn()
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        fn()
                    graphs[name] = g
                row = _alternate_us(graphs, ATTN_BLOCKS)
                row.update(n_splits=n_splits, copies=copies,
                           batch_faster_beyond_spread=bool(row["batch"]["max_us"] < row["loop"]["min_us"]))
                key = f"{gname}/{'fp8' if fp8 else 'bf16'}/B{B}"
                result["cases"][key] = row
                print(key, json.dumps(row), flush=True)
                del graphs
            del caches
            torch.cuda.empty_cache()
    c = result["cases"]
    result["batch_is_default_by_rule"] = bool(c["llama-2-7b/bf16/B2"]["batch_faster_beyond_spread"]
                                              and c["llama-2-7b/bf16/B4"]["batch_faster_beyond_spread"])
    _write(out, result)


SHARED_GEOMS = {"llama-2-7b": (32, 32), "gqa-32x8": (32, 8)}  # H, G
SHARED_S, SHARED_P, SHARED_POS = 2304, 2048, (2048, 2175, 2302)


def attn_shared(out):
    import math

    dev = torch.device("cuda")
    hs, slots, S = 128, 4, SHARED_S
    sc = 1.0 / math.sqrt(hs)
    result = {"what": "us per block: one lga_attention_decode_shared launch vs one lga_attention_decode_batch launch, "
                      f"B samples at one position p behind a {SHARED_P}-token prefix, S = {S}; graphs of 32 blocks "
                      "over distinct cache copies, replayed alternately 9 times each, device events around each replay",
              "cases": {}}
    for gname, (H, G) in SHARED_GEOMS.items():
        n_splits = ops.decode_splits(G, H // G, hs, S)
        cos = torch.randn(S, hs, device=dev)
        sin = torch.randn(S, hs, device=dev)
        qkv = torch.randn(slots, (H + 2 * G) * hs, device=dev).bfloat16()
        one = slots * G * S * hs * 2 * 2  # bytes of one (k, v) copy of all slots
        copies = max(2, min(ATTN_BLOCKS, int(3.0e9 // one)))
        caches = [tuple(torch.randn(slots, G, S, hs, device=dev).bfloat16() for _ in "kv") for _ in range(copies)]
        pre = torch.tensor([SHARED_P], device=dev)
        for B in (2, 4):
            ws = ops.AttentionWorkspace(B, H, G, hs, n_splits, dev)
            y = torch.empty(B, H * hs, device=dev, dtype=torch.bfloat16)
            q = qkv[:B].contiguous()
            for p in SHARED_POS:
                pos1 = torch.tensor([p], device=dev)
                posB = torch.full((B,), p, device=dev)

                def shared():
                    for i in range(ATTN_BLOCKS):
                        c = caches[i % copies]
                        ops.attention_decode_shared(q, c[0], c[1], pos1, pre, cos, sin, H, G, hs, hs, sc, n_splits,
                                                    workspace=ws, out=y)

                def batch():
                    for i in range(ATTN_BLOCKS):
                        c = caches[i % copies]
                        ops.attention_decode_batch(q, c[0], c[1], posB, cos, sin, H, G, hs, hs, sc, n_splits,
                                                   workspace=ws, out=y)

                graphs = {}
                for name, fn in (("shared", shared), ("batch", batch)):
                    fn()
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        fn()
                    graphs[name] = g
                row = _alternate_us(graphs, ATTN_BLOCKS)
                row.update(n_splits=n_splits, copies=copies,
                           shared_faster_beyond_spread=bool(row["shared"]["max_us"] < row["batch"]["min_us"]))
                key = f"{gname}/B{B}/p{p}"
                result["cases"][key] = row
                print(key, json.dumps(row), flush=True)
                del graphs
        del caches
        torch.cuda.empty_cache()
    c = result["cases"]
    result["auto_picks_shared_by_rule"] = bool(all(c[f"llama-2-7b/B{B}/p{p}"]["shared_faster_beyond_spread"]
                                                   for B in (2, 4) for p in SHARED_POS))
    _write(out, result)


def samples(out, n, prompt_len, steps):
    from generate.base import build_model, generate_batch, generate_samples
    from lit_gpt import Config

    dev = torch.device("cuda")
    cfg = Config.from_name("Llama-2-7b-hf")
    model = build_model(cfg, quantize="int4-g128", device=dev, max_seq_length=prompt_len + steps + 1)
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompt = torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to(dev)
    model.set_kv_cache(batch_size=min(n, 4), device=dev)
    routes = {"share_true": lambda new: generate_samples(model, prompt, new, n, temperature=0.0, share=True),
              "share_false": lambda new: generate_samples(model, prompt, new, n, temperature=0.0, share=False),
              "generate_batch": lambda new: [y for i in range(0, n, 4)
                                             for y in generate_batch(model, [prompt] * min(4, n - i), new,
                                                                     temperature=0.0)]}

    def timed(fn, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ys = fn(new)
        torch.cuda.synchronize()
        assert len(ys) == n and all(y.numel() == prompt_len + new for y in ys)
        return time.perf_counter() - t0, ys

    ref = None
    for name, fn in routes.items():  # warm-up of each; the three routes give the same tokens
        _, ys = timed(fn, steps + 1)
        ref = ref or ys
        assert all(torch.equal(a, b) for a, b in zip(ys, ref)), name
    full = {k: [] for k in routes}
    pre = {k: [] for k in routes}
    for _ in range(3):
        for name, fn in routes.items():
            full[name].append(timed(fn, steps + 1)[0])
            pre[name].append(timed(fn, 1)[0])
    result = {"what": f"{n} samples of one {prompt_len}-token prompt, {steps} decode steps, synthetic Llama-2-7B "
                      "int4-g128, greedy; the three routes alternated run by run, 3 runs each after a warm-up of each; "
                      "wall_s includes the prefill(s); decode = wall - the route's run of 1 new token",
              "samples": n, "prompt_len": prompt_len, "steps": steps, "routes": {}}
    for name in routes:
        dec = [a - b for a, b in zip(full[name], pre[name])]
        result["routes"][name] = {"wall_s_runs": full[name], "wall_s_median": statistics.median(full[name]),
                                  "prefill_s_median": statistics.median(pre[name]), "decode_s_runs": dec,
                                  "decode_tokens_per_s": n * steps / statistics.median(dec)}
        print(name, json.dumps(result["routes"][name]), flush=True)
    _write(out, result)


CONT_BUDGETS = (256, 32, 64, 48, 128, 32, 96, 224, 40, 192, 32, 80, 160, 56, 112, 32)  # arrival order


def continuous(out, prompt_len=512, slots=4):
    from generate.base import build_model, generate_batch, generate_continuous
    from lit_gpt import Config

    dev = torch.device("cuda")
    cfg = Config.from_name("Llama-2-7b-hf")
    model = build_model(cfg, quantize="int4-g128", device=dev, max_seq_length=prompt_len + max(CONT_BUDGETS))
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompts = [torch.randint(0, cfg.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to(dev)
               for _ in CONT_BUDGETS]
    total = sum(CONT_BUDGETS)

    def cont():
        ys = generate_continuous(model, prompts, list(CONT_BUDGETS), batch_size=slots, temperature=0.0)
        assert [y.numel() - prompt_len for y in ys] == list(CONT_BUDGETS)

    def waves():
        for i in range(0, len(prompts), slots):
            generate_batch(model, prompts[i:i + slots], max(CONT_BUDGETS[i:i + slots]), temperature=0.0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    model.set_kv_cache(batch_size=slots, device=dev)
    runs = {"continuous": [], "waves": []}
    cont()
    waves()
    for _ in range(3):
        runs["continuous"].append(timed(cont))
        runs["waves"].append(timed(waves))
    result = {"what": f"{len(prompts)} requests, {prompt_len}-token prompts, budgets {list(CONT_BUDGETS)} "
                      f"({total} tokens), {slots} slots, greedy, prefill included; alternated, 3 runs each after a "
                      "warm-up of each; tokens/s counts the requested tokens only"}
    for k, v in runs.items():
        result[k] = {"seconds_runs": v, "seconds_median": statistics.median(v),
                     "tokens_per_s": total / statistics.median(v)}
    result["speedup"] = result["waves"]["seconds_median"] / result["continuous"]["seconds_median"]
    _write(out, result)


def e2e(out, batches, prompt_len, steps, attn_mode="default"):
    import lit_gpt.model as lm
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
    result["batch_attention_default"] = bool(lm.batch_attention)
    for B in batches:
        model.set_kv_cache(batch_size=B, device=dev)
        run(B, new)
        pre = statistics.median(run(B, 1) for _ in range(3))
        if attn_mode == "both" and B > 1:  # the two attention routes, alternated run by run
            default = lm.batch_attention
            lm.batch_attention = False
            run(B, new)  # warm-up of the loop's route
            full = {"batch": [], "loop": []}
            for _ in range(3):
                for name, on in (("batch", True), ("loop", False)):
                    lm.batch_attention = on
                    full[name].append(run(B, new))
            lm.batch_attention = default
            row = {"prefill_s": pre}
            for name, v in full.items():
                dec = [t - pre for t in v]
                row[name] = {"decode_s": statistics.median(dec), "decode_s_runs": dec,
                             "tokens_per_s": B * steps / statistics.median(dec)}
            row["tokens_per_s"] = row["batch" if default else "loop"]["tokens_per_s"]
            result["batches"][str(B)] = row
            print(B, json.dumps(row), flush=True)
            continue
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
    p.add_argument("mode", choices=("kernels", "e2e", "attn", "continuous", "samples"))
    p.add_argument("--shared", action="store_true", help="attn: the shared-prefix launch against the batch launch")
    p.add_argument("--samples", type=int, default=4, help="samples: samples of the one prompt")
    p.add_argument("--out", default=None)
    p.add_argument("--batches", default="1,2,4")
    p.add_argument("--prompt_len", type=int, default=2048)
    p.add_argument("--steps", type=int, default=255)
    p.add_argument("--attn", default="default", choices=("default", "both"),
                   help="e2e: 'both' alternates the batch attention launch and the per-sequence loop")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("batch_decode.py measures on the GPU; there is none here")
    if a.mode == "kernels":
        kernels(a.out)
    elif a.mode == "attn":
        (attn_shared if a.shared else attn)(a.out)
    elif a.mode == "samples":
        samples(a.out, a.samples, a.prompt_len, a.steps)
    elif a.mode == "continuous":
        continuous(a.out)
    else:
        e2e(a.out, [int(b) for b in a.batches.split(",")], a.prompt_len, a.steps, a.attn)
