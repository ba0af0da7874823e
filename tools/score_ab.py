"""Measurements of the scoring path (the scoring section; output kept as profiles/score_ab.txt).

Kernel: lga_token_logprobs against the torch chain it replaces on the same device tensor —
``log_softmax(logits.float(), -1)``, ``gather`` at the targets, ``argmax`` — at rows x n = 256 x 32000, 256 x 50304 and
2048 x 32000, with the kernel's share of 8 TB/s on the rows * n * 2 bytes it reads. lga_logits_kl is timed beside it
(two such matrices). Method (as tools/lora_ab.py): each kind runs as one captured graph of back-to-back calls over
distinct copies of the logits (more than 256 MB in all, so no call finds its input in the last-level cache); the kinds
alternate inside each of ROUNDS rounds, timed with device events; reported per call: median over the rounds, and the
minimum.

Model (``--model``): the synthetic Llama-2-7B (random init, seeded ids), 8192 tokens in windows of 2048 — what
``eval/perplexity.py --synthetic Llama-2-7b-hf --n_tokens 8192 --max_seq_length 2048`` runs: scored tokens per second
for int4-g128, the split of a window between the blocks and the head + reduction, and ``--against bf16`` for each
format (one bf16 model built once, then eval/perplexity.py's ``evaluate`` per format). Random weights: the figures
order the formats on this build's arithmetic; they are not the loss of a trained checkpoint.

usage: python tools/score_ab.py [--rounds 9] [--no-kernel] [--model] [--formats int4-g128,bnb.nf4,...]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

SHAPES = [(256, 32000), (256, 50304), (2048, 32000)]
HBM = 8e12


def capture(run):
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g


def timed(graph, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    graph.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls  # us per call


def kernel_ab(rounds):
    dev = torch.device("cuda", 0)
    print("kernel A/B: us per call, median (min) over", rounds, "rounds; share = rows*n*2 B / time / 8 TB/s")
    for rows, n in SHAPES:
        nbytes = rows * n * 2
        copies = max(3, -(-320 * 2 ** 20 // nbytes))
        xs = [(torch.randn(rows, n, device=dev) * 4).bfloat16() for _ in range(copies)]
        ys = [(torch.randn(rows, n, device=dev) * 4).bfloat16() for _ in range(copies)]
        t32 = torch.randint(0, n, (rows,), device=dev, dtype=torch.int32)
        t64 = t32.long().view(-1, 1)
        lp, am = torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)
        kl, ag = torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev)
        keep = []

        def hip():
            for x in xs:
                ops.token_logprobs(x, t32, logprob_out=lp, argmax_out=am)

        def chain():
            for x in xs:
                keep[:] = [torch.log_softmax(x.float(), -1).gather(1, t64), x.argmax(-1)]

        def klk():
            for x, y in zip(xs, ys):
                ops.logits_kl(x, y, kl_out=kl, agree_out=ag)

        graphs = {"lga_token_logprobs": capture(hip), "torch chain": capture(chain), "lga_logits_kl": capture(klk)}
        # same answers first
        hip()
        ref = torch.log_softmax(xs[-1].float(), -1).gather(1, t64).view(-1)
        assert float((lp - ref).abs().max()) < 1e-3 and torch.equal(am.long(), xs[-1].argmax(-1))
        times = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, g in graphs.items():
                times[k].append(timed(g, copies))
        print(f"rows {rows} x n {n} ({nbytes / 2 ** 20:.0f} MiB per call, {copies} copies)")
        for k, v in times.items():
            med = statistics.median(v)
            b = nbytes * (2 if k == "lga_logits_kl" else 1)
            print(f"  {k:20s} {med:9.1f} ({min(v):9.1f}) us   {b / (med * 1e-6) / HBM:6.1%} of 8 TB/s on its "
                  f"{b / 2 ** 20:.0f} MiB")
        print(f"  torch chain / kernel = {statistics.median(times['torch chain']) / statistics.median(times['lga_token_logprobs']):.2f}x")
        del graphs, xs, ys
        torch.cuda.empty_cache()


@torch.inference_mode()
def model_runs(formats, n_tokens, max_len):
    sys.path.insert(0, str(REPO / "lit-gpt_amd" / "eval"))
    import perplexity
    from generate.base import build_model
    from lit_gpt import Config, score

    dev = torch.device("cuda", 0)
    cfg = Config.from_name("Llama-2-7b-hf")
    g = torch.Generator(device="cpu").manual_seed(1234)
    ids = torch.randint(0, cfg.vocab_size, (n_tokens,), generator=g, dtype=torch.int64).tolist()
    print(f"model: synthetic Llama-2-7b-hf (random init), {n_tokens} seeded ids, windows of {max_len}")
    bf16 = build_model(cfg, quantize=None, device=dev, max_seq_length=max_len)
    for i, fmt in enumerate(formats):
        model = build_model(cfg, quantize=fmt, device=dev, max_seq_length=max_len)
        perplexity.evaluate(model, ids[:max_len], max_len=max_len, prefix_token=0)  # warm-up
        out = perplexity.evaluate(model, ids, max_len=max_len, prefix_token=0, against=bf16)
        print(f"{fmt} --against bf16: {json.dumps(out)}")
        if i == 0:  # the split of one full window: blocks (the no-cache forward) vs ln_f + lm_head + reduction
            window = [0] + ids[:max_len]
            t = torch.tensor(window)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for _ in range(2):
                ev[0].record()
                h = score._hidden(model, t, max_len, max_len)
                ev[1].record()
                tg = t[1:].to(device=dev, dtype=torch.int32)
                for a in range(0, max_len, score.HEAD_ROWS):
                    b = min(max_len, a + score.HEAD_ROWS)
                    ops.token_logprobs(score._head(model, h[a:b]), tg[a:b])
                ev[2].record()
                torch.cuda.synchronize()
            print(f"{fmt} one window of {max_len}: blocks {ev[0].elapsed_time(ev[1]):.1f} ms, head + reduction "
                  f"{ev[1].elapsed_time(ev[2]):.1f} ms")
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--no-kernel", action="store_true")
    p.add_argument("--model", action="store_true")
    p.add_argument("--formats", default="int4-g128,bnb.nf4,bnb.nf4-dq,bnb.fp4,bnb.int8")
    p.add_argument("--n_tokens", type=int, default=8192)
    p.add_argument("--max_seq_length", type=int, default=2048)
    a = p.parse_args()
    if not a.no_kernel:
        kernel_ab(a.rounds)
    if a.model:
        model_runs(a.formats.split(","), a.n_tokens, a.max_seq_length)
