"""Cost of the LLaMA-Adapter (v1) term on the Llama-2-7B geometry (output kept as
profiles/adapter_ab.txt).

Per launch: ONE lga_adapter_attention on T = 1 (a decode step) and on T = 2048 rows (a prefill), H = G = 32, head size
128, adapter_prompt_length 10. Method (as tools/lora_ab.py): each kind runs as one captured graph of 32 back-to-back
launches, one per layer, over distinct qkv / y / prefix K / V buffers (all L2-resident, as inside a decode step); the
kinds alternate inside each of ROUNDS rounds, timed with device events; reported per launch: median over the rounds, and
the minimum.

Model: the synthetic Llama-2-7B in int4-g128, a 2048-token prompt and 255 decode steps through the decode graph, with a
random adapter (adapter_prompt_length 10, adapter_start_layer 2: 30 adapted blocks) and without, interleaved in one
process over REPS repetitions: two models built from one seed, so on equal weights — a plain lit_gpt.GPT and one with
the adapter attached. Reported: the prefill time and the decode rate of both.

usage: python tools/adapter_ab.py [--rounds 7] [--reps 3] [--no-model]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

H = G = 32
HS = 128
AT = 10
LAYERS = 32
REPLAYS = 8


def timed(graph, replays=REPLAYS):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        graph.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / replays  # us per replay


def capture(run):
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g


def launches(rounds, dev):
    print("lga_adapter_attention, us per launch: median (min) over %d alternating rounds; H = G = %d, hs = %d, aT = %d"
          % (rounds, H, HS, AT))
    cos = torch.rand(4096, HS, device=dev)
    sin = torch.rand(4096, HS, device=dev)
    gating = (torch.randn(H, device=dev) * 0.5).bfloat16()
    graphs = {}
    for T in (1, 2048):
        layers = LAYERS if T == 1 else 4
        bufs = [((torch.randn(T, (H + 2 * G) * HS, device=dev)).bfloat16(), torch.randn(T, H * HS, device=dev).bfloat16(),
                 torch.randn(G, AT, HS, device=dev).bfloat16(), torch.randn(G, AT, HS, device=dev).bfloat16())
                for _ in range(layers)]
        pos = torch.arange(T, device=dev, dtype=torch.int64) + (2048 if T == 1 else 0)

        def run(bufs=bufs, pos=pos):
            for qkv, y, ak, av in bufs:
                ops.adapter_attention(y, qkv, ak, av, gating, pos, cos, sin, H, G, HS, HS, HS ** -0.5)

        graphs[T] = (capture(run), layers)
    t = {T: [] for T in graphs}
    for _ in range(rounds):
        for T, (g, layers) in graphs.items():
            t[T].append(timed(g) / layers)
    for T, v in t.items():
        print(f"  T = {T:<5d} {statistics.median(v):9.2f} ({min(v):.2f})   spread (max - min) {max(v) - min(v):.2f}", flush=True)


@torch.inference_mode()
def model(dev, reps, T=2048, steps=255):
    from generate.base import build_model
    from lit_gpt import Config, adapter
    from lit_gpt.runtime import DecodeGraph

    # two models on the same weights (build_model's seed): a plain lit_gpt.GPT that never saw the adapter code, and
    # one with the adapter attached
    cfg = adapter.Config.from_name("Llama-2-7b-hf", adapter_prompt_length=AT, adapter_start_layer=2)
    kw = dict(quantize="int4-g128", device=dev, max_seq_length=T + steps + 1)
    models = {"without": build_model(Config.from_name("Llama-2-7b-hf"), **kw), "with": build_model(cfg, **kw)}
    adapter.attach(models["with"], adapter.random_adapter(cfg), cfg)
    assert type(models["without"]).__module__ == "lit_gpt.model"
    assert torch.equal(models["without"].lm_head.qweight, models["with"].lm_head.qweight)
    g = torch.Generator().manual_seed(7)
    prompt = torch.randint(0, cfg.vocab_size, (1, T), generator=g, dtype=torch.int32).to(dev)

    def run(m):
        for b in m.transformer.h:
            b.attn.kv_cache.reset_parameters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logits = m(prompt, torch.arange(T, device=dev), last_token_only=True)
        torch.cuda.synchronize()
        prefill = time.perf_counter() - t0
        dg = DecodeGraph(m, logits.reshape(-1).argmax().view(1), T, chunk=8)  # runs step 1 eagerly, then captures
        n = steps - 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n // 8):
            dg.steps()
        for _ in range(n % 8):
            dg.step()
        torch.cuda.synchronize()
        return prefill * 1e3, n / (time.perf_counter() - t0)

    for m in models.values():  # warm-up of both
        run(m)
    res = {k: [] for k in models}
    for _ in range(reps):
        for k, m in models.items():
            res[k].append(run(m))
    print(f"Llama-2-7B int4-g128, {T}-token prompt, {steps} decode steps, {reps} interleaved repetitions: median (min .. "
          "max)")
    med = {}
    for k, v in res.items():
        pre, rate = [x[0] for x in v], [x[1] for x in v]
        med[k] = (statistics.median(pre), statistics.median(rate))
        print(f"  {k + ' the adapter':20s} prefill {med[k][0]:8.2f} ms ({min(pre):.2f} .. {max(pre):.2f})   decode "
              f"{med[k][1]:7.2f} tokens/s ({min(rate):.2f} .. {max(rate):.2f})")
    n = cfg.n_layer - cfg.adapter_start_layer
    step = [1e3 / med[k][1] for k in ("without", "with")]
    print(f"  per step: {step[0]:.3f} ms -> {step[1]:.3f} ms, +{(step[1] - step[0]) * 1e3 / n:.2f} us per adapted block "
          f"({n} blocks); prefill +{(med['with'][0] - med['without'][0]) * 1e3 / n:.1f} us per adapted block")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adapter_ab.py measures on the GPU; no device found")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    ops.load_library()
    print(torch.cuda.get_device_name(0))
    launches(a.rounds, dev)
    if not a.no_model:
        model(dev, a.reps)
