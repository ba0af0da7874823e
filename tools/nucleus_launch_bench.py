"""Lab: launch time of the device samplers, lga_sample_topk against lga_sample_nucleus.

    python tools/nucleus_launch_bench.py [OUT.txt]

Each setting is one HIP graph of R = 200 launches over N(0, 3) bf16 logits at temperature 0.8 (counter-driven draws);
the graphs are replayed in turn (A/B alternated in one process), device events around each replay, 12 rounds of which
the first 2 are dropped; min / median / max microseconds per launch.
"""
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402

DEV = "cuda"
R, REP = 200, 12
# (kind, n, top_k, top_p)
SETTINGS = [("topk", 32000, 200, None), ("nucleus", 32000, 200, 0.9), ("nucleus", 32000, None, 0.9),
            ("topk", 50304, 200, None), ("nucleus", 50304, 200, 0.9), ("nucleus", 50304, None, 0.9),
            ("topk", 65536, 200, None), ("nucleus", 65536, 200, 0.9), ("nucleus", 65536, None, 0.9),
            ("nucleus", 32000, None, 0.5), ("nucleus", 32000, None, 0.999)]


def capture(kind, n, k, top_p):
    x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3).to(torch.bfloat16).to(DEV)
    c = torch.zeros(1, dtype=torch.int64, device=DEV)
    o = torch.zeros(1, dtype=torch.int64, device=DEV)

    def one():
        if kind == "topk":
            ops.sample_topk(x, k, 0.8, seed=7, counter=c, out_idx=o)
        else:
            ops.sample_nucleus(x, k, top_p, 0.8, seed=7, counter=c, out_idx=o)

    for _ in range(5):
        one()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(R):
            one()
    g.replay()
    torch.cuda.synchronize()
    return g


def main(out_path: str) -> None:
    ops.load_library()
    graphs = [capture(*s) for s in SETTINGS]
    times = [[] for _ in SETTINGS]
    for _ in range(REP):
        for i, g in enumerate(graphs):  # alternated
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            times[i].append(a.elapsed_time(b) * 1000.0 / R)
    with open(out_path, "w") as f:
        for (kind, n, k, top_p), t in zip(SETTINGS, times):
            t = sorted(t[2:])
            line = (f"{kind:8s} n={n:6d} top_k={str(k):5s} top_p={str(top_p):6s} us/launch min {t[0]:7.2f} "
                    f"median {t[len(t) // 2]:7.2f} max {t[-1]:7.2f}")
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "nucleus_sampler_launch.txt")
