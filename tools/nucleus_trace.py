"""Lab: phase timeline of the nucleus sampler (csrc/sample.hip nucleus_sample_row, lab build with -DLGA_SAMPLE_TRACE).

    make -C lit-gpt_amd/csrc lab-lib LABSRC=sample LABFLAGS=-DLGA_SAMPLE_TRACE LABLIB=../../tools/_fa/libsample_trace.so
    python tools/nucleus_trace.py tools/_fa/libsample_trace.so

Times one temperature 0.8 / top_p 0.9 draw over bf16 logits shaped like a decode step's (N(0, 3)) for each form, then
prints thread 0's timestamps (100 MHz clock, 10 ns resolution) after: the candidates (key max, top-k selection), the
softmax sum, the high-byte weight histogram and its scan, the low-byte pass, the draw.
"""
import ctypes
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]
from lit_gpt import ops  # noqa: E402


def main(lib_path: str) -> None:
    ops._lib = ops.load_library(Path(lib_path))
    lib = ctypes.CDLL(lib_path)
    dev = torch.device("cuda")
    points = [(9, "candidates"), (10, "softmax sum"), (13, "high byte"), (11, "low byte"), (12, "draw")]
    for n, k in ((32000, 200), (32000, None), (50304, None), (65536, None)):
        x = (torch.randn(n, generator=torch.Generator().manual_seed(0)) * 3).bfloat16().to(dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        for _ in range(20):
            ops.sample_nucleus(x, k, 0.9, 0.8, seed=1, counter=counter)
        torch.cuda.synchronize()
        buf = (ctypes.c_ulonglong * 16)()
        assert lib.lga_sample_trace(buf) == 0
        t0 = buf[8]
        row = "  ".join(f"{name} {(buf[i] - t0) * 10 / 1000:6.2f}" for i, name in points)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            ops.sample_nucleus(x, k, 0.9, 0.8, seed=1, counter=counter)
        e1.record()
        torch.cuda.synchronize()
        print(f"n {n:5d} top_k {str(k):4s} launch {e0.elapsed_time(e1) * 10:6.2f} us | us after staging: {row}",
              flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
