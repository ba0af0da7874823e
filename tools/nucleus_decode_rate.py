"""Lab: decode rate of generate() at temperature 0.8 on a synthetic Llama-2-7B int4-g128, 2048-token prompt, 255
decode steps. The prefill (the best of 3 one-token runs) is subtracted from 4 timed runs per setting.

    python tools/nucleus_decode_rate.py TREE TAG name:top_k:top_p ...     (top_k may be 'none'; top_p 1.0 = off)

TREE is a checkout of this repository with its library built (``.`` or another commit's, for an A/B in alternating
processes); results are appended to ``nucleus_decode_rate.txt`` or the file named by the environment variable OUT.
"""
import os
import sys
import time

import torch

P, NEW = 2048, 256


def main(tree: str, tag: str, settings) -> None:
    sys.path.insert(0, os.path.join(tree, "lit-gpt_amd"))
    from generate.base import build_model, generate
    from lit_gpt import Config

    dev = torch.device("cuda", 0)
    cfg = Config.from_name("Llama-2-7b-hf")
    model = build_model(cfg, quantize="int4-g128", device=dev, max_seq_length=P + NEW)
    g = torch.Generator(device="cpu").manual_seed(1234)
    prompt = torch.randint(0, cfg.vocab_size, (P,), generator=g, dtype=torch.int32).to(dev)

    def run(new, **kw):
        for b in model.transformer.h:
            b.attn.kv_cache.reset_parameters()
        torch.manual_seed(1234)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = generate(model, prompt, P + new, temperature=0.8, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, y

    lines = []
    for s in settings:
        name, k, p = s.split(":")
        kw = {"top_k": None if k == "none" else int(k)}
        if float(p) < 1.0:
            kw["top_p"] = float(p)
        run(NEW, **kw)  # warm
        pre = min(run(1, **kw)[0] for _ in range(3))
        rates = []
        for _ in range(4):
            t, y = run(NEW, **kw)
            rates.append((NEW - 1) / (t - pre))
        lines.append(f"{tag:7s} {name:14s} prefill {pre * 1000:7.1f} ms  decode tok/s min {min(rates):7.2f} max "
                     f"{max(rates):7.2f}  ms/step {1000 / max(rates):.3f}..{1000 / min(rates):.3f}  "
                     f"tail {y[-3:].tolist()}")
        print(lines[-1], flush=True)
    with open(os.environ.get("OUT", "nucleus_decode_rate.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
