"""Perplexity of a token stream under a model, and how far one weight format's predictions are from another's.

    python eval/perplexity.py --checkpoint_dir checkpoints/... --text wiki.txt --quantize int4-g128
    python eval/perplexity.py --checkpoint_dir checkpoints/... --tokens ids.npy --quantize bnb.nf4-dq --against bf16
    python eval/perplexity.py --synthetic Llama-2-7b-hf --n_tokens 8192 --max_seq_length 2048 --quantize int4-g128

The stream is cut into windows of at most ``--max_seq_length`` inputs (``lit_gpt.score.rolling_windows``: every token
scored exactly once; ``--min_context c`` makes every scored token see at least ``c`` inputs — strided perplexity — at
the price of more windows) and each window goes through ``lit_gpt.score.score_tokens``: the log-probabilities are
reduced on the device, the logits never reach the host. Prints ONE JSON line:

    {"tokens": N, "nll": sum of -log p, "ppl": exp(nll / N), "windows": W, "tokens_per_s": scored tokens per second}

``--against MODE`` (``bf16`` or a quantize mode) builds a second model from the same weights and adds ``mean_kl`` /
``max_kl`` (KL(MODE model || evaluated model) per position, nats) and ``top1_agree`` (share of positions where both
pick the same token), from ``lit_gpt.score.compare_tokens``.

``--kv_cache fp8`` scores every window as a prefill through an fp8 (e4m3) KV cache (``input_pos = arange(T)``), so
``nll`` / ``ppl`` reflect the quantized K / V: the way to see what that cache format costs on a real checkpoint.
Without it (or with ``--kv_cache bf16``) the windows take the no-cache forward, as before. ``--against`` models keep
the no-cache forward.

``--synthetic NAME`` is a random-init model of a registered config with seeded token ids, as ``generate/base.py
--synthetic``: it measures speed and orders the formats by their distance to bf16 on THIS build's arithmetic; it is not
the loss of a trained checkpoint.
"""

from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path
from typing import Optional

import torch

wd = Path(__file__).parent.parent.resolve()
if str(wd) not in sys.path:
    sys.path.append(str(wd))

from lit_gpt import Config, score  # noqa: E402


@torch.inference_mode()
def evaluate(model, tokens, *, max_len: int, prefix_token: int, min_context: int = 1, against=None,
             cached: bool = False) -> dict:
    """Score ``tokens`` (a sequence of ids) window by window; the dict the command prints. ``cached``: every window is
    a prefill through the model's KV cache, so ``nll`` / ``ppl`` see its format (``--kv_cache fp8``)."""
    toks = [int(t) for t in tokens]
    nll, windows, done, dt = 0.0, 0, 0, 0.0
    kls, agree = [], 0
    for input_ids, n_scored in score.rolling_windows(toks, max_len, prefix_token, min_context):
        done += n_scored
        window = input_ids + [toks[done - 1]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp, _, hidden = score.score_tokens(model, window, n_scored, return_hidden=True, cached=cached)
        nll -= float(lp.double().sum())  # (a device-to-host copy: the window's work is done)
        dt += time.perf_counter() - t0
        windows += 1
        if against is not None:  # outside the timed span; the evaluated model's blocks are not run again
            kl, ag = score.compare_tokens(against, model, window, n_scored, hidden_q=hidden)
            kls.append(kl.double().cpu())
            agree += int(ag.sum())
    out = {"tokens": done, "nll": nll, "ppl": math.exp(nll / done) if done else float("nan"), "windows": windows,
           "tokens_per_s": done / dt if dt > 0 else float("nan")}
    if against is not None:
        k = torch.cat(kls) if kls else torch.zeros(0, dtype=torch.float64)
        out.update(mean_kl=float(k.mean()) if done else float("nan"), max_kl=float(k.max()) if done else float("nan"),
                   top1_agree=agree / done if done else float("nan"))
    return out


def main(*, checkpoint_dir: Optional[Path] = None, text: Optional[Path] = None, tokens: Optional[Path] = None,
         synthetic: Optional[str] = None, n_tokens: int = 2048, quantize: Optional[str] = None,
         precision: Optional[str] = None, max_seq_length: Optional[int] = None, min_context: int = 1,
         against: Optional[str] = None, kv_cache: str = "bf16") -> dict:
    from generate.base import build_model

    precision = precision or "bf16-true"
    if precision not in ("bf16-true", "32-true"):
        raise NotImplementedError("the MI355X path computes in bf16 (bf16-true) or fp32 (32-true)")
    dtype = torch.float32 if precision == "32-true" else torch.bfloat16
    if against is not None and dtype != torch.bfloat16:
        raise NotImplementedError("--against compares bf16 logits (lga_logits_kl): use --precision bf16-true")
    device = torch.device("cuda", torch.cuda.current_device())
    prefix = 0
    if synthetic is not None:
        if text is not None or tokens is not None:
            raise ValueError("--synthetic takes --n_tokens, not --text / --tokens")
        config = Config.from_name(synthetic)
        checkpoint_path = None
        g = torch.Generator(device="cpu").manual_seed(1234)
        ids = torch.randint(0, config.vocab_size, (n_tokens,), generator=g, dtype=torch.int64).tolist()
    else:
        from lit_gpt.tokenizer import Tokenizer
        from lit_gpt.utils import check_valid_checkpoint_dir

        if checkpoint_dir is None or (text is None) == (tokens is None):
            raise ValueError("give --checkpoint_dir with exactly one of --text / --tokens, or --synthetic NAME")
        check_valid_checkpoint_dir(checkpoint_dir)
        config = Config.from_json(checkpoint_dir / "lit_config.json")
        checkpoint_path = checkpoint_dir / "lit_model.pth"
        tokenizer = Tokenizer(checkpoint_dir)
        prefix = tokenizer.eos_id
        if text is not None:
            ids = tokenizer.encode(Path(text).read_text(), bos=False, eos=False).tolist()
        else:
            import numpy as np

            ids = np.load(tokens, allow_pickle=False).reshape(-1).astype(np.int64).tolist()
    max_len = max_seq_length or config.block_size

    def build(mode: Optional[str], kv: str = "bf16"):
        return build_model(config, quantize=None if mode in (None, "bf16") else mode, device=device,
                           checkpoint_path=checkpoint_path, max_seq_length=max_len, dtype=dtype, kv_cache=kv)

    print(f"Loading model {str(checkpoint_path or synthetic)!r} ({quantize or precision})", file=sys.stderr)
    model = build(quantize, kv_cache)
    other = build(against) if against is not None else None
    # fp8: each window is scored as a cached prefill, so the figures carry the cache's quantization; bf16 keeps the
    # no-cache forward (bit for bit the figures without the flag)
    out = evaluate(model, ids, max_len=max_len, prefix_token=prefix, min_context=min_context, against=other,
                   cached=kv_cache == "fp8")
    print(json.dumps(out))
    return out


def _cli(argv=None) -> None:
    p = argparse.ArgumentParser(description="Perplexity of a token stream; optional KL against another weight format.")
    p.add_argument("--checkpoint_dir", type=Path, default=None)
    p.add_argument("--text", type=Path, default=None, help="a text file, tokenized with the checkpoint's tokenizer")
    p.add_argument("--tokens", type=Path, default=None, help="a .npy file of token ids")
    p.add_argument("--synthetic", default=None, help="random-init model of this registered config name")
    p.add_argument("--n_tokens", type=int, default=2048, help="with --synthetic: how many seeded ids to score")
    p.add_argument("--quantize", default=None)
    p.add_argument("--precision", default=None)
    p.add_argument("--max_seq_length", type=int, default=None)
    p.add_argument("--min_context", type=int, default=1)
    p.add_argument("--against", default=None, help="bf16 or a quantize mode: also report KL and top-1 agreement")
    p.add_argument("--kv_cache", default="bf16", choices=["bf16", "fp8"],
                   help="fp8: score every window as a prefill through an fp8 (e4m3) KV cache — what that cache "
                        "format costs in nll / ppl on this checkpoint")
    a = p.parse_args(argv)
    main(checkpoint_dir=a.checkpoint_dir, text=a.text, tokens=a.tokens, synthetic=a.synthetic, n_tokens=a.n_tokens,
         quantize=a.quantize, precision=a.precision, max_seq_length=a.max_seq_length, min_context=a.min_context,
         against=a.against, kv_cache=a.kv_cache)


if __name__ == "__main__":
    _cli()
