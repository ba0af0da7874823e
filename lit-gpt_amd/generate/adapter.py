"""Generation with a LLaMA-Adapter (v1) checkpoint on the MI355X — drop-in for the reference's generate/adapter.py.

Same command line as the reference's generate/adapter.py (``prompt``, ``input``, ``adapter_path``, ``checkpoint_dir``,
``quantize``, ``max_new_tokens``, ``top_k``, ``temperature``, ``precision``). The instruction is wrapped in the Alpaca
prompt the adapter was fine-tuned on and the answer is what follows ``### Response:``. The model comes from
``generate.base.build_model`` (any ``--quantize`` mode of this build, or bf16: the adapter touches no Linear), the
adapter from ``lit_gpt.adapter.attach``, and decoding runs through ``generate.base.generate``: one HIP graph replay per
step, with one ``lga_adapter_attention`` launch per adapted block inside it.

Added to the reference's switches, as in generate/lora.py and generate/base.py:
  * ``--top_p``: nucleus sampling on the device.
  * ``--kv_cache fp8``: the e4m3 KV cache.
  * ``--synthetic NAME``: no tokenizer, the prompt is ``--prompt_len`` synthetic token ids and the generated ids are
    printed. The model is ``checkpoint_dir`` when that holds ``lit_config.json`` and ``lit_model.pth``, else a
    random-init model of the registered config NAME; the adapter is ``adapter_path`` when that file exists, else a
    seeded random one (``lit_gpt.adapter.random_adapter``).

``adapter_prompt_length`` and ``adapter_start_layer`` below must match what the adapter was trained with (the
reference's finetune/adapter.py uses the ``Config`` defaults, 10 and 2).
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path
from typing import List, Optional

import torch

wd = Path(__file__).parent.parent.resolve()
if str(wd) not in sys.path:
    sys.path.append(str(wd))

from generate.base import KV_CACHE_DTYPES, build_model, generate, top_k_arg  # noqa: E402
from generate.lora import generate_prompt  # noqa: E402,F401  (the Alpaca prompt, shared with generate/lora.py)
from lit_gpt import adapter  # noqa: E402
from lit_gpt import quantize as quantize_mod  # noqa: E402

adapter_prompt_length = 10
adapter_start_layer = 2


def _adapter_kwargs() -> dict:
    return dict(adapter_prompt_length=adapter_prompt_length, adapter_start_layer=adapter_start_layer)


@torch.inference_mode()
def main(prompt: str = "What food do llamas eat?", input: str = "",
         adapter_path: Path = Path("out/adapter/alpaca/lit_model_adapter_finetuned.pth"),
         checkpoint_dir: Path = Path("checkpoints/stabilityai/stablelm-base-alpha-3b"),
         quantize: Optional[str] = None, max_new_tokens: int = 100, top_k: Optional[int] = 200,
         temperature: float = 0.8, precision: Optional[str] = None, synthetic: Optional[str] = None,
         prompt_len: int = 16, top_p: float = 1.0, kv_cache: str = "bf16") -> List[int]:
    """Generates a response to an instruction (and optional input) with the adapter of ``adapter_path`` on the model of
    ``checkpoint_dir``; returns the token ids (prompt + generated). Everything that cannot run is refused before the
    model is built."""
    precision = precision or "bf16-true"
    if precision not in ("bf16-true", "32-true"):
        raise NotImplementedError("the MI355X path computes in bf16 (bf16-true) or fp32 (32-true)")
    if kv_cache not in KV_CACHE_DTYPES:
        raise ValueError(f"--kv_cache must be one of {sorted(KV_CACHE_DTYPES)}, got {kv_cache!r}")
    if max_new_tokens < 1:
        raise ValueError(f"--max_new_tokens must be positive, got {max_new_tokens}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"--top_p must be in (0, 1], got {top_p}")
    if quantize is not None:
        quantize_mod.parse_mode(quantize)  # an unknown mode fails here, before any weight is materialised
    checkpoint_dir, adapter_path = Path(checkpoint_dir), Path(adapter_path)
    have_checkpoint = (checkpoint_dir / "lit_config.json").is_file() and (checkpoint_dir / "lit_model.pth").is_file()
    if synthetic is not None and not have_checkpoint:
        config = adapter.Config.from_name(synthetic, **_adapter_kwargs())
        checkpoint_path = None
    else:
        from lit_gpt.utils import check_valid_checkpoint_dir

        if synthetic is None:
            check_valid_checkpoint_dir(checkpoint_dir)
        config = adapter.Config.from_json(checkpoint_dir / "lit_config.json", **_adapter_kwargs())
        checkpoint_path = checkpoint_dir / "lit_model.pth"
    adapter.check_supported(config, precision=precision)
    if synthetic is None and not adapter_path.is_file():
        raise FileNotFoundError(f"no adapter checkpoint at {str(adapter_path)!r} (the output of finetune/adapter.py)")

    device = torch.device("cuda", torch.cuda.current_device())
    tokenizer = None
    if synthetic is not None:
        g = torch.Generator(device="cpu").manual_seed(1234)
        encoded = torch.randint(0, config.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to(device)
    else:
        from lit_gpt.tokenizer import Tokenizer

        tokenizer = Tokenizer(checkpoint_dir)
        encoded = tokenizer.encode(generate_prompt({"instruction": prompt, "input": input}), device=device)
    prompt_length = encoded.size(0)
    max_returned_tokens = prompt_length + max_new_tokens

    print(f"Loading model {str(checkpoint_path or synthetic)!r} with {config.__dict__}", file=sys.stderr)
    t0 = time.perf_counter()
    model = build_model(config, quantize=quantize, device=device, checkpoint_path=checkpoint_path,
                        max_seq_length=max_returned_tokens, prefill_rows=prompt_length, kv_cache=kv_cache)
    if adapter_path.is_file():
        state = torch.load(str(adapter_path), map_location="cpu", weights_only=True)
    else:
        state = adapter.random_adapter(config)
    adapter.attach(model, state, config)
    print(f"Time to load the model weights: {time.perf_counter() - t0:.02f} seconds.", file=sys.stderr)

    torch.manual_seed(1234)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = generate(model, encoded, max_returned_tokens, temperature=temperature, top_k=top_k,
                 eos_id=tokenizer.eos_id if tokenizer is not None else None,
                 **({"top_p": top_p} if top_p < 1.0 else {}))
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    if tokenizer is not None:
        print(tokenizer.decode(y).split("### Response:")[1].strip())
    else:
        print(y.tolist())
    tokens_generated = y.size(0) - prompt_length
    print(f"\n\nTime for inference: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec", file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_allocated() / 1e9:.02f} GB", file=sys.stderr)
    return y.tolist()


def _cli(argv=None) -> None:
    p = argparse.ArgumentParser(description="Generates a response to an instruction with a LLaMA-Adapter model.")
    p.add_argument("--prompt", default="What food do llamas eat?")
    p.add_argument("--input", default="")
    p.add_argument("--adapter_path", type=Path, default=Path("out/adapter/alpaca/lit_model_adapter_finetuned.pth"))
    p.add_argument("--checkpoint_dir", type=Path, default=Path("checkpoints/stabilityai/stablelm-base-alpha-3b"))
    p.add_argument("--quantize", default=None)
    p.add_argument("--max_new_tokens", type=int, default=100)
    p.add_argument("--top_k", type=top_k_arg, default=200, help="an integer, or 'none'")
    p.add_argument("--top_p", type=float, default=1.0, help="nucleus sampling (generate/base.py --top_p)")
    p.add_argument("--temperature", type=float, default=0.8)
    p.add_argument("--precision", default=None)
    p.add_argument("--kv_cache", default="bf16", choices=sorted(KV_CACHE_DTYPES),
                   help="fp8: the e4m3 KV cache (generate/base.py --kv_cache)")
    p.add_argument("--synthetic", default=None, help="no tokenizer: synthetic prompt ids; random-init model of this "
                                                     "registered config name unless checkpoint_dir holds one, and a "
                                                     "random adapter unless adapter_path exists")
    p.add_argument("--prompt_len", type=int, default=16)
    a = p.parse_args(argv)
    main(a.prompt, a.input, a.adapter_path, a.checkpoint_dir, a.quantize, a.max_new_tokens, a.top_k, a.temperature,
         a.precision, a.synthetic, a.prompt_len, a.top_p, a.kv_cache)


if __name__ == "__main__":
    _cli()
