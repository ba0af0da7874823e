"""Generation with a LoRA adapter on the MI355X — drop-in for the reference's generate/lora.py.

Same command line as the reference's generate/lora.py (:33-43: ``prompt``, ``input``, ``lora_path``,
``checkpoint_dir``, ``quantize``, ``max_new_tokens``, ``top_k``, ``temperature``, ``precision``) and the same
module-level ``lora_r`` ... ``lora_head`` settings (:22-30), which must match what the adapter was trained with. The
instruction is wrapped in the Alpaca prompt and the answer is what follows ``### Response:`` (:95-96, :129). The model
comes from ``generate.base.build_model`` (any ``--quantize`` mode of this build, or bf16), the adapter from
``lit_gpt.lora.attach``, and decoding runs through ``generate.base.generate``: one HIP graph replay per step.

Differences from the reference:
  * ``--merge / --no-merge``. The reference always merges (:120), re-quantizing a bitsandbytes weight. Here a bf16 base
    merges by default (the adapter-free decode speed and every fusion return); a quantized base keeps its weight and
    runs the adapter next to it (one ``lga_lora_gemv`` per adapted Linear and step). ``--merge`` on a quantized base is
    refused; ``--no-merge`` on a bf16 base runs the run-time path.
  * ``--synthetic NAME`` (as generate/base.py): no tokenizer, the prompt is ``--prompt_len`` synthetic token ids and
    the generated ids are printed. The model is ``checkpoint_dir`` when that holds ``lit_config.json`` and
    ``lit_model.pth``, else a random-init model of the registered config NAME; the adapter is ``lora_path`` when that
    file exists, else a seeded random one (``lit_gpt.lora.random_adapter``).
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

from generate.base import build_model, generate, top_k_arg  # noqa: E402
from lit_gpt import lora  # noqa: E402

lora_r = 8
lora_alpha = 16
lora_dropout = 0.05
lora_query = True
lora_key = False
lora_value = True
lora_projection = False
lora_mlp = False
lora_head = False


def generate_prompt(example: dict) -> str:
    """The Alpaca prompt the adapter was fine-tuned on (the reference's scripts/prepare_alpaca.py generate_prompt):
    instruction, optional input, and the response marker the answer is split at."""
    if example.get("input"):
        return ("Below is an instruction that describes a task, paired with an input that provides further context. "
                "Write a response that appropriately completes the request.\n\n"
                f"### Instruction:\n{example['instruction']}\n\n### Input:\n{example['input']}\n\n### Response:")
    return ("Below is an instruction that describes a task. "
            "Write a response that appropriately completes the request.\n\n"
            f"### Instruction:\n{example['instruction']}\n\n### Response:")


def _lora_kwargs() -> dict:
    return dict(r=lora_r, alpha=lora_alpha, dropout=lora_dropout, to_query=lora_query, to_key=lora_key,
                to_value=lora_value, to_projection=lora_projection, to_mlp=lora_mlp, to_head=lora_head)


@torch.inference_mode()
def main(prompt: str = "What food do llamas eat?", input: str = "",
         lora_path: Path = Path("out/lora/alpaca/lit_model_lora_finetuned.pth"),
         checkpoint_dir: Path = Path("checkpoints/stabilityai/stablelm-base-alpha-3b"),
         quantize: Optional[str] = None, max_new_tokens: int = 100, top_k: Optional[int] = 200,
         temperature: float = 0.8, precision: Optional[str] = None, merge: Optional[bool] = None,
         synthetic: Optional[str] = None, prompt_len: int = 16, top_p: float = 1.0) -> List[int]:
    """Generates a response to an instruction (and optional input) with the adapter of ``lora_path`` on the model of
    ``checkpoint_dir``; returns the token ids (prompt + generated)."""
    precision = precision or "bf16-true"
    if precision not in ("bf16-true", "32-true"):
        raise NotImplementedError("the MI355X path computes in bf16 (bf16-true) or fp32 (32-true)")
    checkpoint_dir, lora_path = Path(checkpoint_dir), Path(lora_path)
    have_checkpoint = (checkpoint_dir / "lit_config.json").is_file() and (checkpoint_dir / "lit_model.pth").is_file()
    if synthetic is not None and not have_checkpoint:
        config = lora.Config.from_name(synthetic, **_lora_kwargs())
        checkpoint_path = None
    else:
        from lit_gpt.utils import check_valid_checkpoint_dir

        if synthetic is None:
            check_valid_checkpoint_dir(checkpoint_dir)
        config = lora.Config.from_json(checkpoint_dir / "lit_config.json", **_lora_kwargs())
        checkpoint_path = checkpoint_dir / "lit_model.pth"
    # everything an adapter cannot run with is refused here, before any weight is materialised
    lora.check_supported(config, precision=precision)
    if merge is None:
        merge = quantize is None
    if merge and quantize is not None:
        raise NotImplementedError(f"--merge with --quantize {quantize}: merging re-quantizes the weight and rounds the "
                                  "adapter's update to the quantization step; run without --merge (the adapter is "
                                  "applied next to the quantized weight)")
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
                        max_seq_length=max_returned_tokens, prefill_rows=prompt_length)
    if lora_path.is_file():
        adapter = torch.load(str(lora_path), map_location="cpu", weights_only=True)
    elif synthetic is not None:
        adapter = lora.random_adapter(config)
    else:
        raise FileNotFoundError(f"no adapter checkpoint at {str(lora_path)!r} (the output of finetune/lora.py)")
    lora.attach(model, adapter, config)
    if merge:
        lora.merge_lora_weights(model)
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
    p = argparse.ArgumentParser(description="Generates a response to an instruction with a LoRA-adapted model.")
    p.add_argument("--prompt", default="What food do llamas eat?")
    p.add_argument("--input", default="")
    p.add_argument("--lora_path", type=Path, default=Path("out/lora/alpaca/lit_model_lora_finetuned.pth"))
    p.add_argument("--checkpoint_dir", type=Path, default=Path("checkpoints/stabilityai/stablelm-base-alpha-3b"))
    p.add_argument("--quantize", default=None)
    p.add_argument("--max_new_tokens", type=int, default=100)
    p.add_argument("--top_k", type=top_k_arg, default=200, help="an integer, or 'none'")
    p.add_argument("--top_p", type=float, default=1.0, help="nucleus sampling (generate/base.py --top_p)")
    p.add_argument("--temperature", type=float, default=0.8)
    p.add_argument("--precision", default=None)
    p.add_argument("--merge", action=argparse.BooleanOptionalAction, default=None,
                   help="fold the adapter into the weights (default for a bf16 base); --no-merge applies it at run "
                        "time (default, and the only way, for a quantized base)")
    p.add_argument("--synthetic", default=None, help="no tokenizer: synthetic prompt ids; random-init model of this "
                                                     "registered config name unless checkpoint_dir holds one")
    p.add_argument("--prompt_len", type=int, default=16)
    a = p.parse_args(argv)
    main(a.prompt, a.input, a.lora_path, a.checkpoint_dir, a.quantize, a.max_new_tokens, a.top_k, a.temperature,
         a.precision, a.merge, a.synthetic, a.prompt_len, a.top_p)


if __name__ == "__main__":
    _cli()
