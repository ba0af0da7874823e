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
  * ``--lora_paths P0 P1 ... --prompts_file FILE --batch_size B`` serves several adapters on one quantized base
    (``lit_gpt.lora.attach_many``, ``generate.base.generate_continuous``): each line of FILE is ``INDEX<TAB>instruction``
    (under ``--synthetic``: ``INDEX<TAB>prompt length``), INDEX a position in ``--lora_paths`` or ``-`` for no adapter.
    Up to B <= 4 requests decode together, each row of the batched step with its own adapter; the answers are printed
    in file order. 4-bit bases only, never merged.
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import torch

wd = Path(__file__).parent.parent.resolve()
if str(wd) not in sys.path:
    sys.path.append(str(wd))

from generate.base import MAX_BATCH, build_model, generate, generate_continuous, top_k_arg  # noqa: E402
from lit_gpt import lora, ops  # noqa: E402
from lit_gpt import quantize as quantize_mod  # noqa: E402

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


def parse_requests(text: str, n_adapters: int, synthetic: bool = False) -> List[Tuple[Optional[int], object]]:
    """The requests of a ``--prompts_file``: per non-empty line ``INDEX<TAB>instruction`` (``synthetic``:
    ``INDEX<TAB>prompt length``) -> (adapter index or None for ``-``, instruction or length). A line without a tab, an
    INDEX that is no position in ``--lora_paths`` or a prompt length that is no positive integer raises ValueError."""
    out: List[Tuple[Optional[int], object]] = []
    for no, line in enumerate(text.splitlines(), 1):
        if not line.strip():
            continue
        index, tab, body = line.partition("\t")
        if not tab:
            raise ValueError(f"prompts file line {no}: expected INDEX<TAB>{'prompt length' if synthetic else 'instruction'}")
        index = index.strip()
        if index == "-":
            adapter = None
        elif index.isdigit() and int(index) < n_adapters:
            adapter = int(index)
        else:
            raise ValueError(f"prompts file line {no}: INDEX {index!r} is neither '-' nor a position in the "
                             f"{n_adapters} --lora_paths")
        if synthetic:
            if not body.strip().isdigit() or int(body) < 1:
                raise ValueError(f"prompts file line {no}: prompt length {body.strip()!r} is no positive integer")
            out.append((adapter, int(body)))
        else:
            out.append((adapter, body.strip()))
    if not out:
        raise ValueError("prompts file: no requests")
    return out


@torch.inference_mode()
def serve(lora_paths: Sequence[Path], prompts_file: Path, batch_size: int = MAX_BATCH, *,
          checkpoint_dir: Path = Path("checkpoints/stabilityai/stablelm-base-alpha-3b"),
          quantize: Optional[str] = None, max_new_tokens: int = 100, top_k: Optional[int] = 200,
          temperature: float = 0.8, precision: Optional[str] = None, merge: Optional[bool] = None,
          synthetic: Optional[str] = None, top_p: float = 1.0) -> List[List[int]]:
    """The requests of ``prompts_file`` (``parse_requests``), each with the adapter of ``lora_paths`` it names, through
    ``generate_continuous`` on ``batch_size`` slots; returns the token ids per request, in file order. Everything that
    cannot run is refused before the model is built."""
    precision = precision or "bf16-true"
    if precision != "bf16-true":
        raise NotImplementedError("several adapters in a batch compute in bf16 (bf16-true)")
    if merge:
        raise NotImplementedError("--merge with --lora_paths: several adapters share one base and cannot be merged "
                                  "into it; they run next to the quantized weight")
    if quantize is None:
        raise NotImplementedError("--lora_paths with a bf16 base: the batched decode streams 4-bit weights only "
                                  f"(--quantize {quantize_mod.ROWS_MODES})")
    fmt, _ = quantize_mod.parse_mode(quantize)
    if fmt not in (ops.FMT_Q4G, ops.FMT_NF4, ops.FMT_FP4):
        raise NotImplementedError(f"--lora_paths with --quantize {quantize}: the batched decode streams 4-bit weights "
                                  f"only ({quantize_mod.ROWS_MODES})")
    if not 1 <= batch_size <= MAX_BATCH:
        raise NotImplementedError(f"--batch_size {batch_size}: the batched decode runs 1..{MAX_BATCH} sequences per step")
    lora_paths = [Path(p) for p in lora_paths]
    if not lora_paths:
        raise ValueError("--lora_paths: no adapters")
    checkpoint_dir = Path(checkpoint_dir)
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
    lora.check_supported(config, precision=precision)
    requests = parse_requests(Path(prompts_file).read_text(), len(lora_paths), synthetic is not None)
    if synthetic is None:
        for p in lora_paths:
            if not p.is_file():
                raise FileNotFoundError(f"no adapter checkpoint at {str(p)!r} (the output of finetune/lora.py)")
    adapters = [a for a, _ in requests]

    device = torch.device("cuda", torch.cuda.current_device())
    tokenizer = None
    if synthetic is not None:
        g = torch.Generator(device="cpu").manual_seed(1234)
        prompts = [torch.randint(0, config.vocab_size, (n,), generator=g, dtype=torch.int32).to(device)
                   for _, n in requests]
    else:
        from lit_gpt.tokenizer import Tokenizer

        tokenizer = Tokenizer(checkpoint_dir)
        prompts = [tokenizer.encode(generate_prompt({"instruction": text, "input": ""}), device=device)
                   for _, text in requests]
    longest = max(p.size(0) for p in prompts)
    print(f"Loading model {str(checkpoint_path or synthetic)!r} with {config.__dict__}", file=sys.stderr)
    t0 = time.perf_counter()
    model = build_model(config, quantize=quantize, device=device, checkpoint_path=checkpoint_path,
                        max_seq_length=longest + max_new_tokens, prefill_rows=longest)
    states = [torch.load(str(p), map_location="cpu", weights_only=True) if p.is_file()
              else lora.random_adapter(config, seed=1234 + i) for i, p in enumerate(lora_paths)]
    lora.attach_many(model, states, config)
    print(f"Time to load the model weights: {time.perf_counter() - t0:.02f} seconds.", file=sys.stderr)

    torch.manual_seed(1234)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ys = generate_continuous(model, prompts, max_new_tokens, batch_size=batch_size, temperature=temperature,
                             top_k=top_k, eos_id=tokenizer.eos_id if tokenizer is not None else None,
                             adapters=adapters, **({"top_p": top_p} if top_p < 1.0 else {}))
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    for y in ys:
        if tokenizer is not None:
            print(tokenizer.decode(y).split("### Response:")[1].strip())
        else:
            print(y.tolist())
    tokens_generated = sum(y.size(0) - p.size(0) for y, p in zip(ys, prompts))
    print(f"\n\nTime for inference: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec over "
          f"{len(prompts)} requests", file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_allocated() / 1e9:.02f} GB", file=sys.stderr)
    return [y.tolist() for y in ys]


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
    p.add_argument("--lora_paths", type=Path, nargs="+", default=None,
                   help="several adapters on one quantized base, served together (with --prompts_file)")
    p.add_argument("--prompts_file", type=Path, default=None,
                   help="one request per line, INDEX<TAB>instruction (--synthetic: INDEX<TAB>prompt length); INDEX is "
                        "a position in --lora_paths, or - for no adapter")
    p.add_argument("--batch_size", type=int, default=MAX_BATCH, help="requests decoding together (--lora_paths)")
    a = p.parse_args(argv)
    if (a.lora_paths is None) != (a.prompts_file is None):
        p.error("--lora_paths and --prompts_file go together")
    if a.lora_paths is not None:
        serve(a.lora_paths, a.prompts_file, a.batch_size, checkpoint_dir=a.checkpoint_dir, quantize=a.quantize,
              max_new_tokens=a.max_new_tokens, top_k=a.top_k, temperature=a.temperature, precision=a.precision,
              merge=a.merge, synthetic=a.synthetic, top_p=a.top_p)
        return
    main(a.prompt, a.input, a.lora_path, a.checkpoint_dir, a.quantize, a.max_new_tokens, a.top_k, a.temperature,
         a.precision, a.merge, a.synthetic, a.prompt_len, a.top_p)


if __name__ == "__main__":
    _cli()
