"""EleutherAI lm-evaluation-harness (0.3) adapter on the MI355X path — the reference's ``eval/lm_eval_harness.py``.

``EvalHarnessBase`` carries the reference adapter's properties (``eot_token_id``, ``max_length``, ``vocab_size``,
``max_gen_toks``, ``tok_encode`` / ``tok_decode``) and implements the three request methods lm-eval 0.3 calls on a
language model — ``loglikelihood``, ``loglikelihood_rolling``, ``greedy_until`` — directly on ``lit_gpt/score.py``
(per-token log-probabilities reduced on the device, never a ``(T, V)`` logits tensor on the host) and
``generate/base.py``. The reference subclasses ``lm_eval.base.BaseLM``, whose versions of these methods go through
``_model_call`` and a host ``log_softmax``; this class does not import ``lm_eval`` at all, so the scoring logic is
usable (and tested) without the package.

``run_eval`` is the only place that needs ``lm_eval`` (task registry + ``evaluator.evaluate``); it imports the package
lazily and raises an ``ImportError`` naming it when it is missing. That glue has NOT been exercised: no test here
has ``lm_eval`` to run it against.

    python eval/lm_eval_harness.py --checkpoint_dir checkpoints/... --quantize int4-g128 --eval_tasks hellaswag piqa
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import torch

wd = Path(__file__).parent.parent.resolve()
if str(wd) not in sys.path:
    sys.path.append(str(wd))

from lit_gpt import score  # noqa: E402


class EvalHarnessBase:
    def __init__(self, model, tokenizer, batch_size: int = 1) -> None:
        if batch_size != 1:
            raise NotImplementedError("the MI355X path scores and generates at batch size 1")
        self.model = model
        self.tokenizer = tokenizer
        self.batch_size_per_gpu = batch_size

    # ---- the reference adapter's surface ---------------------------------------------------------------------
    @property
    def eot_token_id(self) -> int:
        # end of *text*, as the reference: the tokenizer's eos id
        return self.tokenizer.eos_id

    @property
    def max_length(self) -> int:
        return self.model.max_seq_length

    @property
    def vocab_size(self) -> int:
        return self.tokenizer.vocab_size

    @property
    def max_gen_toks(self) -> int:
        return 256

    @property
    def batch_size(self) -> int:
        return self.batch_size_per_gpu

    @property
    def device(self) -> torch.device:
        return self.model.transformer.wte.weight.device

    def tok_encode(self, string: str) -> List[int]:
        return self.tokenizer.encode(string, bos=False, eos=False).tolist()

    def tok_decode(self, tokens: Sequence[int]) -> str:
        return self.tokenizer.decode(torch.tensor(list(tokens)))

    # ---- lm-eval 0.3 request methods -------------------------------------------------------------------------
    def _score(self, tokens: List[int], n_scored: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return score.score_tokens(self.model, tokens, n_scored)

    def _loglikelihood_tokens(self, context: List[int], continuation: List[int]) -> Tuple[float, bool]:
        """Sum of the continuation's log-probabilities given the context, and whether greedy decoding would have
        produced exactly the continuation. The scored input is ``(context + continuation)[-(max_length + 1):]``
        without its last token; the rows scored are the continuation's."""
        if not continuation:
            return 0.0, True
        tokens = (context + continuation)[-(self.max_length + 1):]
        n = min(len(continuation), len(tokens) - 1)
        lp, greedy = self._score(tokens, n)
        same = torch.equal(greedy.cpu().to(torch.int64), torch.tensor(tokens[len(tokens) - n:], dtype=torch.int64))
        return float(lp.double().sum()), bool(same) and n == len(continuation)

    def loglikelihood(self, requests: Sequence[Tuple[str, str]]) -> List[Tuple[float, bool]]:
        out = []
        for context, continuation in requests:
            ctx = [self.eot_token_id] if context == "" else self.tok_encode(context)
            out.append(self._loglikelihood_tokens(ctx, self.tok_encode(continuation)))
        return out

    def loglikelihood_rolling(self, requests: Sequence[Tuple[str]]) -> List[float]:
        """lm-eval's rolling log-likelihood: the text is cut by ``score.rolling_windows`` (prefix ``eot_token_id``) so
        that every token is scored exactly once with as much left context as ``max_length`` allows."""
        out = []
        for req in requests:
            toks = self.tok_encode(req[0] if isinstance(req, (tuple, list)) else req)
            total, done = 0.0, 0
            for input_ids, n_scored in score.rolling_windows(toks, self.max_length, self.eot_token_id):
                done += n_scored  # the window's last scored token is toks[done - 1]: score_tokens wants it appended
                lp, _ = self._score(input_ids + [toks[done - 1]], n_scored)
                total += float(lp.double().sum())
            out.append(total)
        return out

    def greedy_until(self, requests: Sequence[Tuple[str, dict]]) -> List[str]:
        from generate.base import generate

        out = []
        for context, args in requests:
            until = args["until"] if isinstance(args, dict) else args
            until = [until] if isinstance(until, str) else list(until)
            keep = self.max_length - self.max_gen_toks
            if keep <= 0:
                raise ValueError(f"greedy_until: max_length {self.max_length} leaves no room for a context beside "
                                 f"max_gen_toks {self.max_gen_toks}")
            ctx = self.tok_encode(context)[-keep:]
            eos = self.tok_encode(until[0])[0] if until and until[0] else self.eot_token_id
            prompt = torch.tensor(ctx, dtype=torch.int32, device=self.device)
            y = generate(self.model, prompt, len(ctx) + self.max_gen_toks, temperature=0.0, eos_id=eos)
            for block in self.model.transformer.h:  # as the reference's _model_generate
                block.attn.kv_cache.reset_parameters()
            text = self.tok_decode(y[len(ctx):].tolist())
            for stop in until:
                if stop:
                    text = text.split(stop)[0]
            out.append(text)
        return out

    # ---- the lm_eval glue (unexercised: needs the lm_eval package) ---------------------------------------------
    @torch.inference_mode()
    def run_eval(self, eval_tasks: List[str], num_fewshot: int, limit: Optional[int], bootstrap_iters: int,
                 no_cache: bool) -> Dict:
        try:
            from lm_eval import base, evaluator, tasks
        except ImportError as e:
            raise ImportError("run_eval needs the `lm_eval` package (EleutherAI lm-evaluation-harness 0.3.x), which is "
                              "not installed; the request methods of EvalHarnessBase work without it") from e
        import fnmatch

        names = sorted({m for pat in eval_tasks for m in fnmatch.filter(tasks.ALL_TASKS, pat)})
        print(f"Found tasks: {names}")
        lm = self if no_cache else base.CachingLM(self, "lm_cache/lit-gpt.db")
        results = evaluator.evaluate(lm=lm, task_dict=tasks.get_task_dict(names), num_fewshot=num_fewshot,
                                     limit=limit, bootstrap_iters=bootstrap_iters)
        results["config"] = dict(model=self.model.config.name, batch_size=self.batch_size, device=str(self.device),
                                 num_fewshot=num_fewshot, limit=limit, bootstrap_iters=bootstrap_iters,
                                 no_cache=no_cache)
        return results


@torch.inference_mode()
def run_eval_harness(checkpoint_dir: Path, precision: Optional[str] = None, quantize: Optional[str] = None,
                     eval_tasks: Sequence[str] = ("arc_challenge", "piqa", "hellaswag", "hendrycksTest-*"),
                     save_filepath: Optional[Path] = None, num_fewshot: int = 0, limit: Optional[int] = None,
                     bootstrap_iters: int = 100000, no_cache: bool = True):
    from generate.base import build_model
    from lit_gpt import Config
    from lit_gpt.tokenizer import Tokenizer
    from lit_gpt.utils import check_valid_checkpoint_dir

    precision = precision or "bf16-true"
    if precision not in ("bf16-true", "32-true"):
        raise NotImplementedError("the MI355X path computes in bf16 (bf16-true) or fp32 (32-true)")
    dtype = torch.float32 if precision == "32-true" else torch.bfloat16
    checkpoint_dir = Path(checkpoint_dir)
    check_valid_checkpoint_dir(checkpoint_dir)
    tokenizer = Tokenizer(checkpoint_dir)
    config = Config.from_json(checkpoint_dir / "lit_config.json")
    checkpoint_path = checkpoint_dir / "lit_model.pth"
    device = torch.device("cuda", torch.cuda.current_device())
    print(f"Loading model {str(checkpoint_path)!r} with {config.__dict__}", file=sys.stderr)
    model = build_model(config, quantize=quantize, device=device, checkpoint_path=checkpoint_path, dtype=dtype)
    harness = EvalHarnessBase(model, tokenizer, 1)
    results = harness.run_eval(list(eval_tasks), num_fewshot, limit, bootstrap_iters, no_cache)
    if save_filepath is None:
        print(results)
    else:
        print(f"Saving results to {str(save_filepath)!r}")
        save_filepath = Path(save_filepath)
        save_filepath.parent.mkdir(parents=True, exist_ok=True)
        save_filepath.write_text(json.dumps(results))
    return results


def _cli(argv=None) -> None:
    p = argparse.ArgumentParser(description="Runs lm-evaluation-harness tasks on a checkpoint (needs `lm_eval`).")
    p.add_argument("--checkpoint_dir", type=Path, default=Path("checkpoints/stabilityai/stablelm-base-alpha-3b"))
    p.add_argument("--precision", default=None)
    p.add_argument("--quantize", default=None)
    p.add_argument("--eval_tasks", nargs="+", default=["arc_challenge", "piqa", "hellaswag", "hendrycksTest-*"])
    p.add_argument("--save_filepath", type=Path, default=None)
    p.add_argument("--num_fewshot", type=int, default=0)
    p.add_argument("--limit", type=int, default=None)
    p.add_argument("--bootstrap_iters", type=int, default=100000)
    p.add_argument("--no_cache", type=lambda s: s.lower() not in ("0", "false", "no"), default=True)
    a = p.parse_args(argv)
    run_eval_harness(a.checkpoint_dir, a.precision, a.quantize, a.eval_tasks, a.save_filepath, a.num_fewshot, a.limit,
                     a.bootstrap_iters, a.no_cache)


if __name__ == "__main__":
    _cli()
