"""Speculative decoding on the MI355X, greedy or under top-k sampling: a drafter proposes up to ``speculate``
tokens, the target model scores them as ONE verify window (``GPT.decode_window``: every weight streamed once for the
window's rows, one window attention launch per block), and the longest prefix the target agrees with is kept, plus
the target's own next token.

The promise: **speculation never changes the result.** Row r of the verify window has the bits of the one-row decode
step at that position (the rows GEMVs and ``lga_attention_decode_window`` are bit-identical to their one-row
launches), so ``generate_speculative`` returns exactly the tokens ``generate`` returns, whatever the drafter
proposes: at temperature 0 the arg-maxes, and at ``temperature > 0`` with ``top_k`` the tokens ``generate`` samples
with the same seed. Two things this rests on:

  * the same ``max_seq_length``: ``ops.decode_splits`` derives the attention split count from the cache length and
    the bits of the attention output depend on it, so the run uses the cache ``generate`` would use — it is never
    padded for the window; the last windows are shortened instead;
  * stale cache rows: rejected rows leave K/V past the accepted position. Decode attention reads no row past its own
    position and the next window overwrites them, so no rollback copy is made.

Sampling (``temperature > 0`` with ``top_k`` in 1..1024, the device sampler of ``generate``): that sampler's uniform
for draw number n is a pure function of (seed, n), so the n-th generated token is a function of (the target's logits
at its position, seed, n). The verify window samples row r with draw number c + r, c the tokens generated so far
(``lga_spec_accept_sample``), and accepts draft r iff it EQUALS that sample: every emitted token is the one
``generate`` draws, and the drafts only decide how many a round yields. This is not rejection sampling (which has
the right distribution but does not reproduce ``generate``). Without ``top_k`` the run is greedy only: sampling at
temperature > 0 raises ``NotImplementedError``.
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence

import torch

wd = Path(__file__).parent.parent.resolve()
if str(wd) not in sys.path:
    sys.path.append(str(wd))

from lit_gpt import GPT, Config  # noqa: E402

# Default draft length. Measured on Llama-2-7B int4-g128: a verify round costs 1.50 / 2.27 / 3.76
# one-row steps at gamma = 1 / 3 / 7, so with each draft accepted independently at rate r the expected speed-up is
# best at gamma = 3 for r between about 0.75 and 0.9 (gamma = 7 only ties it at 0.9 and loses below; gamma = 1 wins
# only below 0.7, where nothing gains much)
DEFAULT_SPECULATE = 3


class NgramDrafter:
    """Prompt-lookup drafting on the host, for users with no second checkpoint: propose the tokens that followed the
    most recent earlier occurrence of the last ``n`` tokens of prompt + output, or of a shorter suffix down to one
    token. No match proposes nothing, and the round is then an ordinary one-row step."""

    def __init__(self, n: int = 3) -> None:
        if n < 1:
            raise ValueError("NgramDrafter: n must be at least 1")
        self.n = n

    def begin(self, prompt: torch.Tensor, first_token: int) -> None:
        pass

    def propose(self, tokens: Sequence[int], k: int) -> List[int]:
        L = len(tokens)
        if k <= 0:
            return []
        for m in range(min(self.n, L - 1), 0, -1):  # the longest suffix first
            suffix = list(tokens[L - m:])
            for i in range(L - m - 1, -1, -1):  # the most recent earlier occurrence first
                if list(tokens[i:i + m]) == suffix:
                    return list(tokens[i + m:i + m + k])  # (a slice: never past the sequence)
        return []


class ScriptedDrafter:
    """Drafts from a known continuation (tests and ``tools/spec_decode.py``): ``reference`` is the full token sequence
    ``generate`` returns; ``wrong(round, index)`` says whether draft ``index`` of verify round ``round`` is corrupted
    (replaced by another token id), which forces the acceptance pattern."""

    def __init__(self, reference: Sequence[int], wrong: Callable[[int, int], bool], vocab: int) -> None:
        self.reference, self.wrong, self.vocab = list(reference), wrong, vocab
        self.round = 0

    def begin(self, prompt: torch.Tensor, first_token: int) -> None:
        self.round = 0

    def propose(self, tokens: Sequence[int], k: int) -> List[int]:
        L = len(tokens)
        out = []
        for i, t in enumerate(self.reference[L:L + k]):
            out.append((t + 1) % self.vocab if self.wrong(self.round, i) else t)
        self.round += 1
        return out


class ModelDrafter:
    """A second ``GPT`` on the target's device as the drafter, with its own KV cache and one-row ``DecodeGraph``: any
    model the one-sequence greedy graph runs, with the target's ``padded_vocab_size``. It prefills the prompt,
    proposes by one-row greedy steps whose tokens stay on the device, and before each round is re-pointed
    (``DecodeGraph.reset``) at the accepted prefix. Its cache holds the K/V of positions below ``valid``; after a fully
    accepted round the last draft token's K/V is missing (that token was proposed, never run), so ``propose`` first
    runs the missing positions, then drafts.

    Under sampling (``set_sampling``) with ``coupled=True`` the draft model proposes by sampling its OWN logits with
    the TARGET's uniforms: draft i of a round that starts with n tokens generated uses draw number n + i of the
    target's seed, at the target's temperature and top_k (its ``DecodeGraph`` samples with a counter of its own, set
    to n before the step that produces draft 0). The target accepts a draft iff it equals its own sample under that
    same uniform, so a coupled draft is accepted whenever both inverse CDFs land on the same token — with probability
    approaching 1 as the draft's distribution approaches the target's — while a greedy draft is accepted with at most
    the target's largest probability. ``coupled=False`` keeps greedy drafting under sampling."""

    def __init__(self, draft_model: GPT, coupled: bool = True) -> None:
        self.model = draft_model
        self.coupled = coupled
        self.dg = None
        self.valid = 0
        self.buf: Optional[torch.Tensor] = None
        self.sampling = None  # (temperature, top_k, seed) while drafting with the target's uniforms
        self.top_p = 1.0
        self.rng = None
        self.T = 0

    def check(self, target: GPT) -> None:
        if self.model.config.padded_vocab_size != target.config.padded_vocab_size:
            raise ValueError(f"draft model vocabulary ({self.model.config.padded_vocab_size} padded) differs from the "
                             f"target's ({target.config.padded_vocab_size}): drafts must be the target's token ids")
        if self.model.transformer.wte.weight.device != target.transformer.wte.weight.device:
            raise ValueError("the draft model must sit on the target's device")

    def set_sampling(self, temperature: float, top_k: Optional[int], seed: int, top_p: float = 1.0) -> None:
        """The target's sampling setting for the run about to ``begin`` (temperature 0: greedy). ``top_p`` < 1: the
        draft model's logits are sampled at the target's ``top_p`` too (``top_k`` may then be None)."""
        k = None if top_k is None else int(top_k)
        self.sampling = (float(temperature), k, int(seed)) if temperature > 0.0 and self.coupled else None
        self.top_p = float(top_p)

    def begin(self, prompt: torch.Tensor, first_token: int) -> None:
        m = self.model
        T = prompt.size(0)
        if m.max_seq_length < T + 1:
            raise NotImplementedError(f"draft model max_seq_length {m.max_seq_length} is shorter than the prompt")
        m(prompt.view(1, -1), torch.arange(0, T, device=prompt.device), last_token_only=True)  # fills its cache
        self.valid = self.T = T
        self.dg = None
        self.buf = torch.zeros(GPT.MAX_WINDOW, dtype=torch.int32, device=prompt.device)
        self.rng = None
        if self.sampling is not None:
            from generate.base import SamplerRNG

            self.rng = SamplerRNG(prompt.device, seed=self.sampling[2])

    def _run(self, token: int, pos: int) -> None:
        """One draft step of ``token`` at ``pos``; its successor (greedy, or sampled with the draw number in
        ``rng.counter``, which the step advances) is left in ``dg.token``."""
        if self.dg is None:
            from lit_gpt.runtime import DecodeGraph

            first = torch.tensor([token], dtype=torch.int32, device=self.buf.device)
            kw = {}
            if self.rng is not None:
                kw = dict(temperature=self.sampling[0], top_k=self.sampling[1], rng=self.rng)
                if self.top_p < 1.0:
                    kw["top_p"] = self.top_p
            self.dg = DecodeGraph(self.model, first, pos, **kw)  # runs that step itself, then captures
        else:
            self.dg.reset(token, pos)
            self.dg.step()

    def propose(self, tokens: Sequence[int], k: int):
        P = len(tokens) - 1  # the position of the last emitted token
        k = min(k, self.model.max_seq_length - 1 - P)
        if k <= 0:
            return []
        self.valid = min(self.valid, P)  # draft rows past the accepted prefix are stale
        while self.valid < P:  # catch up (after a fully accepted round: the last draft token's position)
            self._run(int(tokens[self.valid]), self.valid)
            self.valid += 1
        if self.rng is not None:  # draft 0 is generated token number len(tokens) - T (the catch-up steps drew too)
            self.rng.counter.fill_(len(tokens) - self.T)
        self._run(int(tokens[P]), P)
        self.buf[0:1].copy_(self.dg.token.view(-1))
        for i in range(1, k):
            self.buf[i:i + 1].copy_(self.dg.step().view(-1))
        self.valid = P + k
        return self.buf[:k]


def speculative_rounds(executor, drafter, tokens: List[int], n_steps: int, max_seq: int, speculate: int,
                       eos_id: Optional[int] = None, stats: Optional[Dict[str, int]] = None) -> List[int]:
    """The round loop. ``tokens`` is the host copy of prompt + the prefill's token (the last entry is the last emitted
    token, at position ``len(tokens) - 1``); ``executor.step(drafts) -> (a, new)`` verifies the drafts after it and
    returns the accepted count and the a + 1 tokens the round emits (``lit_gpt.runtime.WindowDecodeGraph``). Each
    round asks for k = min(speculate, steps left - 1, cache rows left - 1) drafts, so a round never emits more than
    the budget nor writes past the cache. Returns the ``<= n_steps`` decoded tokens, cut after the first ``eos_id``."""
    new_tokens: List[int] = []
    seq = list(tokens)
    rounds = proposed = accepted = 0
    while len(new_tokens) < n_steps:
        P = len(seq) - 1
        k = min(speculate, n_steps - len(new_tokens) - 1, max_seq - P - 1)
        drafts = drafter.propose(seq, k) if k > 0 else []
        if len(drafts) > k:
            drafts = drafts[:k]
        a, new = executor.step(drafts)
        rounds += 1
        proposed += len(drafts)
        accepted += a
        if eos_id is not None and eos_id in new:  # tokens after an eos are dropped, as in generate
            new_tokens.extend(new[:new.index(eos_id) + 1])
            break
        new_tokens.extend(new)
        seq.extend(new)
    if stats is not None:
        stats["rounds"] = stats.get("rounds", 0) + rounds
        stats["proposed"] = stats.get("proposed", 0) + proposed
        stats["accepted"] = stats.get("accepted", 0) + accepted
        stats["tokens"] = stats.get("tokens", 0) + len(new_tokens)
    return new_tokens


@torch.inference_mode()
def generate_speculative(model: GPT, prompt: torch.Tensor, max_returned_tokens: int, drafter, *,
                         speculate: int = DEFAULT_SPECULATE, eos_id: Optional[int] = None, use_graph: bool = True,
                         stats: Optional[Dict[str, int]] = None, temperature: float = 0.0,
                         top_k: Optional[int] = None, rng=None, top_p: float = 1.0) -> torch.Tensor:
    """``generate(model, prompt, max_returned_tokens, temperature=0.0, eos_id=eos_id)``, token for token, in fewer
    target passes: each round verifies up to ``speculate`` drafts of ``drafter`` (``NgramDrafter``, ``ModelDrafter``)
    in one window and emits the accepted ones plus the target's next token. The KV cache must be the one ``generate``
    would run with (same ``max_seq_length``: see the module docstring). One device -> host read per round.
    ``stats`` collects ``rounds`` (target passes), ``proposed``, ``accepted`` and ``tokens``.

    With ``temperature > 0`` and ``top_k`` in 1..1024 it returns, token for token, what ``generate(model, prompt,
    max_returned_tokens, temperature=temperature, top_k=top_k, eos_id=eos_id, rng=SamplerRNG(device, seed=s))``
    returns for the seed ``s`` of ``rng`` (a ``generate.base.SamplerRNG``; omitted: seeded from torch's generator, as
    ``generate`` does). The prefill's token is draw 0 and the n-th generated token draw n. With ``top_p`` < 1 the
    same holds for ``generate(..., top_p=top_p)`` on the device nucleus sampler, and ``top_k`` may be None."""
    from generate.base import SamplerRNG, check_top_p, next_token
    from lit_gpt import ops

    sampling = temperature > 0.0
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"generate_speculative: top_p must be in (0, 1], got {top_p}")
    if not sampling:
        top_p = 1.0  # greedy: top-p cannot change the arg-max
    nucleus = top_p < 1.0
    if nucleus:
        check_top_p("generate_speculative", top_p, temperature, top_k, model.transformer.wte.weight.dtype,
                    model.config.padded_vocab_size)
    if sampling and top_k is None and not nucleus:
        raise NotImplementedError("without top_k generate_speculative is greedy only: speculative sampling runs on "
                                  f"the device top-k sampler (top_k 1..{ops.MAX_TOP_K})")
    if sampling and top_k is not None and not 1 <= top_k <= ops.MAX_TOP_K:
        raise NotImplementedError(f"speculative sampling runs on the device top-k sampler: top_k must be in "
                                  f"1..{ops.MAX_TOP_K}, got {top_k}")
    if not 1 <= speculate <= GPT.MAX_WINDOW - 1:
        raise ValueError(f"speculate must be in 1..{GPT.MAX_WINDOW - 1} (a verify window holds {GPT.MAX_WINDOW} rows)")
    T = prompt.size(0)
    assert max_returned_tokens > T
    if model.max_seq_length < max_returned_tokens - 1:
        raise NotImplementedError(f"max_seq_length {model.max_seq_length} needs to be >= {max_returned_tokens - 1}")
    c = model.config
    from generate.base import graph_sampling
    from lit_gpt.runtime import WindowDecodeGraph

    # everything the verify step refuses is refused here, before the prefill
    model._rows_check("speculative decoding")
    if sampling and not nucleus and not graph_sampling(model, temperature, top_k):
        raise NotImplementedError("speculative sampling runs on the device top-k sampler: bf16 logits of at most "
                                  f"{ops.MAX_SAMPLE_VOCAB} entries (this model: {c.padded_vocab_size})")
    if not ops.decode_fusable(c.head_size, c.rope_n_elem) or c.n_head // c.n_query_groups not in (1, 2, 4, 8):
        raise NotImplementedError("speculative decoding needs the fused decode attention's geometry (head_size == "
                                  "rope_n_elem == 128, 1 / 2 / 4 / 8 heads per query group)")
    if hasattr(drafter, "check"):
        drafter.check(model)
    device = prompt.device
    rng = (rng or SamplerRNG(device)) if sampling else None
    if hasattr(drafter, "set_sampling"):
        drafter.set_sampling(temperature, top_k, rng.seed if sampling else 0, *((top_p,) if nucleus else ()))
    kw = dict(temperature=temperature, top_k=top_k, rng=rng) if sampling else dict(temperature=0.0)
    if nucleus:
        kw["top_p"] = top_p
    token = next_token(model, torch.arange(0, T, device=device), prompt.view(1, -1), **kw).clone()
    n_steps = max_returned_tokens - T - 1
    if n_steps <= 0:
        return torch.cat([prompt, token])
    tokens = prompt.tolist() + [int(token)]
    drafter.begin(prompt, tokens[-1])
    ex = WindowDecodeGraph(model, token, T, use_graph=use_graph, **(kw if sampling else {}))
    new = speculative_rounds(ex, drafter, tokens, n_steps, model.max_seq_length, speculate, eos_id, stats)
    return torch.cat([prompt, token, torch.tensor(new, dtype=prompt.dtype, device=device)])


@torch.inference_mode()
def main(prompt: str = "What food do llamas eat?", *, max_new_tokens: int = 50,
         checkpoint_dir: Path = Path("checkpoints/stabilityai/stablelm-base-alpha-3b"),
         quantize: Optional[str] = "int4-g128", precision: Optional[str] = None, synthetic: Optional[str] = None,
         prompt_len: int = 16, draft: Optional[str] = None, draft_checkpoint_dir: Optional[Path] = None,
         draft_synthetic: Optional[str] = None, draft_quantize: Optional[str] = "int4-g128",
         speculate: int = DEFAULT_SPECULATE, temperature: float = 0.0, top_k: Optional[int] = None,
         kv_cache: str = "bf16", top_p: float = 1.0) -> None:
    """``kv_cache`` is the TARGET's cache format (generate/base.py ``--kv_cache``); a draft model keeps bf16.
    ``temperature`` > 0 needs ``top_k`` in 1..1024 and prints what generate/base.py prints at that setting; with
    ``top_p`` < 1 (nucleus sampling) ``top_k`` may be None."""
    from generate.base import build_model
    from lit_gpt import ops

    if (precision or "bf16-true") != "bf16-true":
        raise NotImplementedError("speculative decoding runs 4-bit weights under bf16-true")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"--top_p must be in (0, 1], got {top_p}")
    if temperature > 0.0 and ((top_k is None and top_p == 1.0) or
                              (top_k is not None and not 1 <= top_k <= ops.MAX_TOP_K)):
        raise NotImplementedError("without --top_k in 1..1024 generate/speculative.py is greedy only (temperature 0)")
    kinds = [draft is not None, draft_checkpoint_dir is not None, draft_synthetic is not None]
    if sum(kinds) != 1:
        raise ValueError("choose one drafter: --draft ngram, --draft_checkpoint_dir DIR or --draft_synthetic NAME")
    if draft is not None and draft != "ngram":
        raise ValueError(f"--draft {draft!r}: the host drafter is 'ngram'")
    device = torch.device("cuda", torch.cuda.current_device())
    tokenizer = None
    if synthetic is not None:
        config = Config.from_name(synthetic)
        checkpoint_path = None
        g = torch.Generator(device="cpu").manual_seed(1234)
        encoded = torch.randint(0, config.vocab_size, (prompt_len,), generator=g, dtype=torch.int32).to(device)
    else:
        from lit_gpt.tokenizer import Tokenizer
        from lit_gpt.utils import check_valid_checkpoint_dir

        check_valid_checkpoint_dir(checkpoint_dir)
        config = Config.from_json(checkpoint_dir / "lit_config.json")
        checkpoint_path = checkpoint_dir / "lit_model.pth"
        tokenizer = Tokenizer(checkpoint_dir)
        encoded = tokenizer.encode(prompt, device=device)
    prompt_length = encoded.size(0)
    max_returned_tokens = prompt_length + max_new_tokens
    print(f"Loading model {str(checkpoint_path or synthetic)!r} with {config.__dict__}", file=sys.stderr)
    t0 = time.perf_counter()
    model = build_model(config, quantize=quantize, device=device, checkpoint_path=checkpoint_path,
                        max_seq_length=max_returned_tokens, prefill_rows=prompt_length, kv_cache=kv_cache)
    if draft == "ngram":
        drafter = NgramDrafter()
    else:
        if draft_synthetic is not None:
            dconfig, dpath = Config.from_name(draft_synthetic), None
        else:
            from lit_gpt.utils import check_valid_checkpoint_dir

            check_valid_checkpoint_dir(draft_checkpoint_dir)
            dconfig = Config.from_json(draft_checkpoint_dir / "lit_config.json")
            dpath = draft_checkpoint_dir / "lit_model.pth"
        drafter = ModelDrafter(build_model(dconfig, quantize=draft_quantize, device=device, checkpoint_path=dpath,
                                           max_seq_length=max_returned_tokens, prefill_rows=prompt_length, seed=4321))
    print(f"Time to load the model weights: {time.perf_counter() - t0:.02f} seconds.", file=sys.stderr)
    eos_id = tokenizer.eos_id if tokenizer is not None else None
    stats: Dict[str, int] = {}
    torch.manual_seed(1234)  # as generate/base.py's main: the sampler's seed is drawn from torch's generator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = generate_speculative(model, encoded, max_returned_tokens, drafter, speculate=speculate, eos_id=eos_id,
                             stats=stats, temperature=temperature, top_k=top_k,
                             **({"top_p": top_p} if top_p < 1.0 else {}))
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    print(tokenizer.decode(y) if tokenizer is not None else y.tolist())
    tokens_generated = y.size(0) - prompt_length
    print(f"Time for inference 1: {t:.02f} sec total, {tokens_generated / t:.02f} tokens/sec", file=sys.stderr)
    rate = stats.get("accepted", 0) / max(1, stats.get("proposed", 0))
    print(f"Speculation: {stats.get('accepted', 0)} of {stats.get('proposed', 0)} drafts accepted ({rate:.1%}), "
          f"{stats.get('tokens', 0) / max(1, stats.get('rounds', 0)):.2f} tokens per target pass over "
          f"{stats.get('rounds', 0)} passes", file=sys.stderr)
    print(f"Memory used: {torch.cuda.max_memory_allocated() / 1e9:.02f} GB", file=sys.stderr)


def _top_k_arg(text: str) -> Optional[int]:
    return None if text.strip().lower() == "none" else int(text)


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Speculative decoding: the tokens of generate/base.py at temperature 0, "
                                            "or at --temperature T --top_k K with the same seed, in fewer "
                                            "target-model passes.")
    p.add_argument("--prompt", default="What food do llamas eat?")
    p.add_argument("--max_new_tokens", type=int, default=50)
    p.add_argument("--checkpoint_dir", type=Path, default=Path("checkpoints/stabilityai/stablelm-base-alpha-3b"))
    p.add_argument("--quantize", default="int4-g128", help="the target's 4-bit format (the verify window streams "
                                                           "plain 4-bit Linears)")
    p.add_argument("--precision", default=None)
    p.add_argument("--temperature", type=float, default=0.0,
                   help="0: greedy; > 0 samples as generate/base.py does and needs --top_k")
    p.add_argument("--top_k", type=_top_k_arg, default=None,
                   help="with --temperature > 0: sample among the top_k (1..1024); 'none' with --top_p")
    p.add_argument("--top_p", type=float, default=1.0,
                   help="with --temperature > 0: nucleus sampling as generate/base.py --top_p (1.0: off)")
    p.add_argument("--synthetic", default=None, help="random-init target of this registered config name")
    p.add_argument("--prompt_len", type=int, default=16)
    p.add_argument("--draft", default=None, choices=["ngram"], help="prompt-lookup drafting on the host")
    p.add_argument("--draft_checkpoint_dir", type=Path, default=None, help="a draft model checkpoint")
    p.add_argument("--draft_synthetic", default=None, help="random-init draft model of this registered config name")
    p.add_argument("--draft_quantize", default="int4-g128")
    p.add_argument("--speculate", type=int, default=DEFAULT_SPECULATE,
                   help=f"drafts per round (1..{GPT.MAX_WINDOW - 1})")
    p.add_argument("--kv_cache", default="bf16", choices=["bf16", "fp8"],
                   help="the target's KV cache format (fp8: e4m3 codes + one scale per row); a draft model keeps bf16")
    a = p.parse_args(argv)
    if sum(x is not None for x in (a.draft, a.draft_checkpoint_dir, a.draft_synthetic)) != 1:
        p.error("choose one drafter: --draft ngram, --draft_checkpoint_dir DIR or --draft_synthetic NAME")
    if not 1 <= a.speculate <= GPT.MAX_WINDOW - 1:
        p.error(f"--speculate must be in 1..{GPT.MAX_WINDOW - 1}")
    if a.top_k is not None and not 1 <= a.top_k <= 1024:
        p.error("--top_k must be in 1..1024 (the device top-k sampler)")
    if not 0.0 < a.top_p <= 1.0:
        p.error("--top_p must be in (0, 1]")
    if a.temperature > 0.0 and a.top_k is None and a.top_p == 1.0:
        p.error("--temperature > 0 needs --top_k in 1..1024: without it speculative decoding here is greedy only")
    return a


def _cli(argv=None) -> None:
    a = parse_args(argv)
    main(a.prompt, max_new_tokens=a.max_new_tokens, checkpoint_dir=a.checkpoint_dir, quantize=a.quantize,
         precision=a.precision, synthetic=a.synthetic, prompt_len=a.prompt_len, draft=a.draft,
         draft_checkpoint_dir=a.draft_checkpoint_dir, draft_synthetic=a.draft_synthetic,
         draft_quantize=a.draft_quantize, speculate=a.speculate, temperature=a.temperature, top_k=a.top_k,
         kv_cache=a.kv_cache, top_p=a.top_p)


if __name__ == "__main__":
    _cli()
