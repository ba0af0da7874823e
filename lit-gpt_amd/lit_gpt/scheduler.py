"""Host bookkeeping of continuous batching (generate.base.generate_continuous): which prompt sits in which slot of
the batched decode step, how many tokens each sequence has collected and sampled, where it ends, and what goes to the
next free slot. Pure Python on ints and floats — it touches no tensor on a device; the step executor
(lit_gpt.runtime.SlotDecodeGraph) does what it says.

A sequence's decode tokens are the ones ``generate`` would return after the prefill's token: collected up to and
including the first ``eos_id``, or up to its budget of ``max_new - 1`` decode steps (the prefill's token is the first
of the ``max_new`` and is never tested against eos, as in ``generate``). Tokens a slot produced past that point
within a launch of several steps are dropped."""

from __future__ import annotations

from collections import deque
from typing import Deque, List, Optional, Sequence, Tuple, Union

from lit_gpt import ops


class SlotScheduler:
    def __init__(self, prompt_lens: Sequence[int], max_new_tokens: Union[int, Sequence[int]], n_slots: int, *,
                 chunk: int = 1, eos_id: Optional[int] = None, seeds: Optional[Sequence[int]] = None,
                 max_seq_length: Optional[int] = None) -> None:
        """``prompt_lens[i]`` tokens in prompt i, ``max_new_tokens`` new tokens for every prompt or one count per
        prompt, ``n_slots`` sequences per decode step, ``chunk`` steps per long launch. ``seeds[i]``: the sampler seed
        of prompt i (None: greedy, no uniforms). ``max_seq_length``: the cache length every sequence must fit."""
        n = len(prompt_lens)
        if n == 0:
            raise ValueError("SlotScheduler: no prompts")
        budgets = [int(max_new_tokens)] * n if isinstance(max_new_tokens, int) else [int(m) for m in max_new_tokens]
        if len(budgets) != n:
            raise ValueError(f"SlotScheduler: {len(budgets)} max_new_tokens for {n} prompts")
        if any(m < 1 for m in budgets):
            raise ValueError("SlotScheduler: max_new_tokens must be at least 1")
        if any(int(t) < 1 for t in prompt_lens):
            raise ValueError("SlotScheduler: empty prompt")
        if n_slots < 1:
            raise ValueError("SlotScheduler: needs at least one slot")
        if seeds is not None and len(seeds) != n:
            raise ValueError(f"SlotScheduler: {len(seeds)} seeds for {n} prompts")
        need = max(int(t) + m - 1 for t, m in zip(prompt_lens, budgets))
        if max_seq_length is not None and max_seq_length < need:
            raise NotImplementedError(f"max_seq_length {max_seq_length} needs to be >= {need}")
        self.prompt_lens = [int(t) for t in prompt_lens]
        self.steps_budget = [m - 1 for m in budgets]  # decode steps after the prefill's token
        self.n_slots = min(int(n_slots), n)
        self.chunk = max(1, int(chunk))
        self.eos_id = eos_id
        self.seeds = None if seeds is None else [int(s) for s in seeds]
        self.queue: Deque[int] = deque(range(n))
        self.slot_prompt: List[Optional[int]] = [None] * self.n_slots
        self.collected = [0] * self.n_slots  # decode tokens kept so far, per slot
        self.draws = [0] * self.n_slots      # tokens the slot's sequence has sampled so far (the prefill's is draw 0)
        self.tokens: List[Optional[List[int]]] = [None] * n  # per prompt: its decode tokens, once started
        self.finished = [False] * n
        self.served: List[List[int]] = [[] for _ in range(self.n_slots)]  # per slot: the prompts it has held

    # ------------------------------------------------------------------------------------------------ admission
    def next_fill(self) -> Optional[Tuple[int, int]]:
        """(slot, prompt index) of the next admission — the lowest free slot takes the head of the queue — or None
        when no slot is free or nothing waits. The caller prefills the prompt into the slot, then calls ``start``."""
        if not self.queue:
            return None
        for b, i in enumerate(self.slot_prompt):
            if i is None:
                return b, self.queue[0]
        return None

    def start(self, slot: int) -> bool:
        """The head of the queue now sits in ``slot``, its prefill's token sampled (draw 0). Returns whether the slot
        decodes (True: the executor's ``fill``) — False when the budget was that one token: the sequence is finished
        and the slot is free again."""
        if self.slot_prompt[slot] is not None:
            raise RuntimeError(f"slot {slot} is taken")
        i = self.queue.popleft()
        self.tokens[i] = []
        self.served[slot].append(i)
        if self.steps_budget[i] == 0:
            self.finished[i] = True
            return False
        self.slot_prompt[slot] = i
        self.collected[slot] = 0
        self.draws[slot] = 1
        return True

    # ------------------------------------------------------------------------------------------------- stepping
    @property
    def active(self) -> List[bool]:
        return [i is not None for i in self.slot_prompt]

    @property
    def done(self) -> bool:
        return not self.queue and all(i is None for i in self.slot_prompt)

    def remaining(self, slot: int) -> int:
        return self.steps_budget[self.slot_prompt[slot]] - self.collected[slot]

    def next_launch(self) -> int:
        """Steps of the next launch: ``chunk`` while every active slot has that many left to collect, else 1 (a slot
        near its budget is stepped singly, so it is refilled the step after its last token; only an eos can leave
        dropped tokens behind it within a chunk)."""
        left = [self.remaining(b) for b in range(self.n_slots) if self.slot_prompt[b] is not None]
        if not left:
            raise RuntimeError("next_launch: no active slot")
        return self.chunk if self.chunk > 1 and min(left) >= self.chunk else 1

    def uniforms(self, n_steps: int) -> List[List[float]]:
        """(n_steps, n_slots) uniforms of the next launch: slot b at step s draws ``ops.sampler_uniform(seed, draws +
        s)`` of its sequence; an idle slot gets 0.5 (its sample is never read)."""
        if self.seeds is None:
            raise RuntimeError("uniforms: the scheduler was built without seeds (greedy)")
        return [[0.5 if i is None else ops.sampler_uniform(self.seeds[i], self.draws[b] + s)
                 for b, i in enumerate(self.slot_prompt)] for s in range(n_steps)]

    def consume(self, history: Sequence[Sequence[int]]) -> List[int]:
        """``history[s][b]``: the token slot b produced at step s of the launch just read. Collects each active
        slot's tokens up to and including its first eos or up to its budget, drops the rest, and returns the slots
        whose sequence finished (now free: the caller releases them, ``next_fill`` hands them out again)."""
        freed = []
        n = len(history)
        for b, i in enumerate(self.slot_prompt):
            if i is None:
                continue
            self.draws[b] += n
            for s in range(n):
                tok = int(history[s][b])
                self.tokens[i].append(tok)
                self.collected[b] += 1
                if (self.eos_id is not None and tok == self.eos_id) or self.collected[b] == self.steps_budget[i]:
                    self.finished[i] = True
                    self.slot_prompt[b] = None
                    freed.append(b)
                    break
        return freed

    def results(self) -> List[List[int]]:
        """The decode tokens of every prompt, in prompt order (after ``done``)."""
        if not all(self.finished):
            raise RuntimeError("results: sequences are still running")
        return [list(t) for t in self.tokens]
