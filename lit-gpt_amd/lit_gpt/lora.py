"""LoRA adapters at inference — the reference's lit_gpt/lora.py (Config, LoRALinear / LoRAQKVLinear forward,
merge_lora_weights) on the MI355X kernels.

The reference builds a ``lora.GPT`` whose Linears carry ``lora_A`` / ``lora_B`` next to ``linear.weight``, loads base
and adapter into it and merges (generate/lora.py:104-120). Here the model comes from the unchanged ``build_model``
(any ``--quantize`` mode or bf16), and ``attach`` swaps the targeted Linears for ``LoraLinear``: the base Linear as it
is, plus the adapter in the device layout of csrc/lora.hip. On a bf16 base ``merge_lora_weights`` folds the adapter
into the weight (``lga_lora_merge``) and puts the plain ``nn.Linear`` back. A 4-bit or int8 weight cannot take a
low-rank update without being quantized again (what the reference's ``merge`` does for bitsandbytes, lora.py:150-161,
and which loses the adapter's small values to the quantization step), so there the adapter runs next to the base in
every forward: one extra launch per adapted Linear and decode step (``lga_lora_gemv``), two per prefill.

Device layout (the LoRA section): ``lora_A`` (R, K) bf16, ``lora_B`` (N, r) bf16 in OUTPUT-row order,
``row_off`` (N,) int32 or None. A plain LoRALinear has R = r and no ``row_off``. The fused qkv Linear has one segment
of r rows of A per enabled q / k / v (R = r * enabled); output row n of the interleaved [G][q_per_kv + 2][hs] layout
uses the segment of its slot — ``row_off[n]`` = its first row, -1 where the slot has no adapter. That is the reference's
``lora_ind`` / ``zero_pad`` / grouped ``conv1d`` (lora.py:263-278, :281-377) scattered once: reference ``lora_B`` row i
lands at output row ``lora_ind[i]``. r is zero-padded to a multiple of 8 (exact zeros in the fp32 sums).

``attach_many`` attaches SEVERAL adapters of one ``Config`` to a 4-bit base for batched serving: every targeted Linear
becomes a ``MultiLoraLinear`` with the adapters stacked (``lora_A`` (n, R, K), ``lora_B`` (n, N, r)), and the model's
``AdapterSet`` (``model.lora_adapters``) says which adapter runs where — ``select(i)`` for one-sequence calls, device-
resident row ids for the batched decode step, which applies every row's own adapter in one ``lga_lora_gemv_rows`` per
adapted Linear (several adapters per batch).

``dropout`` is accepted and ignored: inference makes it the identity.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from lit_gpt import ops, quantize
from lit_gpt.config import Config as BaseConfig


@dataclass
class Config(BaseConfig):
    """lit_gpt.Config plus the reference's adapter fields (lora.py:473-494): rank ``r``, ``alpha`` (the update is
    scaled by alpha / r), ``dropout`` (ignored) and which Linears carry an adapter."""

    r: int = 0
    alpha: int = 1
    dropout: float = 0.0
    to_query: bool = False
    to_key: bool = False
    to_value: bool = False
    to_projection: bool = False
    to_mlp: bool = False
    to_head: bool = False


def padded_rank(r: int) -> int:
    return (r + 7) // 8 * 8


def check_supported(config: Config, *, precision: str = "bf16-true", world_size: int = 1) -> None:
    """What an adapter cannot run with on this build, refused before any weight is materialised."""
    if config.r <= 0:
        raise ValueError(f"LoRA rank r must be positive, got {config.r}")
    if not any((config.to_query, config.to_key, config.to_value, config.to_projection, config.to_mlp,
                config.to_head)):
        raise ValueError("the LoRA config enables no target (to_query / to_key / to_value / to_projection / to_mlp / "
                         "to_head)")
    if padded_rank(config.r) > ops.LORA_MAX_RANK:
        raise NotImplementedError(f"LoRA rank r={config.r}: the adapter kernels take r <= {ops.LORA_MAX_RANK}")
    if config.n_embd % 8 or config.intermediate_size % 8 or max(config.n_embd, config.intermediate_size) > ops.LORA_MAX_K:
        raise NotImplementedError("LoRA adapter: the adapter kernels read 16-byte chunks of rows of at most "
                                  f"{ops.LORA_MAX_K} elements; n_embd={config.n_embd}, intermediate_size="
                                  f"{config.intermediate_size}")
    if world_size > 1:
        raise NotImplementedError("a LoRA adapter with tensor parallelism: the fused GEMV + all-reduce takes plain "
                                  "4-bit or bf16 shards only; run the adapter on one device")
    if config.to_mlp and config._mlp_class == "LLaMAMoE":
        raise NotImplementedError("LoRA to_mlp with a sparse-MoE model: the routed expert kernels stack the experts' "
                                  "4-bit weights and take no adapter; adapt the attention Linears or the head instead")
    if precision == "32-true":
        raise NotImplementedError("a LoRA adapter with --precision 32-true: the adapter kernels compute in bf16 "
                                  "(bf16-true)")


def qkv_slots(out_features: int, n_head: int, n_query_groups: int) -> torch.Tensor:
    """(out_features,) int64: 0 / 1 / 2 where output row n of the fused qkv Linear is a query / key / value row. Per
    query group the rows are q_per_kv query heads, one key head, one value head (model.py CausalSelfAttention)."""
    per_group = n_head // n_query_groups + 2
    head_size = out_features // (n_query_groups * per_group)
    if head_size * n_query_groups * per_group != out_features:
        raise ValueError(f"qkv Linear with {out_features} rows does not split into {n_query_groups} groups of "
                         f"{per_group} heads")
    head = (torch.arange(out_features) // head_size) % per_group
    return (head - (per_group - 3)).clamp_(min=0)


def qkv_lora_ind(out_features: int, n_head: int, n_query_groups: int, enable: Sequence[bool]) -> List[torch.Tensor]:
    """Per enabled slot (q, k, v order) the output rows it covers, ascending: concatenated, the reference's
    ``lora_ind`` (lora.py:263-278)."""
    slots = qkv_slots(out_features, n_head, n_query_groups)
    return [torch.nonzero(slots == s).flatten() for s in range(3) if enable[s]]


def build_layout(lora_A: torch.Tensor, lora_B: torch.Tensor, r: int, out_features: int,
                 qkv: Optional[Tuple[int, int, Sequence[bool]]] = None):
    """Reference-layout adapter tensors -> (A (R', K), B (out_features, r'), row_off (out_features,) int32 or None) in
    the device layout, r' = r padded to a multiple of 8, still on the tensors' device and in their dtype.
    ``qkv`` = (n_head, n_query_groups, (to_query, to_key, to_value)) for the fused qkv Linear, None for a plain one."""
    rp = padded_rank(r)
    K = lora_A.shape[1]
    if qkv is None:
        if tuple(lora_A.shape) != (r, K) or tuple(lora_B.shape) != (out_features, r):
            raise ValueError(f"adapter shapes lora_A {tuple(lora_A.shape)} / lora_B {tuple(lora_B.shape)} do not match "
                             f"r={r}, out_features={out_features}")
        A = lora_A.new_zeros(rp, K)
        A[:r] = lora_A
        B = lora_B.new_zeros(out_features, rp)
        B[:, :r] = lora_B
        return A, B, None
    n_head, n_query_groups, enable = qkv
    ind = qkv_lora_ind(out_features, n_head, n_query_groups, enable)
    n_seg, rows = len(ind), sum(i.numel() for i in ind)
    if tuple(lora_A.shape) != (r * n_seg, K) or tuple(lora_B.shape) != (rows, r):
        raise ValueError(f"qkv adapter shapes lora_A {tuple(lora_A.shape)} / lora_B {tuple(lora_B.shape)} do not match "
                         f"r={r} with (to_query, to_key, to_value)={tuple(bool(e) for e in enable)}: expected "
                         f"({r * n_seg}, {K}) / ({rows}, {r})")
    A = lora_A.new_zeros(rp * n_seg, K)
    B = lora_B.new_zeros(out_features, rp)
    row_off = torch.full((out_features,), -1, dtype=torch.int32)
    first = 0
    for s, rows_s in enumerate(ind):
        A[s * rp:s * rp + r] = lora_A[s * r:(s + 1) * r]
        B[rows_s.to(lora_B.device), :r] = lora_B[first:first + rows_s.numel()]
        row_off[rows_s] = s * rp
        first += rows_s.numel()
    return A, B, row_off


class LoraLinear(quantize._Kernels, nn.Module):
    """A base Linear of any format (``QuantLinear``, ``Int8Linear``, a bf16 ``nn.Linear``) with a LoRA adapter applied
    at run time. ``forward`` is the ``_Kernels`` skeleton: one row -> the base's GEMV (RMSNorm fused where the base
    fuses it, no residual) and ONE ``lga_lora_gemv`` on the same x and norm that adds the adapter and the residual in
    place; several rows -> the base's GEMM, ``lga_lora_down`` and ``lga_lora_up``. ``lora_A`` / ``lora_B`` / ``row_off``
    are in the device layout (module docstring)."""

    def __init__(self, base: nn.Module, lora_A: torch.Tensor, lora_B: torch.Tensor, row_off: Optional[torch.Tensor],
                 scaling: float) -> None:
        super().__init__()
        k = quantize.kernels(base)
        if k.act_dtype != torch.bfloat16:
            raise NotImplementedError("a LoRA adapter on an fp32 Linear (--precision 32-true): the adapter kernels "
                                      "compute in bf16 (bf16-true)")
        dev = base.weight.device
        self.base = base
        self._kernels = k  # (a bf16 nn.Linear's per-call wrapper, made once)
        self.in_features, self.out_features = k.in_features, k.out_features
        self.register_buffer("lora_A", lora_A.to(device=dev, dtype=torch.bfloat16).contiguous())
        self.register_buffer("lora_B", lora_B.to(device=dev, dtype=torch.bfloat16).contiguous())
        self.register_buffer("row_off", None if row_off is None else row_off.to(device=dev, dtype=torch.int32))
        self.scaling = float(scaling)
        ops._lora_dims(self.lora_A, self.lora_B, self.row_off, "LoraLinear")
        if self.lora_A.shape[1] != self.in_features or self.lora_B.shape[0] != self.out_features:
            raise ValueError(f"adapter for ({self.lora_B.shape[0]}, {self.lora_A.shape[1]}) on a Linear of "
                             f"({self.out_features}, {self.in_features})")

    @property
    def weight(self) -> torch.Tensor:
        return self.base.weight

    @property
    def bias(self) -> Optional[torch.Tensor]:
        return self.base.bias

    def gemv_fuses_norm(self, dual: bool = False) -> bool:
        return self._kernels.gemv_fuses_norm(dual)

    def pairs_with(self, o) -> bool:  # an adapted fc_1 / fc_2 runs as two Linears + lga_swiglu
        return False

    def gemv(self, x, res, norm_weight, eps):
        y = self._kernels.gemv(x, None, norm_weight, eps).view(-1)
        return ops.lora_gemv(x, self.lora_A, self.lora_B, self.row_off, self.scaling, base=y, residual=res,
                             norm_weight=norm_weight, eps=eps, out=y)

    def gemm(self, x, res):
        y = self._kernels.gemm(x, None)
        t = ops.lora_down(x, self.lora_A)
        return ops.lora_up(t, self.lora_B, self.row_off, self.scaling, base=y, residual=res, out=y)

    def extra_repr(self) -> str:
        return f"r={self.lora_B.shape[1]}, segments={self.lora_A.shape[0] // self.lora_B.shape[1]}, scaling={self.scaling}"


class AdapterSet:
    """The adapters of one ``attach_many`` model (``model.lora_adapters``) and which of them runs where. ``rows``
    (ops.MAX_GEMV_ROWS,) int32 on the device, -1 (no adapter) at first: the id of every row of the batched decode step,
    read by ``lga_lora_gemv_rows`` itself, so a captured step follows ``assign``. ``select`` is the host-side choice of
    the one-sequence calls (prefill, ``generate``): those run the single-adapter kernels on adapter i's views."""

    def __init__(self, n: int, device) -> None:
        self.n = int(n)
        self.rows = torch.full((ops.MAX_GEMV_ROWS,), -1, dtype=torch.int32, device=device)
        self.selected: Optional[int] = None

    def check(self, i: Optional[int], who: str = "AdapterSet") -> Optional[int]:
        if i is None:
            return None
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < self.n:
            raise ValueError(f"{who}: adapter {i!r} is not None or an index into the set's {self.n} adapters")
        return i

    def assign(self, b: int, i: Optional[int]) -> None:
        """Row (slot) b of the batched step runs adapter i from now on, None = no adapter: a stream-ordered device
        write."""
        if not 0 <= b < self.rows.numel():
            raise ValueError(f"AdapterSet.assign: row {b} of {self.rows.numel()}")
        i = self.check(i, "AdapterSet.assign")
        self.rows[b:b + 1].fill_(-1 if i is None else i)

    def select(self, i: Optional[int]) -> "AdapterSet":
        """One-sequence calls run adapter i from now on, None = the plain base model."""
        self.selected = self.check(i, "AdapterSet.select")
        return self


class MultiLoraLinear(quantize._Kernels, nn.Module):
    """A base Linear with the n adapters of an ``AdapterSet`` stacked next to it: ``lora_A`` (n, R, K) and ``lora_B``
    (n, N, r), adapter i of each with the bits ``build_layout`` gives that adapter alone; ``row_off`` and ``scaling``
    are shared (one ``Config`` for the set). One row or a prefill runs as ``LoraLinear`` does on the views of the
    set's selected adapter, or as the plain base without one. The batched decode step (``gemv_rows``) runs the base's
    rows GEMV and ONE ``lga_lora_gemv_rows`` in place, every row with the adapter ``adapters.rows`` names."""

    def __init__(self, base: nn.Module, lora_A: torch.Tensor, lora_B: torch.Tensor, row_off: Optional[torch.Tensor],
                 scaling: float, adapters: AdapterSet) -> None:
        super().__init__()
        k = quantize.kernels(base)
        if k.act_dtype != torch.bfloat16:
            raise NotImplementedError("a LoRA adapter on an fp32 Linear (--precision 32-true): the adapter kernels "
                                      "compute in bf16 (bf16-true)")
        dev = base.weight.device
        self.base = base
        self._kernels = k
        self.adapters = adapters
        self.in_features, self.out_features = k.in_features, k.out_features
        self.register_buffer("lora_A", lora_A.to(device=dev, dtype=torch.bfloat16).contiguous())
        self.register_buffer("lora_B", lora_B.to(device=dev, dtype=torch.bfloat16).contiguous())
        self.register_buffer("row_off", None if row_off is None else row_off.to(device=dev, dtype=torch.int32))
        self.scaling = float(scaling)
        if self.lora_A.dim() != 3 or self.lora_B.dim() != 3 or not self.lora_A.shape[0] == self.lora_B.shape[0] == adapters.n:
            raise ValueError(f"stacked adapters lora_A {tuple(self.lora_A.shape)} / lora_B {tuple(self.lora_B.shape)} "
                             f"for a set of {adapters.n}")
        ops._lora_dims(self.lora_A[0], self.lora_B[0], self.row_off, "MultiLoraLinear")
        if self.lora_A.shape[2] != self.in_features or self.lora_B.shape[1] != self.out_features:
            raise ValueError(f"adapters for ({self.lora_B.shape[1]}, {self.lora_A.shape[2]}) on a Linear of "
                             f"({self.out_features}, {self.in_features})")

    @property
    def weight(self) -> torch.Tensor:
        return self.base.weight

    @property
    def bias(self) -> Optional[torch.Tensor]:
        return self.base.bias

    def gemv_fuses_norm(self, dual: bool = False) -> bool:
        return self._kernels.gemv_fuses_norm(dual)

    def pairs_with(self, o) -> bool:  # as LoraLinear: two Linears + lga_swiglu
        return False

    def gemv(self, x, res, norm_weight, eps):
        i = self.adapters.selected
        if i is None:
            return self._kernels.gemv(x, res, norm_weight, eps)
        y = self._kernels.gemv(x, None, norm_weight, eps).view(-1)
        return ops.lora_gemv(x, self.lora_A[i], self.lora_B[i], self.row_off, self.scaling, base=y, residual=res,
                             norm_weight=norm_weight, eps=eps, out=y)

    def gemm(self, x, res):
        i = self.adapters.selected
        if i is None:
            return self._kernels.gemm(x, res)
        y = self._kernels.gemm(x, None)
        t = ops.lora_down(x, self.lora_A[i])
        return ops.lora_up(t, self.lora_B[i], self.row_off, self.scaling, base=y, residual=res, out=y)

    def gemv_rows(self, x, res, norm_weight, eps):
        y = self._kernels.gemv_rows(x, None, norm_weight, eps).view(x.shape[0], self.out_features)
        return ops.lora_gemv_rows(x, self.lora_A, self.lora_B, self.row_off, self.adapters.rows[:x.shape[0]],
                                  self.scaling, base=y, residual=res, norm_weight=norm_weight, eps=eps, out=y)

    def extra_repr(self) -> str:
        n, R, _ = self.lora_A.shape
        return f"adapters={n}, r={self.lora_B.shape[2]}, segments={R // self.lora_B.shape[2]}, scaling={self.scaling}"


def _targets(model, config: Config) -> Dict[str, Tuple[nn.Module, str, Optional[tuple]]]:
    """Reference key prefix -> (parent module, attribute, qkv geometry or None) of every Linear the config adapts."""
    out: Dict[str, Tuple[nn.Module, str, Optional[tuple]]] = {}
    enable = (config.to_query, config.to_key, config.to_value)
    for i, block in enumerate(model.transformer.h):
        pre = f"transformer.h.{i}"
        if any(enable):
            out[f"{pre}.attn.attn"] = (block.attn, "attn", (config.n_head, config.n_query_groups, enable))
        if config.to_projection:
            out[f"{pre}.attn.proj"] = (block.attn, "proj", None)
        if config.to_mlp:
            for name in {"LLaMAMLP": ("fc_1", "fc_2", "proj"), "GptNeoxMLP": ("fc", "proj")}[config._mlp_class]:
                out[f"{pre}.mlp.{name}"] = (block.mlp, name, None)
    if config.to_head:
        out["lm_head"] = (model, "lm_head", None)
    return out


def _checked_state(lora_state, targets) -> Dict[str, torch.Tensor]:
    """The adapter tensors of ``lora_state`` (flat or nested under ``"model"``), whose ``lora_`` keys must be exactly
    those of ``targets``."""
    state = lora_state.get("model", lora_state)
    lora_keys = {k for k in state if "lora_" in k}
    want = {f"{p}.{ab}" for p in targets for ab in ("lora_A", "lora_B")}
    if lora_keys != want:
        missing, surplus = sorted(want - lora_keys), sorted(lora_keys - want)
        raise KeyError(f"adapter checkpoint does not match the LoRA config: missing {missing[:4]} "
                       f"({len(missing)} in all), not targeted by the config {surplus[:4]} ({len(surplus)} in all)")
    return state


def _refuse_adapted(model) -> None:
    for m in model.modules():
        if isinstance(m, (LoraLinear, MultiLoraLinear)):
            raise RuntimeError("the model already carries a LoRA adapter")


def attach(model, lora_state: Dict[str, torch.Tensor], config: Config):
    """Swap the Linears that ``config`` targets for ``LoraLinear`` carrying the adapter tensors of ``lora_state``: the
    reference's key names (``transformer.h.0.attn.attn.lora_A``, ``...mlp.fc_1.lora_B``, ``lm_head.lora_A``, ...),
    directly or nested under ``"model"`` (what finetune/lora.py saves). Keys without ``lora_`` are ignored (a full
    checkpoint may be passed); a missing, surplus or mis-shaped adapter tensor raises. Returns the model."""
    from lit_gpt import comm

    group = comm.get_default()  # a tensor-parallel group that is up: the model's Linears are its shards
    dtype = model.transformer.wte.weight.dtype
    check_supported(config, precision="32-true" if dtype == torch.float32 else "bf16-true",
                    world_size=1 if group is None else group.world)
    targets = _targets(model, config)
    state = _checked_state(lora_state, targets)
    _refuse_adapted(model)
    new = {}
    for prefix, (parent, name, qkv) in targets.items():  # every layout first: a bad tensor leaves the model as it was
        base = getattr(parent, name)
        A, B, row_off = build_layout(state[f"{prefix}.lora_A"].detach().float().cpu(),
                                     state[f"{prefix}.lora_B"].detach().float().cpu(), config.r, base.out_features,
                                     qkv)
        if A.shape[1] != base.in_features:
            raise ValueError(f"{prefix}.lora_A has {A.shape[1]} columns, the Linear {base.in_features} inputs")
        new[prefix] = (parent, name, base, A, B, row_off)
    for parent, name, base, A, B, row_off in new.values():
        setattr(parent, name, LoraLinear(base, A, B, row_off, config.alpha / config.r))
    return model


def attach_many(model, lora_states: Sequence[Dict[str, torch.Tensor]], config: Config) -> AdapterSet:
    """Attach several adapters of ONE ``config`` (same r, alpha and targets) to a model for batched serving: every
    targeted Linear becomes a ``MultiLoraLinear`` holding the adapters stacked, adapter i in the layout ``attach``
    gives it alone. Each state is checked as ``attach`` checks its own (a missing, surplus or mis-shaped tensor
    raises and leaves the model as it was), and an already-adapted model is refused. Returns the ``AdapterSet``, also
    kept as ``model.lora_adapters``: ``select(i)`` for one-sequence calls, ``assign(b, i)`` for the rows of a batched
    decode step (generate.base.generate_batch / generate_continuous take ``adapters=[...]``)."""
    from lit_gpt import comm

    if len(lora_states) == 0:
        raise ValueError("attach_many: no adapters")
    group = comm.get_default()
    dtype = model.transformer.wte.weight.dtype
    check_supported(config, precision="32-true" if dtype == torch.float32 else "bf16-true",
                    world_size=1 if group is None else group.world)
    targets = _targets(model, config)
    states = [_checked_state(s, targets) for s in lora_states]
    _refuse_adapted(model)
    if getattr(model, "lora_adapters", None) is not None:
        raise RuntimeError("the model already carries a LoRA adapter")
    adapters = AdapterSet(len(states), model.transformer.wte.weight.device)
    new = []
    for prefix, (parent, name, qkv) in targets.items():  # every layout first: a bad tensor leaves the model as it was
        base = getattr(parent, name)
        layouts = [build_layout(st[f"{prefix}.lora_A"].detach().float().cpu(),
                                st[f"{prefix}.lora_B"].detach().float().cpu(), config.r, base.out_features, qkv)
                   for st in states]
        if layouts[0][0].shape[1] != base.in_features:
            raise ValueError(f"{prefix}.lora_A has {layouts[0][0].shape[1]} columns, the Linear {base.in_features} "
                             "inputs")
        new.append((parent, name, base, torch.stack([l[0] for l in layouts]), torch.stack([l[1] for l in layouts]),
                    layouts[0][2]))  # (row_off depends on the config alone)
    for parent, name, base, A, B, row_off in new:
        setattr(parent, name, MultiLoraLinear(base, A, B, row_off, config.alpha / config.r, adapters))
    model.lora_adapters = adapters
    return adapters


def merge_lora_weights(model) -> None:
    """Fold every adapter into its base weight (reference lora.py:724-728, LoRALinear.merge :140-149 with its bf16
    roundings) and put the plain ``nn.Linear`` back, so every fusion of the adapter-free model and its decode speed
    return. bf16 bases only: a quantized base raises before anything is merged."""
    found = [(parent, name, m) for parent in model.modules() for name, m in parent.named_children()
             if isinstance(m, LoraLinear)]
    for _, name, m in found:
        if not (type(m.base) is nn.Linear and m.base.weight.dtype == torch.bfloat16):
            raise NotImplementedError(
                f"merge_lora_weights: {name} has a {type(m.base).__name__} base. Merging into a quantized weight means "
                "dequantize, add, quantize again, which rounds the adapter's small update to the quantization step; the "
                "adapter runs next to the quantized weight instead (the run-time path, --no-merge)")
    for parent, name, m in found:
        ops.lora_merge(m.base.weight.data, m.lora_A, m.lora_B, m.row_off, m.scaling)
        setattr(parent, name, m.base)


def random_adapter(config: Config, seed: int = 1234, b_std: float = 0.02) -> Dict[str, torch.Tensor]:
    """A seeded random adapter in the reference's key names and shapes (``--synthetic``, tools, tests): ``lora_A`` as
    the reference initialises it (kaiming-uniform, lora.py:135), ``lora_B`` normal with ``b_std`` (the reference's zero
    init would leave the model unchanged)."""
    g = torch.Generator().manual_seed(seed)
    c, r = config, config.r
    kv = c.n_query_groups * c.head_size
    enable = (config.to_query, config.to_key, config.to_value)
    shapes: Dict[str, Tuple[int, int, int]] = {}  # prefix -> (rows of A, K, rows of B)
    for i in range(c.n_layer):
        pre = f"transformer.h.{i}"
        if any(enable):
            rows = c.n_embd * enable[0] + kv * enable[1] + kv * enable[2]
            shapes[f"{pre}.attn.attn"] = (r * sum(enable), c.n_embd, rows)
        if config.to_projection:
            shapes[f"{pre}.attn.proj"] = (r, c.n_embd, c.n_embd)
        if config.to_mlp and c._mlp_class == "LLaMAMLP":
            shapes[f"{pre}.mlp.fc_1"] = shapes[f"{pre}.mlp.fc_2"] = (r, c.n_embd, c.intermediate_size)
            shapes[f"{pre}.mlp.proj"] = (r, c.intermediate_size, c.n_embd)
        elif config.to_mlp and c._mlp_class == "GptNeoxMLP":
            shapes[f"{pre}.mlp.fc"] = (r, c.n_embd, c.intermediate_size)
            shapes[f"{pre}.mlp.proj"] = (r, c.intermediate_size, c.n_embd)
    if config.to_head:
        shapes["lm_head"] = (r, c.n_embd, c.padded_vocab_size)
    out = {}
    for prefix, (ra, K, rb) in shapes.items():
        bound = 1.0 / K ** 0.5  # kaiming_uniform_(a=sqrt(5)) on (r, K): U(-1/sqrt(K), 1/sqrt(K))
        out[f"{prefix}.lora_A"] = (torch.rand(ra, K, generator=g) * 2 - 1) * bound
        out[f"{prefix}.lora_B"] = torch.randn(rb, r, generator=g) * b_std
    return out
