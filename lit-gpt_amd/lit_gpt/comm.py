"""Tensor-parallel all-reduce for decode activations over xGMI peer memory (``lga_allreduce_bf16``).

The reference sums the row-parallel partial outputs with a collective in a forward hook
(/root/reference/generate/tp.py:73-74, ``all_reduce(outs, "sum", list(range(world_size)))``), 64 times per
Llama-2-7B token. ``XgmiAllReduce`` is the MI355X replacement for those one-token messages: every rank owns a
mailbox (uncached HBM, IPC-exported), the handles are exchanged once over the process group, and each call is
ONE single-workgroup kernel that pushes the partial into every peer's mailbox, waits for the peers' flags and
sums the ranks in order 0..W-1 (bit-identical on every rank), optionally adding the Block residual. The launch
is graph-capturable. Prefill-sized messages (more than ``cap`` elements) stay on ``torch.distributed``
(RCCL over xGMI with the ``nccl`` backend).

One process per GPU, all ranks of the group on this node (xGMI / same-device IPC). Ranks may also share one GPU
(tests run two ranks on cuda:0 with a gloo group for the handle exchange).
"""

from __future__ import annotations

import ctypes
import os
import socket
from typing import List, Optional

import torch
import torch.distributed as dist

from lit_gpt import ops, quantize

DEFAULT_CAP = 32768  # bf16 elements per message (64 KB): decode activations of every config (k * C for MoE)

_default: Optional["XgmiAllReduce"] = None
fallback_reason: Optional[str] = None  # why init_distributed fell back to RCCL (None: it did not)


# lga_comm_trace's device buffer: allocated once per process and never freed (graphs may hold its pointer)
_TRACE_BUF = None

class XgmiUnavailable(RuntimeError):
    """Raised on EVERY rank (the outcome is agreed over the group) when the peer mailboxes cannot be mapped or the
    start-up self-test of the one-shot all-reduce fails."""


class XgmiAllReduce:
    def __init__(self, group=None, device: Optional[torch.device] = None, cap: int = DEFAULT_CAP) -> None:
        lib = ops.load_library()
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        if not 1 <= self.world <= 8:
            raise ValueError(f"XgmiAllReduce supports 1..8 ranks, got {self.world}")
        self.cap = cap
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        nbytes = lib.lga_comm_mailbox_bytes(cap)
        handle = ctypes.create_string_buffer(64)
        own = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            ops._check(lib.lga_comm_alloc(nbytes, ctypes.byref(own), handle))
        self._own = own
        handles: List[Optional[bytes]] = [None] * self.world
        dist.all_gather_object(handles, bytes(handle.raw), group=group)
        ptrs = []
        self._opened = []
        failure = None
        with torch.cuda.device(self.device):
            for r, h in enumerate(handles):
                if r == self.rank:
                    ptrs.append(own.value)
                    continue
                p = ctypes.c_void_p()
                try:
                    ops._check(lib.lga_comm_open(h, ctypes.byref(p)))
                except RuntimeError as e:  # agreed below, so no rank waits on a peer that gave up
                    failure = f"rank {self.rank}: mapping rank {r}'s mailbox failed: {e}"
                    break
                self._opened.append(p)
                ptrs.append(p.value)
        self.seq = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        # lga_q4_gemv_allreduce's arrival counters (9 words at a 256-B stride) + the tagged form's launch counter
        self.arrive = torch.zeros(10 * 64, dtype=torch.int32, device=self.device)
        # the fused row-parallel GEMV's protocol: "tagged" (granules; every workgroup waits only for other ranks)
        # when every rank owns its GPU, "flags" (last arriver, one workgroup waits) when ranks share a device — the
        # one-GPU tests and rehearsals, where the tagged form's waiting workgroups of one rank could occupy the CUs
        # the others' kernels need. LGA_AR_PROTOCOL=flags|tagged overrides.
        self.protocol = self._choose_protocol(group)
        self._agree(failure, "mailbox mapping")
        self._mailboxes = (ctypes.c_void_p * self.world)(*ptrs)
        self._self_test()
        self.fused_ok = True  # lga_q4_gemv_allreduce passed its own self-test (else linear_reduce uses two launches)
        self.fused_fallback: Optional[str] = None
        self._self_test_fused()

    def _choose_protocol(self, group) -> str:
        env = os.environ.get("LGA_AR_PROTOCOL", "auto")
        if env in ("flags", "tagged"):
            return env
        ident = str(getattr(torch.cuda.get_device_properties(self.device), "uuid", self.device.index))
        ids: List[Optional[str]] = [None] * self.world
        dist.all_gather_object(ids, (socket.gethostname(), ident), group=group)
        return "tagged" if len(set(ids)) == self.world else "flags"

    def _agree(self, failure: Optional[str], what: str) -> None:
        """All ranks learn whether any rank failed (MIN over a flag); on failure every rank raises."""
        flag = torch.tensor([0 if failure else 1], dtype=torch.int32,
                            device=self.device if dist.get_backend(self.group) == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
        if int(flag.item()) == 0:
            self.close()
            raise XgmiUnavailable(failure or f"{what} failed on another rank")

    def _self_test(self) -> None:
        """One reduction of known values (rank r contributes r + 1 at every element, + a residual of 0.5): checks
        that the peers' pushes and flags are visible through the mapped memory before any real call trusts it. A
        launch error on one rank is caught and agreed like a wrong sum, so no peer is left waiting in the
        collective."""
        n = 1024
        want = float(self.world * (self.world + 1) // 2) + 0.5
        failure = None
        try:
            x = torch.full((n,), float(self.rank + 1), dtype=torch.bfloat16, device=self.device)
            res = torch.full((n,), 0.5, dtype=torch.bfloat16, device=self.device)
            with torch.cuda.device(self.device):
                y = self.all_reduce(x, residual=res)
                torch.cuda.synchronize(self.device)
            if self.errors():
                failure = f"rank {self.rank}: self-test timed out waiting for a peer"
            elif not bool((y.float() == want).all()):
                failure = f"rank {self.rank}: self-test sum wrong ({y.float()[:4].tolist()} vs {want})"
        except Exception as e:  # noqa: BLE001 - any launch / runtime error is this rank's failure, agreed below
            failure = f"rank {self.rank}: self-test raised {type(e).__name__}: {e}"
        self._agree(failure, "self-test")

    def _self_test_fused(self, n: int = 512, k: int = 1024, calls: int = 4) -> None:
        """The fused row-parallel GEMV + all-reduce against the two-launch form (GEMV, then ``all_reduce`` with the
        residual) it must equal bit for bit: ``calls`` back-to-back launches of per-rank weights. Its cross-GPU
        hand-off (every workgroup's pushes, then the last arriver's flags) is a different protocol from the one-shot
        kernel's, so it is checked on its own; when it fails on any rank, every rank keeps the xGMI one-shot
        all-reduce and only the fusion is dropped (``fused_ok``, ``fused_fallback``). A timeout or a launch error on
        any rank instead raises ``XgmiUnavailable`` on every rank (RCCL for all decode all-reduces)."""
        import types

        g = torch.Generator().manual_seed(1000 + self.rank)
        failure = None
        code = 0  # 0 ok; 1 results differ (drop the fusion only); 2 a peer timed out or a launch raised
        try:
            w = (torch.randn(n, k, generator=g) * 0.02).to(self.device)
            x = torch.randn(k, generator=g).bfloat16().to(self.device)
            res = torch.randn(n, generator=g).bfloat16().to(self.device)
            with torch.cuda.device(self.device):
                qw, sc = ops.quantize(w, ops.FMT_Q4G, 128)
                lin = types.SimpleNamespace(out_features=n, in_features=k, qweight=qw, scales=sc, bias=None,
                                            group=128, fmt=ops.FMT_Q4G)
                want = self.all_reduce(ops.q4_gemv(x, qw, sc, n, k, 128, ops.FMT_Q4G), residual=res)
                got = [self.gemv_all_reduce(lin, x, residual=res) for _ in range(calls)]
                torch.cuda.synchronize(self.device)
            if self.errors():
                code, failure = 2, f"rank {self.rank}: fused GEMV all-reduce self-test timed out waiting for a peer"
            else:
                bad = [i for i, y in enumerate(got) if not torch.equal(y, want)]
                if bad:
                    code = 1
                    failure = f"rank {self.rank}: fused GEMV all-reduce differs from GEMV + all-reduce at calls {bad}"
        except Exception as e:  # noqa: BLE001 - agreed below so that no peer waits in the collective
            code, failure = 2, f"rank {self.rank}: fused GEMV all-reduce self-test raised {type(e).__name__}: {e}"
        flag = torch.tensor([code], dtype=torch.int32,
                            device=self.device if dist.get_backend(self.group) == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.group)
        agreed = int(flag.item())
        if agreed == 2:
            # a timeout leaves the mailboxes' sequence flags out of step between the ranks, and the one-shot kernel
            # uses the same mailboxes, flags and counter: every rank leaves xGMI for RCCL
            self.close()
            raise XgmiUnavailable(failure or "fused GEMV all-reduce self-test timed out or raised on another rank")
        if agreed == 1:
            self.fused_ok = False
            self.fused_fallback = failure or "fused GEMV all-reduce self-test failed on another rank"

    def supports(self, t: torch.Tensor) -> bool:
        return (t.is_cuda and t.dtype == torch.bfloat16 and t.numel() <= self.cap and t.numel() % 8 == 0
                and t.is_contiguous())

    def all_reduce(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bf16(sum over ranks of x) (+ residual, rounded as the Block's ``x + h``); a new tensor unless ``out``."""
        if not self.supports(x):
            raise ValueError(f"XgmiAllReduce: needs a contiguous bf16 GPU tensor of <= {self.cap} elements "
                             f"(multiple of 8), got {tuple(x.shape)} {x.dtype}")
        y = out if out is not None else torch.empty_like(x)
        res = None
        if residual is not None:
            if residual.numel() != x.numel():
                raise ValueError("XgmiAllReduce: residual shape differs from x")
            res = ops._dev(residual.contiguous(), "residual", torch.bfloat16)
        ops._check(ops.load_library().lga_allreduce_bf16(
            ops._dev(x, "x", torch.bfloat16), res, ops._dev(y, "y", torch.bfloat16), x.numel(), self._mailboxes,
            self.rank, self.world, self.cap, self.seq.data_ptr(), self.err.data_ptr(), ops._stream()))
        return y

    def gemv_all_reduce(self, lin, x: torch.Tensor, residual: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bf16(sum over ranks of ``lin(x)``) (+ residual) for a one-token row-parallel ``QuantLinear``, in ONE launch
        (``lga_q4_gemv_allreduce``): the GEMV's workgroups push their partial rows into the mailboxes and the last
        one sums the ranks. Bit-identical to ``all_reduce(lin(x), residual)``."""
        N, K = lin.out_features, lin.in_features
        if x.numel() != K or not self.supports_rows(N):
            raise ValueError(f"XgmiAllReduce.gemv_all_reduce: needs one row of {K} and N % 8 == 0, N <= {self.cap}")
        y = out if out is not None else torch.empty(N, dtype=torch.bfloat16, device=x.device)
        res = None
        if residual is not None:
            if residual.numel() != N:
                raise ValueError("XgmiAllReduce.gemv_all_reduce: residual shape differs from the output")
            res = ops._dev(residual.contiguous(), "residual", torch.bfloat16)
        lib = ops.load_library()
        fn = lib.lga_q4_gemv_allreduce_tagged if self.protocol == "tagged" else lib.lga_q4_gemv_allreduce
        ops._check(fn(
            ops._dev(x.contiguous(), "x", torch.bfloat16), ops._dev(lin.qweight, "qweight", torch.uint8),
            ops._dev(lin.scales, "scales"), ops._opt(lin.bias, "bias", torch.bfloat16), res,
            ops._dev(y, "y", torch.bfloat16), N, K, lin.group, lin.fmt, self._mailboxes, self.rank, self.world,
            self.cap, self.seq.data_ptr(), self.arrive.data_ptr(), self.err.data_ptr(), ops._stream()))
        return y

    def enable_trace(self, n_records: int = 256) -> None:
        """Diagnostics (lga_comm_trace): every later all-reduce launch of this process records its call — entry,
        flags-raised and wait-done times, timeout, the peers' flag words seen — in a device buffer (``traces()``).
        Process-wide; install it before capturing graphs that should record. Graphs captured with tracing on keep its
        device pointer, so the buffer lives for the rest of the process: a second call (or one after ``close()``)
        re-installs the same buffer instead of freeing it under such graphs; asking for more records raises."""
        global _TRACE_BUF
        if _TRACE_BUF is None:
            _TRACE_BUF = torch.zeros(n_records, 16, dtype=torch.int64, device=self.device)
        elif _TRACE_BUF.size(0) < n_records or _TRACE_BUF.device != torch.device(self.device):
            raise ValueError("enable_trace: the process-wide trace buffer exists with fewer records or on another "
                             "device; it cannot be replaced while captured graphs may still write into it")
        self._trace = _TRACE_BUF
        ops._check(ops.load_library().lga_comm_trace(self._trace.data_ptr(), self._trace.size(0)))

    def traces(self):
        """The recorded calls as a (n, 16) int64 numpy array (rows of calls not made are zero); syncs."""
        torch.cuda.synchronize(self.device)
        return self._trace.cpu().numpy()

    def supports_rows(self, n: int) -> bool:
        return 0 < n <= self.cap and n % 8 == 0

    def errors(self) -> int:
        """Non-zero when a call timed out waiting for a peer since the last check (syncs; clears the word)."""
        e = int(self.err.item())
        self.err.zero_()
        return e

    def close(self) -> None:
        lib = ops.load_library()
        torch.cuda.synchronize(self.device)
        if getattr(self, "_trace", None) is not None:
            lib.lga_comm_trace(None, 0)  # later launches stop recording; _TRACE_BUF itself stays alive (enable_trace)
            self._trace = None
        self._mailboxes = None
        for p in self._opened:
            lib.lga_comm_close(p)
        self._opened = []
        if self._own is not None:
            lib.lga_comm_free(self._own)
            self._own = None


class AllReduceTimeout(RuntimeError):
    """An xGMI all-reduce gave up waiting for a peer (5 s bound in the kernel): the logits of that step were
    summed from partial data, so the run is void. Raised on every rank (the outcome is agreed over the group)."""


def check_errors(comm: Optional["XgmiAllReduce"] = None) -> None:
    """Collective: every rank reports whether any of its all-reduce calls since the last check timed out, the
    ranks agree (MAX over the group) and all of them raise ``AllReduceTimeout`` if one did. Call it at the same
    point on every rank (generate() does after each run, bench.py after the timed region). No-op without an
    installed communicator."""
    comm = comm or _default
    if comm is None:
        return
    mine = comm.errors()
    flag = torch.tensor([1 if mine else 0], dtype=torch.int32,
                        device=comm.device if dist.get_backend(comm.group) == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=comm.group)
    if int(flag.item()):
        raise AllReduceTimeout(f"rank {comm.rank}: an xGMI all-reduce timed out waiting for a peer "
                               f"({'this rank' if mine else 'another rank'}); the generated tokens are invalid")


def set_default(comm: Optional[XgmiAllReduce]) -> None:
    """Install the communicator the TP hooks (generate/tp.py all_reduce_output) use for small messages."""
    global _default
    _default = comm


def get_default() -> Optional[XgmiAllReduce]:
    return _default


def all_reduce_output(world_size: int, module: torch.nn.Module, ins, outs) -> torch.Tensor:
    """The TP forward hook (reference generate/tp.py:73-74): sum the row-parallel partial outputs over the ranks.
    One-token messages go through the xGMI one-shot kernel when a communicator is installed; everything else
    (prefill, CPU / gloo groups) through ``torch.distributed.all_reduce`` (RCCL with the ``nccl`` backend)."""
    if world_size <= 1:
        return outs
    comm = _default
    if comm is not None and comm.world == world_size and comm.supports(outs):
        return comm.all_reduce(outs)
    dist.all_reduce(outs, op=dist.ReduceOp.SUM)
    return outs


def tp_hook(module: torch.nn.Module):
    """The ``all_reduce_output`` hook when it is the module's only forward hook (then Block may run the module
    without hooks and fuse the reduction with the residual add); None otherwise."""
    import functools

    hooks = list(module._forward_hooks.values())
    if len(hooks) == 1 and isinstance(hooks[0], functools.partial) and hooks[0].func is all_reduce_output:
        return hooks[0]
    return None


def linear_reduce(hook, lin: torch.nn.Module, x: torch.Tensor, residual: Optional[torch.Tensor],
                  compute) -> torch.Tensor:
    """The row-parallel Linear under TP, its all-reduce hook and the Block residual add: ONE fused launch
    (``XgmiAllReduce.gemv_all_reduce``) for a one-token 4-bit Linear when a communicator is installed, else
    ``compute()`` (the plain Linear) followed by the hook's reduction (+ residual)."""
    comm = _default
    world = hook.args[0]
    if (comm is not None and comm.world == world and quantize.gemv_allreduce_supported(lin, x)
            and comm.supports_rows(lin.out_features) and (residual is None or residual.numel() == lin.out_features)
            and fused_gemv_allreduce and getattr(comm, "fused_ok", True)):
        y = comm.gemv_all_reduce(lin, x.reshape(-1), residual)
        return y.view(*x.shape[:-1], lin.out_features)
    h = compute()
    if residual is None:
        return hook(lin, (), h)
    return reduce_add(hook, lin, h, residual)


# the fused row-parallel GEMV + all-reduce (lga_q4_gemv_allreduce); False keeps the two-launch form (tests A/B them)
fused_gemv_allreduce = True


def reduce_add(hook, module: torch.nn.Module, h: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """residual + all_reduce(h), the Block's ``x + attn(...)`` / ``x + mlp(...)`` under TP: one fused kernel for
    decode messages, else the hook's collective followed by the bf16 add."""
    comm = _default
    world = hook.args[0]
    if comm is not None and comm.world == world and comm.supports(h) and residual.numel() == h.numel():
        return comm.all_reduce(h, residual=residual.contiguous()).view_as(residual)
    h = hook(module, (), h)
    return ops.add(h.contiguous(), residual.contiguous()).view_as(residual)
