"""Bit comparison of decode-attention builds in ONE process: every attention entry point on identical inputs through
each library, the outputs compared bit for bit (y, the appended K / V rows, for fp8 caches the codes and scales, and
once per geometry the whole caches). For a change that must not move a bit: build the parent beside the tree
(`git archive <rev> lit-gpt_amd include`, `make OUT=...`) and compare the two; a library against itself is the tool's
own sanity check.

usage: AB_LIBS=parent.so,lit-gpt_amd/lit_gpt/_lib/liblitgpt_amd.so python tools/attn_bits.py
Exit status 1 names the first differing case. The shapes are the smallest that reach every path of the kernels: H = 8
with q_per_kv 1, 2, 4, 8 (and Llama-2-7B's 32 / 32 for its (UNR, NW) choice), max_seq 320, 1 / 2 / 5 splits (with
the launch's own head slices and, for q_per_kv > 1, with LGA_ATTN_HSPLIT=1: all heads in one workgroup), positions
that give empty splits, a step ending exactly at k_end, the new key in the first, a middle and the last split, and the
last cache row. A few seconds on one MI355X.
"""

import math
import os
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "lit-gpt_amd"), str(REPO)]

from lit_gpt import ops  # noqa: E402

S, HS, SLOTS = 320, 128, 8
GEOMETRIES = [(8, 8), (8, 4), (8, 2), (8, 1), (32, 32)]  # (H, G)
SPLITS = [1, 2, 5]
POSITIONS = [0, 1, 63, 64, 65, 200, 319]
WINDOWS = [1, 3, 8]
BATCHES = [1, 3, 4, 5, 8]


class Side:
    """One library and its own copies of every buffer a launch writes (the caches start out identical)."""

    def __init__(self, lib, base):
        self.lib = lib
        self.t = {k: v.clone() for k, v in base.items()}
        self.ws = {}

    def workspace(self, rows, H, G, hs, n_splits):
        key = (rows, H, G, hs, n_splits)
        if key not in self.ws:
            self.ws[key] = ops.AttentionWorkspace(*key, self.t["k"].device)
        return self.ws[key]


def make_inputs(H, G, dev, gen):
    def rn(*shape):
        return torch.randn(*shape, device=dev, generator=gen)

    theta = 1.0 / (10000 ** (torch.arange(0, HS // 2, device=dev).float() / (HS // 2)))
    ang = torch.outer(torch.arange(S, device=dev).float(), theta).repeat(1, 2)
    codes = lambda: (torch.randint(0, 127, (SLOTS, G, S, HS), device=dev, generator=gen)  # noqa: E731 (no NaN code)
                     + 128 * torch.randint(0, 2, (SLOTS, G, S, HS), device=dev, generator=gen)).to(torch.uint8)
    scales = lambda: torch.exp2(torch.randint(-9, -4, (SLOTS, G, S), device=dev, generator=gen).float())  # noqa: E731
    const = {"qkv": rn(SLOTS, (H + 2 * G) * HS).bfloat16(), "q": rn(len(POSITIONS), H, HS).bfloat16(),
             "q64": rn(len(POSITIONS), H, 64).bfloat16(), "cos": ang.cos().contiguous(), "sin": ang.sin().contiguous()}
    written = {"k": rn(SLOTS, G, S, HS).bfloat16(), "v": rn(SLOTS, G, S, HS).bfloat16(),
               "k64": rn(G, S, 64).bfloat16(), "v64": rn(G, S, 64).bfloat16(),
               "kc8": codes(), "vc8": codes(), "ks8": scales(), "vs8": scales()}
    return const, written


def cases(H, G, n_splits, dev):
    """(name, run(side) -> tensors to compare) for one geometry and split count."""
    a = (H, G, HS, HS, 1.0 / math.sqrt(HS), n_splits)
    pos_all = torch.tensor(POSITIONS, device=dev)

    def rows_written(side, names, slots, p):  # row p of the listed slots of each named cache
        return [side.t[n][slots, :, p] for n in names]

    def kv8(side, slots=None):
        return tuple(side.t[n] if slots is None else side.t[n][slots] for n in ("kc8", "vc8", "ks8", "vs8"))

    for hs, kq, kk, kvv in ((HS, "q", "k", "v"), (64, "q64", "k64", "v64")):  # lga_attention, T < 16
        def rows(side, c, T=None, hs=hs, kq=kq, kk=kk, kvv=kvv):
            q = c[kq] if T is None else c[kq][T:T + 1]
            ip = pos_all if T is None else pos_all[T:T + 1]
            kc, vc = (side.t[kk][0], side.t[kvv][0]) if hs == HS else (side.t[kk], side.t[kvv])
            n = q.shape[0]
            return [ops.attention(q, kc, vc, ip, H, G, hs, 1.0 / math.sqrt(hs), n_splits,
                                  side.workspace(n, H, G, hs, n_splits) if n_splits > 1 else None)]
        yield f"attention hs={hs} T={len(POSITIONS)}", rows
        for i, p in enumerate(POSITIONS):
            yield f"attention hs={hs} T=1 p={p}", (lambda side, c, i=i, rows=rows: rows(side, c, i))
    for p in POSITIONS:
        pos = torch.tensor([p], device=dev)

        def fused(side, c, pos=pos, p=p):
            y = ops.attention_decode_fused(c["qkv"][:1], side.t["k"][0], side.t["v"][0], pos, pos, c["cos"], c["sin"],
                                           *a, side.workspace(1, H, G, HS, n_splits))
            return [y] + rows_written(side, ("k", "v"), 0, p)

        def fused8(side, c, pos=pos, p=p):
            y = ops.attention_decode_fused_kv8(c["qkv"][:1], kv8(side, 0), pos, pos, c["cos"], c["sin"], *a,
                                               side.workspace(1, H, G, HS, n_splits))
            return [y] + rows_written(side, ("kc8", "vc8", "ks8", "vs8"), 0, p)

        yield f"decode_fused p={p}", fused
        yield f"decode_fused_kv8 p={p}", fused8
        for M in WINDOWS:
            p0 = min(p, S - M)  # (every row of the window inside the cache)
            pos0 = torch.tensor([p0], device=dev)

            def window(side, c, M=M, p0=p0, pos0=pos0, fp8=False):
                ws = side.workspace(M, H, G, HS, n_splits) if n_splits > 1 else None
                if fp8:
                    y = ops.attention_decode_window_kv8(c["qkv"][:M], kv8(side, 0), pos0, c["cos"], c["sin"], *a, ws)
                    names = ("kc8", "vc8", "ks8", "vs8")
                else:
                    y = ops.attention_decode_window(c["qkv"][:M], side.t["k"][0], side.t["v"][0], pos0, c["cos"],
                                                    c["sin"], *a, ws)
                    names = ("k", "v")
                return [y] + [side.t[n][0, :, p0:p0 + M] for n in names]

            yield f"decode_window M={M} pos0={p0}", window
            yield f"decode_window_kv8 M={M} pos0={p0}", (lambda side, c, w=window: w(side, c, fp8=True))
        for B in BATCHES:
            bpos = torch.tensor([POSITIONS[(POSITIONS.index(p) + b) % len(POSITIONS)] for b in range(B)], device=dev)
            ppos = pos.expand(B).contiguous()
            for idle in (False, True):
                if idle and B < 2:
                    continue
                active = torch.tensor([int(b % 3 != 1) for b in range(B)], dtype=torch.int32, device=dev) if idle else None
                tag = f"B={B} p={p}" + (" idle rows" if idle else "")

                def batch(side, c, B=B, bpos=bpos, active=active, fp8=False):
                    ws = side.workspace(B, H, G, HS, n_splits) if n_splits > 1 else None
                    if fp8:
                        y = ops.attention_decode_batch_kv8(c["qkv"][:B], kv8(side), bpos, c["cos"], c["sin"], *a, ws,
                                                           active)
                        names = ("kc8", "vc8", "ks8", "vs8")
                    else:
                        y = ops.attention_decode_batch(c["qkv"][:B], side.t["k"], side.t["v"], bpos, c["cos"],
                                                       c["sin"], *a, ws, active)
                        names = ("k", "v")
                    bi = torch.arange(B, device=dev)
                    return [y] + [side.t[n][bi, :, bpos] for n in names]

                yield f"decode_batch {tag}", batch
                yield f"decode_batch_kv8 {tag}", (lambda side, c, f=batch: f(side, c, fp8=True))
                for P in sorted({0, 64, 130, p}):
                    pl = torch.tensor([P], device=dev)

                    def shared(side, c, B=B, ppos=ppos, pl=pl, active=active, p=p):
                        y = ops.attention_decode_shared(c["qkv"][:B], side.t["k"], side.t["v"], ppos[:1], pl, c["cos"],
                                                        c["sin"], *a, side.workspace(B, H, G, HS, n_splits)
                                                        if n_splits > 1 else None, active)
                        return [y] + rows_written(side, ("k", "v"), slice(0, B), p)

                    yield f"decode_shared {tag} P={P}", shared


def main():
    libs = os.environ["AB_LIBS"].split(",")
    if len(libs) != 2:
        sys.exit("AB_LIBS names two libraries")
    dev = torch.device("cuda")
    loaded = [ops.load_library(Path(p), strict=False) for p in libs]
    n_cases = 0
    for H, G in GEOMETRIES:
        gen = torch.Generator(device=dev).manual_seed(1000 * H + G)
        const, written = make_inputs(H, G, dev, gen)
        sides = [Side(lib, written) for lib in loaded]
        names, flags = [], []
        for n_splits in SPLITS:
            # the launch's own head slices, then (where that changes the kernel) all heads in one workgroup
            for hsplit in (None, 1) if H // G > 1 and n_splits > 1 else (None,):
                if hsplit is None:
                    os.environ.pop("LGA_ATTN_HSPLIT", None)
                else:
                    os.environ["LGA_ATTN_HSPLIT"] = str(hsplit)
                for name, run in cases(H, G, n_splits, dev):
                    outs = []
                    for side in sides:
                        ops._lib = side.lib
                        outs.append([t.clone(memory_format=torch.contiguous_format) for t in run(side, const)])
                    same = torch.stack([(x.view(torch.uint8) == y.view(torch.uint8)).all() if x.dtype != torch.uint8
                                        else (x == y).all() for x, y in zip(*outs)]).all()
                    flags.append(same)
                    names.append(f"H={H} G={G} splits={n_splits} hsplit={hsplit or 'auto'}: {name}")
        os.environ.pop("LGA_ATTN_HSPLIT", None)
        for k in written:  # nothing else was written either
            flags.append(torch.equal(sides[0].t[k].view(torch.uint8), sides[1].t[k].view(torch.uint8))
                         * torch.ones((), dtype=torch.bool, device=dev))
            names.append(f"H={H} G={G}: the whole {k} buffer after all cases")
        bad = (~torch.stack(flags)).nonzero().flatten().tolist()
        n_cases += len(flags)
        if bad:
            print(f"DIFFERENT BITS: {names[bad[0]]} ({len(bad)} of {len(flags)} cases of this geometry differ)", flush=True)
            sys.exit(1)
        print(f"H={H} G={G}: {len(flags)} cases, same bits", flush=True)
    print(f"{n_cases} cases, {Path(libs[0]).name} == {Path(libs[1]).name} bit for bit")


if __name__ == "__main__":
    main()
