"""Greedy speculative decoding on the MI355X: the window attention kernel (lga_attention_decode_window), the
acceptance kernel (lga_spec_accept), ``GPT.decode_window``, ``WindowDecodeGraph`` and ``generate_speculative``.

The promise under test: speculation never changes the result. The window launch leaves y and the caches with the
bits (``torch.equal``) of M successive one-row ``attention_decode_fused`` calls, row r of ``decode_window`` has the
bits of the one-row model step, and ``generate_speculative`` returns ``generate``'s tokens whatever the drafter says.
"""

import math

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
HS = 128
S = 96  # cache rows: ops.decode_splits gives 6 splits


@pytest.fixture(scope="module")
def ops():
    from lit_gpt import ops as _ops

    _ops.load_library()
    return _ops


_CACHE = {}


def _bf16(shape, name, std=1.0):
    key = ("v", shape, name, std)
    if key not in _CACHE:
        _CACHE[key] = torch.from_numpy(synth.normal(shape, name, 5, std)).to(DEV).to(torch.bfloat16)
    return _CACHE[key]


def _rope(rows):
    from lit_gpt.model import build_rope_cache

    if ("rope", rows) not in _CACHE:
        cos, sin = build_rope_cache(rows, HS, device=torch.device(DEV))
        _CACHE[("rope", rows)] = (cos.float().contiguous(), sin.float().contiguous())
    return _CACHE[("rope", rows)]


def _sequential(ops, qkv, kc, vc, p0, H, G, n_splits, max_seq):
    """The reference: M one-row fused launches on rows 0..M-1 at p0..p0+M-1 (rows at or past max_seq are not run)."""
    cos, sin = _rope(max_seq)
    ws = ops.AttentionWorkspace(1, H, G, HS, n_splits, DEV)
    ys = []
    for r in range(qkv.shape[0]):
        if p0 + r >= max_seq:
            ys.append(None)
            continue
        pos = torch.tensor([p0 + r], device=DEV)
        ys.append(ops.attention_decode_fused(qkv[r:r + 1].contiguous(), kc, vc, pos, pos, cos, sin, H, G, HS, HS,
                                             1.0 / math.sqrt(HS), n_splits, workspace=ws).clone())
    return ys


def _window(ops, qkv, kc, vc, pos0, H, G, n_splits, max_seq, ws=None):
    cos, sin = _rope(max_seq)
    ws = ws or ops.AttentionWorkspace(qkv.shape[0], H, G, HS, n_splits, DEV)
    return ops.attention_decode_window(qkv, kc, vc, pos0, cos, sin, H, G, HS, HS, 1.0 / math.sqrt(HS), n_splits,
                                       workspace=ws)


def _check_window(ops, H, G, M, p0, max_seq=S):
    n_splits = ops.decode_splits(G, H // G, HS, max_seq)
    k0 = _bf16((G, max_seq, HS), f"k{G}x{max_seq}")
    v0 = _bf16((G, max_seq, HS), f"v{G}x{max_seq}")
    qkv = _bf16((8, (H + 2 * G) * HS), f"qkv{G}")[:M].contiguous()
    kr, vr = k0.clone(), v0.clone()
    ref = _sequential(ops, qkv, kr, vr, p0, H, G, n_splits, max_seq)
    kw, vw = k0.clone(), v0.clone()
    y = _window(ops, qkv, kw, vw, torch.tensor([p0], device=DEV), H, G, n_splits, max_seq)
    assert y.shape == (M, H * HS)
    for r in range(M):
        if ref[r] is not None:
            assert torch.equal(y[r], ref[r][0]), (r, int((y[r] != ref[r][0]).sum()))
    assert torch.equal(kw, kr), int((kw != kr).sum())
    assert torch.equal(vw, vr), int((vw != vr).sum())
    return n_splits, (k0, v0, kw, vw)


GEOMS = [(8, 8), (8, 4), (8, 2), (8, 1)]  # q_per_kv 1, 2, 4, 8 (the last two take head slices at 6 splits)
ROWS = [1, 2, 3, 5, 8]


@pytest.mark.parametrize("H,G", GEOMS)
@pytest.mark.parametrize("M", ROWS)
def test_window_attention_bit_identical_to_sequential_launches(ops, H, G, M):
    # p0: an empty cache; p + 1 crosses a multiple of the 6 splits inside the window (41 -> 42; for M = 1 the row sits
    # on the multiple); no crossing for M <= 5 (43..47); the last row in the last cache row
    for p0 in (0, 40 if M > 1 else 41, 42, S - M):
        n_splits, _ = _check_window(ops, H, G, M, p0)
        assert n_splits == 6


def test_window_attention_long_cache_32_splits(ops):
    n_splits, _ = _check_window(ops, 8, 2, 8, 12270, max_seq=12288)
    assert n_splits == 32


def test_window_attention_rows_past_the_cache_store_nothing(ops):
    """p0 = 94, M = 4 on 96 rows: rows 94 and 95 match the sequential calls; rows 96 and 97 do not exist — an unmasked
    store would land in rows 0, 1 of the next group."""
    for H, G in ((8, 8), (8, 2)):
        _, (k0, v0, kw, vw) = _check_window(ops, H, G, 4, 94)
        assert torch.equal(kw[:, :94], k0[:, :94]) and torch.equal(vw[:, :94], v0[:, :94])
        assert not torch.equal(kw[:, 94:], k0[:, 94:])


def test_window_attention_graph_replay_with_advancing_position(ops):
    H, G, M = 8, 4, 3
    n_splits = ops.decode_splits(G, H // G, HS, S)
    qkv = _bf16((8, (H + 2 * G) * HS), f"qkv{G}")[:M].contiguous()
    kr, vr = _bf16((G, S, HS), f"k{G}x{S}").clone(), _bf16((G, S, HS), f"v{G}x{S}").clone()
    kw, vw = kr.clone(), vr.clone()
    pos0 = torch.tensor([10], device=DEV)
    ws = ops.AttentionWorkspace(M, H, G, HS, n_splits, DEV)
    y = torch.empty(M, H * HS, dtype=torch.bfloat16, device=DEV)
    cos, sin = _rope(S)

    def launch():
        ops.attention_decode_window(qkv, kw, vw, pos0, cos, sin, H, G, HS, HS, 1.0 / math.sqrt(HS), n_splits,
                                    workspace=ws, out=y)

    launch()  # warm-up at p0 = 10 (a real run: the reference runs it too)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for i, p in enumerate((10, 12, 16)):  # 16 + 1 .. 16 + 3 crosses 18 = 3 * 6
        ref = _sequential(ops, qkv, kr, vr, p, H, G, n_splits, S)
        if i:
            pos0.fill_(p)
            g.replay()
        for r in range(M):
            assert torch.equal(y[r], ref[r][0]), (p, r)
        assert torch.equal(kw, kr) and torch.equal(vw, vr)
    assert int(ws.counters.abs().sum()) == 0  # re-armed


def test_window_attention_argument_errors(ops):
    H, G = 8, 8
    kc, vc = _bf16((G, S, HS), f"k{G}x{S}").clone(), _bf16((G, S, HS), f"v{G}x{S}").clone()
    qkv = _bf16((9, (H + 2 * G) * HS), "qkv9")
    pos0 = torch.tensor([3], device=DEV)
    cos, sin = _rope(S)
    err = (ValueError, RuntimeError)
    for rows in (qkv[:0], qkv):  # M = 0, M = 9
        with pytest.raises(err):
            ops.attention_decode_window(rows, kc, vc, pos0, cos, sin, H, G, HS, HS, 0.1)
    with pytest.raises(err):  # head_size 64
        ops.attention_decode_window(_bf16((2, (H + 2 * G) * 64), "qkv64"), kc, vc, pos0, cos, sin, H, G, 64, 64, 0.1)
    with pytest.raises(err):  # splits without a workspace
        ops.attention_decode_window(qkv[:2].contiguous(), kc, vc, pos0, cos, sin, H, G, HS, HS, 0.1, n_splits=6)
    lib = ops.load_library()  # the C entry point checks the same before any launch
    p = qkv.data_ptr()
    f = lib.lga_attention_decode_window
    assert f(p, p, p, p, p, p, S, p, p, p, 0, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"[1, 8]" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, S, p, p, p, 9, H, G, HS, HS, S, 1, 0.1, None) != 0
    assert b"[1, 8]" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, S, p, p, p, 2, H, G, 64, 64, S, 1, 0.1, None) != 0
    assert b"head_size" in lib.lga_last_error_string()
    assert f(p, p, p, p, p, p, S, p, None, None, 2, H, G, HS, HS, S, 6, 0.1, None) != 0
    assert b"workspace" in lib.lga_last_error_string()
    assert torch.equal(kc, _bf16((G, S, HS), f"k{G}x{S}"))  # nothing was launched


# ------------------------------------------------------------------------------------------------ spec_accept
def _np_accept(logits: np.ndarray, window: np.ndarray):
    """NaN first, ties to the lowest index; the accepted prefix."""
    M = logits.shape[0]
    t = []
    for r in range(M):
        nan = np.isnan(logits[r])
        t.append(int(np.argmax(nan)) if nan.any() else int(np.argmax(logits[r])))
    a = 0
    while a < M - 1 and window[a + 1] == t[a]:
        a += 1
    return a, t


def _accept_case(ops, logits: torch.Tensor, window, pos=17):
    M = logits.shape[0]
    w = torch.tensor(window, dtype=torch.int32, device=DEV)
    tok = torch.tensor([-5], dtype=torch.int32, device=DEV)
    p = torch.tensor([pos], dtype=torch.int64, device=DEV)
    out = ops.spec_accept(logits, w, token_inout=tok, pos_inout=p).tolist()
    a, t = _np_accept(logits.float().cpu().numpy(), np.asarray(window))
    assert out[0] == a and out[1:a + 2] == t[:a + 1], (out, a, t)
    assert all(v == -1 for v in out[a + 2:])
    assert int(tok) == t[a] and int(p) == pos + a + 1
    return a, t


@pytest.mark.parametrize("n", [32000, 1003])  # 16-B rows (vector loads) and an odd row length (scalar loads)
def test_spec_accept_against_numpy(ops, n):
    M = 6
    logits = _bf16((8, 32000), "logits")[:M, :n].contiguous()
    t = [int(v) for v in torch.argmax(logits.float(), dim=-1)]
    a, _ = _accept_case(ops, logits, [7] + t[:M - 1])  # every draft right
    assert a == M - 1
    for i in range(M - 1):  # a wrong draft at each index (0: the first draft wrong)
        w = [7] + t[:M - 1]
        w[1 + i] = (w[1 + i] + 1) % n
        a, _ = _accept_case(ops, logits, w)
        assert a == i
    tied = logits.clone()  # a row with tied maxima: the lowest index wins
    tied[1, 900] = tied[1, 40] = tied[1, 333] = 200.0
    a, tt = _accept_case(ops, tied, [7, t[0], 40, t[2], t[3], t[4]])
    assert tt[1] == 40 and a == M - 1
    assert _accept_case(ops, tied, [7, t[0], 333, t[2], t[3], t[4]])[0] == 1
    nan = logits.clone()  # a row holding NaN: the first NaN wins
    nan[2, 555] = float("nan")
    nan[2, 77] = float("nan")
    a, tt = _accept_case(ops, nan, [7, t[0], t[1], 77, t[3], t[4]])
    assert tt[2] == 77 and a == M - 1
    a, tt = _accept_case(ops, logits[:1].contiguous(), [7])  # M = 1: a plain argmax step
    assert a == 0 and tt[0] == t[0]
    one = ops.argmax(logits[0].contiguous())
    assert int(one) == t[0]
    with pytest.raises((ValueError, RuntimeError)):
        ops.spec_accept(_bf16((9, 64), "l9"), torch.zeros(9, dtype=torch.int32, device=DEV))
    assert ops.load_library().lga_spec_accept(logits.data_ptr(), 0, n, logits.data_ptr(), logits.data_ptr(), None,
                                              None, None) != 0


def test_new_kernels_use_no_scratch():
    from lit_gpt import ops as _ops
    from test_native_library import _kernel_scratch

    scratch = _kernel_scratch(_ops.LIB_PATH)
    new = {k: v for k, v in scratch.items()
           if "window_append_kernel" in k or "spec_accept_kernel" in k
           or ("attn_kernel" in k and k.split("EEEv")[0].endswith("Lb1ELb1ELb1"))}  # <.., FUSED, PIPE, WINDOW>
    # window_append_kernel<KV8>: the bf16 and the fp8 instantiation of the one append kernel
    assert sum("window_append" in k for k in new) == 2 and sum("spec_accept" in k for k in new) == 2
    assert sum("attn_kernel" in k for k in new) == 5, sorted(new)
    assert all(v == (0, 0) for v in new.values()), new


# ------------------------------------------------------------------------------------------------ model
MODELS = [("int4-g128", 8), ("nf4", 8), ("int4-g128", 4)]  # (mode, n_query_groups), as tests/test_gpu_batch.py
NEW = 24


def _model(mode, groups, seed=1234, copy=0):
    from generate.base import build_model
    from lit_gpt import Config

    key = ("model", mode, groups, seed, copy)
    if key not in _CACHE:
        cfg = Config.from_name("Llama-2-7b-hf", n_layer=2, n_embd=1024, n_head=8, n_query_groups=groups,
                               intermediate_size=2816)
        _CACHE[key] = build_model(cfg, quantize=mode, device=torch.device(DEV), max_seq_length=S, seed=seed)
    return _CACHE[key]


def _prompt(vocab, T):
    return torch.from_numpy(synth.token_ids(T, vocab, seed=20 + T)).to(DEV)


def _fresh(model):
    model.set_kv_cache(batch_size=1, device=torch.device(DEV))


def _caches(model):
    return [(b.attn.kv_cache.k.clone(), b.attn.kv_cache.v.clone()) for b in model.transformer.h]


def _prefill(model, prompt):
    T = prompt.numel()
    return model(prompt.view(1, -1), torch.arange(T, device=DEV), last_token_only=True)


@pytest.mark.parametrize("mode,groups", MODELS)
def test_decode_window_rows_equal_one_row_steps(mode, groups):
    model = _model(mode, groups)
    MW = model.MAX_WINDOW
    toks = torch.from_numpy(synth.token_ids(MW, model.config.vocab_size, seed=3)).to(DEV).to(torch.int32)
    with torch.inference_mode():
        for T in (5, 33):
            prompt = _prompt(model.config.vocab_size, T)
            _fresh(model)
            _prefill(model, prompt)
            one, caches = [], []
            for r in range(MW):  # the reference, once per prompt: the same tokens, one row at a time
                one.append(model(toks[r].view(1, 1), torch.tensor([T + r], device=DEV)).view(-1).clone())
                caches.append(_caches(model))
            for M in sorted({2, 4, MW}):
                _fresh(model)
                _prefill(model, prompt)
                logits = model.decode_window(toks[:M], torch.tensor([T], device=DEV))
                assert logits.shape == (M, model.config.padded_vocab_size)
                for r in range(M):
                    assert torch.equal(logits[r], one[r]), (T, M, r)
                for (k, v), (kr, vr) in zip(_caches(model), caches[M - 1]):
                    assert torch.equal(k, kr) and torch.equal(v, vr), (T, M)
    _fresh(model)


def test_rejected_rows_leave_nothing_behind():
    """A window whose last rows are rejected, then a window from the earlier position: the logits of never having run
    the rejected rows (their stale K/V sits past every later row's position until overwritten)."""
    model = _model("int4-g128", 4)
    T = 33
    prompt = _prompt(model.config.vocab_size, T)
    a = torch.from_numpy(synth.token_ids(6, model.config.vocab_size, seed=4)).to(DEV).to(torch.int32)
    b = torch.from_numpy(synth.token_ids(5, model.config.vocab_size, seed=5)).to(DEV).to(torch.int32)
    with torch.inference_mode():
        _fresh(model)
        _prefill(model, prompt)
        model.decode_window(a[:2], torch.tensor([T], device=DEV))  # only rows 0, 1 ever run
        clean = model.decode_window(b, torch.tensor([T + 2], device=DEV)).clone()
        _fresh(model)
        _prefill(model, prompt)
        model.decode_window(a, torch.tensor([T], device=DEV))  # rows 2..5 are "rejected"
        again = model.decode_window(b, torch.tensor([T + 2], device=DEV))
        assert torch.equal(again, clean)
    _fresh(model)


def _reference(model, prompt, **kw):
    from generate.base import generate

    key = ("gen", id(model), prompt.numel(), tuple(sorted(kw.items())))
    if key not in _CACHE:
        _fresh(model)
        _CACHE[key] = generate(model, prompt, prompt.numel() + NEW, temperature=0.0, **kw).cpu()
    return _CACHE[key]


@pytest.mark.parametrize("mode,groups", MODELS)
@pytest.mark.parametrize("gamma", [1, 3, 7])
def test_generate_speculative_scripted_drafter_equals_generate(mode, groups, gamma):
    from generate.speculative import ScriptedDrafter, generate_speculative

    model = _model(mode, groups)
    V = model.config.vocab_size
    prompt = _prompt(V, 33)
    T = prompt.numel()
    ref = _reference(model, prompt)
    assert ref.numel() == T + NEW
    steps = NEW - 1  # decode steps after the prefill's token
    schedules = {"never": lambda rnd, i: False, "always": lambda rnd, i: True}
    for j in range(gamma):
        schedules[f"index{j}"] = (lambda j: lambda rnd, i: i == j)(j)
    for name, wrong in schedules.items():
        stats = {}
        _fresh(model)
        y = generate_speculative(model, prompt, T + NEW, ScriptedDrafter(ref.tolist(), wrong, V), speculate=gamma,
                                 stats=stats)
        assert torch.equal(y.cpu(), ref), (name, gamma)
        assert stats["tokens"] == steps
        if name == "never":
            assert stats["rounds"] == -(-steps // (gamma + 1)) and stats["accepted"] == stats["proposed"]
        if name == "always":
            assert stats["rounds"] == steps and stats["accepted"] == 0
    eos = int(ref[T + 1 + 9])  # from the middle of the output (the prefill's token is never tested)
    cut = _reference(model, prompt, eos_id=eos)
    assert cut.numel() < T + NEW and int(cut[-1]) == eos
    for wrong in (schedules["never"], schedules["index0"]):
        _fresh(model)
        y = generate_speculative(model, prompt, T + NEW, ScriptedDrafter(ref.tolist(), wrong, V), speculate=gamma,
                                 eos_id=eos)
        assert torch.equal(y.cpu(), cut), gamma
    _fresh(model)


def test_generate_speculative_graph_equals_eager():
    from generate.speculative import ScriptedDrafter, generate_speculative

    model = _model("int4-g128", 8)
    V = model.config.vocab_size
    prompt = _prompt(V, 5)
    ref = _reference(model, prompt)
    outs = []
    for use_graph in (True, False):
        _fresh(model)
        d = ScriptedDrafter(ref.tolist(), lambda rnd, i: (rnd + i) % 3 == 2, V)
        outs.append(generate_speculative(model, prompt, 5 + NEW, d, speculate=3, use_graph=use_graph).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], ref)
    _fresh(model)


@pytest.mark.parametrize("draft", ["same", "other-seed", "nf4-twin"])
def test_model_drafter_equals_generate(draft):
    from generate.speculative import ModelDrafter, generate_speculative

    model = _model("int4-g128", 8)
    dm = {"same": lambda: _model("int4-g128", 8, copy=1),  # a second instance: same config, seed and format
          "other-seed": lambda: _model("int4-g128", 8, seed=77),
          "nf4-twin": lambda: _model("nf4", 8)}[draft]()
    assert dm is not model
    prompt = _prompt(model.config.vocab_size, 33)
    ref = _reference(model, prompt)
    for gamma in (3, 7):
        stats = {}
        _fresh(model)
        y = generate_speculative(model, prompt, 33 + NEW, ModelDrafter(dm), speculate=gamma, stats=stats)
        assert torch.equal(y.cpu(), ref), (draft, gamma)
        print(f"{draft} gamma {gamma}: accepted {stats['accepted']} of {stats['proposed']} in {stats['rounds']} rounds")
        if draft == "same":  # every round fully accepted: each next round starts with the catch-up step
            assert stats["accepted"] == stats["proposed"] and stats["rounds"] == -(-(NEW - 1) // (gamma + 1))
    _fresh(model)
    _fresh(dm)


def test_ngram_drafter_on_repeated_prompt_equals_generate():
    from generate.speculative import NgramDrafter, generate_speculative

    model = _model("int4-g128", 4)
    block = _prompt(model.config.vocab_size, 9)
    prompt = block.repeat(4)
    ref = _reference(model, prompt)
    stats = {}
    _fresh(model)
    y = generate_speculative(model, prompt, prompt.numel() + NEW, NgramDrafter(3), speculate=3, stats=stats)
    assert torch.equal(y.cpu(), ref)
    assert stats["proposed"] > 0
    _fresh(model)


def test_speculative_refusals():
    from generate.base import build_model
    from generate.speculative import ModelDrafter, NgramDrafter, generate_speculative
    from lit_gpt import Config, lora

    dev = torch.device(DEV)
    model = _model("int4-g128", 8)
    prompt = _prompt(model.config.vocab_size, 5)
    with pytest.raises(NotImplementedError, match="greedy only"):
        generate_speculative(model, prompt, 12, NgramDrafter(), temperature=0.8)
    for gamma in (0, model.MAX_WINDOW):
        with pytest.raises(ValueError, match="speculate"):
            generate_speculative(model, prompt, 12, NgramDrafter(), speculate=gamma)
    tiny = dict(n_layer=1, n_embd=256, n_head=2, n_query_groups=2, intermediate_size=512, vocab_size=1000,
                padding_multiple=64, block_size=64)
    small = _prompt(1000, 5)
    bf16 = build_model(Config.from_name("Llama-2-7b-hf", **tiny), quantize=None, device=dev, max_seq_length=32)
    with pytest.raises(NotImplementedError, match="speculative"):
        generate_speculative(bf16, small, 12, NgramDrafter())
    lcfg = lora.Config.from_name("Llama-2-7b-hf", r=8, alpha=16, to_query=True, to_value=True, **tiny)
    adapted = build_model(lcfg, quantize="int4-g128", device=dev, max_seq_length=32)
    lora.attach(adapted, lora.random_adapter(lcfg), lcfg)
    with pytest.raises(NotImplementedError, match="speculative"):
        generate_speculative(adapted, small, 12, NgramDrafter())
    other = build_model(Config.from_name("Llama-2-7b-hf", **tiny), quantize="int4-g128", device=dev, max_seq_length=32)
    with pytest.raises(ValueError, match="vocabulary"):
        generate_speculative(model, prompt, 12, ModelDrafter(other))
    with pytest.raises(NotImplementedError, match="window"):
        model.decode_window(torch.zeros(model.MAX_WINDOW + 1, dtype=torch.int32, device=DEV),
                            torch.tensor([0], device=DEV))
