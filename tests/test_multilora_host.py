"""Several LoRA adapters per batch without a GPU: the stacked layout ``lit_gpt.lora.attach_many`` builds against
``build_layout`` per adapter, its refusals, the ``adapters`` argument checks of ``generate_batch`` /
``generate_continuous`` (they come before anything touches the device), the prompts-file parser and the refusals of
generate/lora.py's multi-adapter command line, and the argument validation of ``lga_lora_gemv_rows`` (it returns before
any launch)."""

import ctypes
import dataclasses
import types

import pytest
import torch


class _Recorder(torch.nn.Module):
    """Stands in for MultiLoraLinear on a meta model: attach_many's key mapping and layouts without the kernels."""

    def __init__(self, base, A, B, row_off, scaling, adapters):
        super().__init__()
        self.base, self.A, self.B, self.row_off, self.scaling, self.adapters = base, A, B, row_off, scaling, adapters


def _config(**kw):
    from lit_gpt import lora

    base = dict(n_layer=2, n_embd=64, n_head=4, n_query_groups=2, intermediate_size=128, vocab_size=250,
                padding_multiple=64, block_size=32, r=4, alpha=16, to_query=True, to_value=True)
    base.update(kw)
    return lora.Config.from_name("Llama-2-7b-hf", **base)


def _meta_model(cfg):
    from lit_gpt import GPT

    with torch.device("meta"):
        return GPT(cfg).to(torch.bfloat16)


@pytest.mark.parametrize("targets", ["q+v", "all"])
def test_attach_many_stacks_the_layout_build_layout_gives_each_adapter(monkeypatch, targets):
    from lit_gpt import lora

    monkeypatch.setattr(lora, "MultiLoraLinear", _Recorder)
    every = dict(to_key=True, to_projection=True, to_mlp=True, to_head=True, r=16)
    cfg = _config(**(every if targets == "all" else {}))
    model = _meta_model(cfg)
    states = [lora.random_adapter(cfg, seed=40 + i) for i in range(3)]
    aset = lora.attach_many(model, [states[0], {"model": states[1]}, states[2]], cfg)  # flat or nested, as attach
    assert aset is model.lora_adapters and aset.n == 3 and aset.selected is None
    assert aset.rows.dtype == torch.int32 and aset.rows.shape == (8,)
    adapted = {n: m for n, m in model.named_modules() if isinstance(m, _Recorder)}
    per_block = ["attn.attn"] if targets == "q+v" else ["attn.attn", "attn.proj", "mlp.fc_1", "mlp.fc_2", "mlp.proj"]
    want = {f"transformer.h.{i}.{n}" for i in range(cfg.n_layer) for n in per_block}
    want |= {"lm_head"} if cfg.to_head else set()
    assert set(adapted) == want
    rp = lora.padded_rank(cfg.r)
    for name, m in adapted.items():
        qkv = (cfg.n_head, cfg.n_query_groups, (cfg.to_query, cfg.to_key, cfg.to_value)) if name.endswith("attn.attn") else None
        assert isinstance(m.base, torch.nn.Linear) and m.scaling == cfg.alpha / cfg.r and m.adapters is aset
        assert m.A.shape[0] == m.B.shape[0] == 3 and m.B.shape[1:] == (m.base.out_features, rp)
        for i, st in enumerate(states):
            A, B, off = lora.build_layout(st[f"{name}.lora_A"], st[f"{name}.lora_B"], cfg.r, m.base.out_features, qkv)
            assert torch.equal(m.A[i], A) and torch.equal(m.B[i], B), (name, i)
            assert (off is None and m.row_off is None) or torch.equal(m.row_off, off)
    assert not torch.equal(adapted["transformer.h.0.attn.attn"].B[0], adapted["transformer.h.0.attn.attn"].B[1])


def test_attach_many_refusals_leave_the_model_as_it_was(monkeypatch):
    from lit_gpt import lora

    monkeypatch.setattr(lora, "MultiLoraLinear", _Recorder)
    cfg = _config()
    model = _meta_model(cfg)
    good = [lora.random_adapter(cfg, seed=i) for i in range(2)]
    other_rank = lora.random_adapter(dataclasses.replace(cfg, r=8), seed=3)
    with pytest.raises(ValueError, match="do not match"):  # an adapter of another rank in the set
        lora.attach_many(model, [good[0], other_rank], cfg)
    surplus = dict(good[1], **{"lm_head.lora_A": torch.zeros(4, 64), "lm_head.lora_B": torch.zeros(256, 4)})
    with pytest.raises(KeyError, match="not targeted"):  # an adapter of other targets in the set
        lora.attach_many(model, [good[0], surplus], cfg)
    missing = {k: v for k, v in good[1].items() if k != "transformer.h.1.attn.attn.lora_B"}
    with pytest.raises(KeyError, match="missing"):
        lora.attach_many(model, [missing], cfg)
    with pytest.raises(ValueError, match="no adapters"):
        lora.attach_many(model, [], cfg)
    assert not any(isinstance(m, _Recorder) for m in model.modules()) and not hasattr(model, "lora_adapters")
    lora.attach_many(model, good, cfg)
    with pytest.raises(RuntimeError, match="already carries"):
        lora.attach_many(model, good, cfg)


def test_attach_and_attach_many_refuse_a_model_the_other_has_adapted(monkeypatch):
    from lit_gpt import lora

    class One(lora.LoraLinear):
        def __init__(self, base, *a):
            torch.nn.Module.__init__(self)
            self.base = base

    class Many(lora.MultiLoraLinear):
        def __init__(self, base, *a):
            torch.nn.Module.__init__(self)
            self.base = base

    monkeypatch.setattr(lora, "LoraLinear", One)
    monkeypatch.setattr(lora, "MultiLoraLinear", Many)
    cfg = _config()
    states = [lora.random_adapter(cfg, seed=i) for i in range(2)]
    model = _meta_model(cfg)
    lora.attach(model, states[0], cfg)
    with pytest.raises(RuntimeError, match="already carries"):
        lora.attach_many(model, states, cfg)
    model = _meta_model(cfg)
    lora.attach_many(model, states, cfg)
    with pytest.raises(RuntimeError, match="already carries"):
        lora.attach(model, states[0], cfg)


def test_adapter_set_select_and_assign():
    from lit_gpt import lora, ops

    aset = lora.AdapterSet(3, "cpu")
    assert aset.n == 3 and aset.rows.tolist() == [-1] * ops.MAX_GEMV_ROWS
    aset.assign(2, 1)
    aset.assign(0, 2)
    aset.assign(2, None)
    assert aset.rows.tolist() == [2, -1, -1, -1, -1, -1, -1, -1]
    assert aset.select(2) is aset and aset.selected == 2 and aset.select(None).selected is None
    for bad in (3, -1, 1.0, True, "0"):
        with pytest.raises(ValueError, match="index into the set's 3 adapters"):
            aset.select(bad)
        with pytest.raises(ValueError, match="index into the set's 3 adapters"):
            aset.assign(0, bad)
    with pytest.raises(ValueError, match="row 8"):
        aset.assign(8, 0)
    assert aset.selected is None and aset.rows.tolist()[0] == 2


class _Untouchable:
    """A model of which nothing but ``lora_adapters`` may be read: the refusal came before any other use of it."""

    def __init__(self, aset=None):
        if aset is not None:
            self.lora_adapters = aset

    def __getattr__(self, name):
        if name == "lora_adapters":
            raise AttributeError(name)
        raise AssertionError(f"model.{name} was used before the adapters were checked")


@pytest.mark.parametrize("fn", ["generate_batch", "generate_continuous"])
def test_generate_refuses_bad_adapters_before_anything_else(fn):
    import generate.base as gb
    from lit_gpt import lora

    run = getattr(gb, fn)
    prompts = [torch.arange(4, dtype=torch.int32), torch.arange(6, dtype=torch.int32), torch.arange(3, dtype=torch.int32)]
    with pytest.raises(ValueError, match="no adapter set"):
        run(_Untouchable(), prompts, 4, temperature=0.0, adapters=[0, None, 1])
    model = _Untouchable(lora.AdapterSet(2, "cpu"))
    with pytest.raises(ValueError, match="2 adapters for 3 prompts"):
        run(model, prompts, 4, temperature=0.0, adapters=[0, None])
    for bad in ([0, 2, 1], [0, -1, 1], [0, "1", None]):
        with pytest.raises(ValueError, match="index into the set's 2 adapters"):
            run(model, prompts, 4, temperature=0.0, adapters=bad)
    assert model.lora_adapters.selected is None and model.lora_adapters.rows.tolist() == [-1] * 8


def test_runtime_executors_refuse_adapters_without_a_set():
    from lit_gpt import runtime

    model = types.SimpleNamespace()
    with pytest.raises(ValueError, match="no adapter set"):
        runtime._assign_adapters(model, [0, 1], 2)
    runtime._assign_adapters(model, None, 2)
    ex = runtime.SlotDecodeGraph.__new__(runtime.SlotDecodeGraph)
    ex.model = model
    with pytest.raises(ValueError, match="no adapter set"):
        ex.fill(0, torch.zeros(1, dtype=torch.int32), 3, adapter=1)


def test_prompts_file_parsing():
    import generate.lora as gl

    text = "0\tWhat do llamas eat?\n-\tName a colour.\n\n2\tTabs\tinside stay\n"
    assert gl.parse_requests(text, 3) == [(0, "What do llamas eat?"), (None, "Name a colour."),
                                          (2, "Tabs\tinside stay")]
    assert gl.parse_requests("1\t12\n-\t5\n", 2, synthetic=True) == [(1, 12), (None, 5)]
    with pytest.raises(ValueError, match="line 2: INDEX '3'"):
        gl.parse_requests("0\ta\n3\tb\n", 3)
    with pytest.raises(ValueError, match="line 1: INDEX '-1'"):
        gl.parse_requests("-1\ta\n", 3)
    with pytest.raises(ValueError, match="line 1: INDEX 'x'"):
        gl.parse_requests("x\ta\n", 3)
    with pytest.raises(ValueError, match="line 2: expected INDEX<TAB>instruction"):
        gl.parse_requests("0\ta\n1 no tab here\n", 3)
    with pytest.raises(ValueError, match="prompt length 'twelve'"):
        gl.parse_requests("0\ttwelve\n", 3, synthetic=True)
    with pytest.raises(ValueError, match="prompt length '0'"):
        gl.parse_requests("0\t0\n", 3, synthetic=True)
    with pytest.raises(ValueError, match="no requests"):
        gl.parse_requests("\n\n", 3)


def test_multi_adapter_cli_refuses_before_building_the_model(monkeypatch, tmp_path):
    import generate.lora as gl

    def boom(*a, **kw):
        raise AssertionError("the model was built before the refusal")

    monkeypatch.setattr(gl, "build_model", boom)
    f = tmp_path / "requests.txt"
    f.write_text("0\t8\n-\t5\n1\t12\n")
    paths = [str(tmp_path / "a0.pth"), str(tmp_path / "a1.pth")]
    common = ["--synthetic", "Llama-2-7b-hf", "--checkpoint_dir", str(tmp_path), "--prompts_file", str(f),
              "--lora_paths", *paths]
    with pytest.raises(NotImplementedError, match="--merge with --lora_paths"):
        gl._cli(common + ["--quantize", "int4-g128", "--merge"])
    with pytest.raises(NotImplementedError, match="bf16 base"):
        gl._cli(common)
    with pytest.raises(NotImplementedError, match="4-bit weights only"):
        gl._cli(common + ["--quantize", "bnb.int8"])
    with pytest.raises(NotImplementedError, match="bf16-true"):
        gl._cli(common + ["--quantize", "nf4", "--precision", "32-true"])
    with pytest.raises(NotImplementedError, match="--batch_size 5"):
        gl._cli(common + ["--quantize", "nf4", "--batch_size", "5"])
    f.write_text("0\t8\n2\t5\n")
    with pytest.raises(ValueError, match="line 2: INDEX '2'"):
        gl._cli(common + ["--quantize", "int4-g128"])
    f.write_text("0\t8\n")
    monkeypatch.setattr(gl, "lora_mlp", True)
    with pytest.raises(NotImplementedError, match="sparse-MoE"):  # what check_supported refuses
        gl._cli(["--synthetic", "Mixtral-8x7B-v0.1", "--checkpoint_dir", str(tmp_path), "--prompts_file", str(f),
                 "--lora_paths", *paths, "--quantize", "nf4"])
    with pytest.raises(SystemExit):  # one without the other
        gl._cli(["--synthetic", "Llama-2-7b-hf", "--lora_paths", *paths])


def test_lora_gemv_rows_signature_and_argument_validation():
    """The entry point is bound, and rejects bad arguments before any launch (no GPU needed)."""
    from lit_gpt import ops

    assert "lga_lora_gemv_rows" in ops.SIGNATURES
    lib = ops.load_library()
    p = ctypes.c_void_p(4096)
    N, K, R, r, n = 64, 64, 16, 8, 3

    def call(x=p, A=p, B=p, adapter=p, base=p, y=p, n_adapters=n, a_stride=R * K, b_stride=N * r, M=2, K=K, R=R, r=r):
        return lib.lga_lora_gemv_rows(x, None, 1e-5, A, B, None, adapter, n_adapters, a_stride, b_stride, 2.0, base,
                                      None, y, M, N, K, R, r, None)

    for null in ("x", "A", "B", "adapter", "base", "y"):
        assert call(**{null: None}) != 0, null
        assert b"null" in lib.lga_last_error_string()
    for M in (0, 9, -1):
        assert call(M=M) != 0
        assert b"1..8" in lib.lga_last_error_string()
    assert call(n_adapters=0) != 0
    assert b"n_adapters" in lib.lga_last_error_string()
    assert call(a_stride=R * K - 8) != 0  # strides below one block
    assert b"stride" in lib.lga_last_error_string()
    assert call(b_stride=N * r - 8) != 0
    assert b"stride" in lib.lga_last_error_string()
    assert call(a_stride=R * K + 4) != 0  # a stride that would break the 16-byte alignment of the blocks
    assert call(R=72, r=72, a_stride=72 * K, b_stride=N * 72) != 0  # r > 64
    assert b"r <= 64" in lib.lga_last_error_string()
    assert call(r=4) != 0 and call(R=200, a_stride=200 * K) != 0
    assert call(K=100, a_stride=R * 100) != 0
    assert b"multiple of 8" in lib.lga_last_error_string()
    # the Python wrapper's own checks
    A, B = torch.zeros(3, 16, 64), torch.zeros(3, 32, 8)
    ids = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="stacked"):
        ops.lora_gemv_rows(torch.zeros(2, 64), A[0], B[0], None, ids, 2.0, base=torch.zeros(2, 32))
    with pytest.raises(ValueError, match="needs row_off"):
        ops.lora_gemv_rows(torch.zeros(2, 64), A, B, None, ids, 2.0, base=torch.zeros(2, 32))
    off = torch.zeros(32, dtype=torch.int32)
    with pytest.raises(ValueError, match="1 <= M <= 8"):
        ops.lora_gemv_rows(torch.zeros(9, 64), A, B, off, ids, 2.0, base=torch.zeros(9, 32))
    with pytest.raises(ValueError, match="3 ids for 2 rows"):
        ops.lora_gemv_rows(torch.zeros(2, 64), A, B, off, torch.zeros(3, dtype=torch.int32), 2.0,
                           base=torch.zeros(2, 32))
    with pytest.raises(ValueError, match="base is required"):
        ops.lora_gemv_rows(torch.zeros(2, 64), A, B, off, ids, 2.0, base=None)
    with pytest.raises(ValueError, match="residual holds"):
        ops.lora_gemv_rows(torch.zeros(2, 64), A, B, off, ids, 2.0, base=torch.zeros(2, 32), residual=torch.zeros(32))
