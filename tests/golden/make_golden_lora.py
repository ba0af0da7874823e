"""Generate the LoRA fixture by running the REFERENCE's lit_gpt/lora.py on the CPU.

Run once, where the reference sources are (make_golden.py REF; they are not part of this repository):
    python tests/golden/make_golden_lora.py
Writes ``g6_lora.npz`` next to this script: for two tiny Llama-family models with a LoRA adapter, in fp32, the adapter
tensors under the reference's key names, the reference's ``lora_ind`` of every fused qkv Linear, a 12-token prompt,
the reference's UNMERGED logits over the prompt and its logits after ``merge_lora_weights``. The base weights are
``oracle.synth.state_dict(cfg, seed)`` (counter-based, regenerable anywhere; 8 MB per model as fp32, far over what a
committed file may hold), so the fixture carries the seed instead; the two configs are ``tests/lora_spec.py`` MODELS.

``lora_B`` is drawn with std 0.05: the reference initialises it to zero (lora.py:136), which would test nothing.
``lora_A`` keeps the reference's own initialisation (kaiming-uniform under a fixed torch seed).

  (a) ``mha``: n_embd 256, 4 heads, 2 layers, r 8, query + value only (the reference's generate/lora.py defaults);
  (b) ``gqa``: 4 heads in 2 query groups, r 4, every target on but ``to_key`` (r 4 exercises the rank padding).
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from make_golden import import_reference  # noqa: E402  (puts the repository root on sys.path)

sys.path.insert(0, str(HERE.parent))

from lora_spec import B_STD, MODELS, PROMPT, SEED  # noqa: E402


def import_reference_lora():
    """The reference's lit_gpt.lora next to make_golden's import of its model code; its one missing import,
    lit_gpt.utils.map_old_state_dict_weights (renames ``attn.weight`` to ``attn.linear.weight`` on load), is supplied
    by loading the base weights under the LoRA model's own names instead, so the stub only has to exist."""
    config, model, gbase, gtp = import_reference()
    sys.modules["lit_gpt.utils"].map_old_state_dict_weights = lambda state_dict, mapping, prefix: state_dict
    import lit_gpt.lora as lora

    return lora


def lora_names(sd, lora_model):
    """The base state dict under the names of the reference's LoRA model (``X.weight`` -> ``X.linear.weight`` for
    every LoRALinear)."""
    wrapped = {n for n, m in lora_model.named_modules() if hasattr(m, "linear")}
    out = {}
    for k, v in sd.items():
        mod, _, attr = k.rpartition(".")
        out[f"{mod}.linear.{attr}" if mod in wrapped else k] = torch.from_numpy(v)
    return out


@torch.inference_mode()
def main():
    from oracle import synth

    lora = import_reference_lora()
    out = {}
    for key, spec in MODELS.items():
        kw = dict(spec["base"])
        cfg = lora.Config.from_name(kw.pop("name"), **kw, **spec["lora"])
        sd = synth.state_dict(cfg, seed=SEED)
        torch.manual_seed(SEED)
        m = lora.GPT(cfg)  # lora_A: the reference's kaiming-uniform init under this seed
        state = lora_names(sd, m)
        for name, p in m.named_parameters():
            if name.endswith("lora_A"):
                state[name] = p.detach().clone()
            elif name.endswith("lora_B"):
                state[name] = torch.from_numpy(synth.normal(tuple(p.shape), name, SEED, B_STD))
        m.load_state_dict(state, strict=True)
        m.eval()
        prompt = torch.from_numpy(synth.token_ids(PROMPT, cfg.vocab_size, seed=SEED))
        unmerged = m(prompt.view(1, -1).long())[0].float()
        zero = lora.GPT(cfg)
        zero.load_state_dict({k: (torch.zeros_like(v) if k.endswith("lora_B") else v) for k, v in state.items()})
        plain = zero.eval()(prompt.view(1, -1).long())[0].float()
        lora.merge_lora_weights(m)
        merged = m(prompt.view(1, -1).long())[0].float()
        for name, v in state.items():
            if "lora_" in name:
                out[f"{key}/{name}"] = v.numpy()
        for i, blk in enumerate(m.transformer.h):
            out[f"{key}/transformer.h.{i}.attn.attn.lora_ind"] = np.asarray(blk.attn.attn.lora_ind, dtype=np.int64)
        out[f"{key}/prompt"] = prompt.numpy()
        out[f"{key}/logits_unmerged"] = unmerged.numpy()
        out[f"{key}/logits_merged"] = merged.numpy()
        out[f"{key}/logits_no_adapter"] = plain.numpy()
        moved = int((unmerged.argmax(-1) != plain.argmax(-1)).sum())
        scale = float(unmerged.abs().max())
        print(f"{key}: merged vs unmerged {float((merged - unmerged).abs().max()) / scale:.2e} of the logit scale; "
              f"argmax moved at {moved} of {PROMPT} positions against B = 0")
    out["seed"] = np.asarray(SEED)
    np.savez_compressed(HERE / "g6_lora.npz", **out)
    print("wrote", HERE / "g6_lora.npz")


if __name__ == "__main__":
    main()
