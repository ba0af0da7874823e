"""Generate the LLaMA-Adapter fixture by running the REFERENCE's lit_gpt/adapter.py on the CPU.

Run once, where the reference sources are (make_golden.py REF; they are not part of this repository):
    python tests/golden/make_golden_adapter.py
Writes ``g7_adapter.npz`` next to this script: for two tiny Llama-family models with a v1 adapter, in fp32, the adapter
tensors under the reference's key names, a 12-token prompt, the reference's logits over the prompt with the adapter and
its logits with every gating factor set to zero. The base weights are ``oracle.synth.state_dict(cfg, seed)``
(regenerable anywhere), so the fixture carries the seed instead; the two configs are ``tests/adapter_spec.py`` MODELS
(3 layers, ``adapter_start_layer`` 1: one block without and two with the adapter).

``adapter_wte`` keeps the reference's own initialisation under ``torch.manual_seed(SEED)``. ``gating_factor`` is drawn
with std 0.5: the reference initialises it to zero, which would test nothing. The script asserts that the adapter
moves the reference's argmax at ``MIN_MOVED`` or more of the 12 positions in each model.
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

from adapter_spec import GATING_STD, MIN_MOVED, MODELS, PROMPT, SEED  # noqa: E402


@torch.inference_mode()
def main():
    from oracle import synth

    import_reference()
    import lit_gpt.adapter as adapter  # the reference's

    out = {}
    for key, spec in MODELS.items():
        kw = dict(spec["base"])
        cfg = adapter.Config.from_name(kw.pop("name"), **kw, **spec["adapter"])
        state = {k: torch.from_numpy(v) for k, v in synth.state_dict(cfg, seed=SEED).items()}
        torch.manual_seed(SEED)
        m = adapter.GPT(cfg)  # adapter_wte: the reference's init under this seed
        for name, p in m.named_parameters():
            if "adapter_wte" in name:
                state[name] = p.detach().clone()
            elif "gating_factor" in name:
                state[name] = torch.randn_like(p) * GATING_STD
        m.load_state_dict(state, strict=True)
        m.eval()
        prompt = torch.from_numpy(synth.token_ids(PROMPT, cfg.vocab_size, seed=SEED))
        with_adapter = m(prompt.view(1, -1).long())[0].float()
        zero = adapter.GPT(cfg)
        zero.load_state_dict({k: (torch.zeros_like(v) if "gating_factor" in k else v) for k, v in state.items()})
        plain = zero.eval()(prompt.view(1, -1).long())[0].float()
        for name, v in state.items():
            if "adapter_wte" in name or "gating_factor" in name:
                out[f"{key}/{name}"] = v.numpy()
        out[f"{key}/prompt"] = prompt.numpy()
        out[f"{key}/logits_adapter"] = with_adapter.numpy()
        out[f"{key}/logits_zero_gating"] = plain.numpy()
        moved = int((with_adapter.argmax(-1) != plain.argmax(-1)).sum())
        rel = float((with_adapter - plain).abs().max() / with_adapter.abs().max())
        print(f"{key}: argmax moved at {moved} of {PROMPT} positions against zero gating; logits shift by {rel:.1%} of "
              "their scale")
        assert moved >= MIN_MOVED, f"{key}: the adapter moves only {moved} positions"
    out["seed"] = np.asarray(SEED)
    np.savez_compressed(HERE / "g7_adapter.npz", **out)
    print("wrote", HERE / "g7_adapter.npz")


if __name__ == "__main__":
    main()
