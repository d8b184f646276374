"""Writes tests/golden/g7_clip_text.npz: transformers' own CLIP text features on hash-initialised weights.

    python tests/golden/make_clip_golden.py

transformers.CLIPModel(CLIPConfig()) -- the default config is ViT-B/32's text tower and needs no files --
gets its text-side weights by name from tests/clip_ref.py (hashinit values, q / k gains that make the
attention peaked).  Recorded for the 4 prompts of clip_ref.prompts(30): ids, masks, get_text_features in
fp32, the same under torch.autocast("cpu", dtype=torch.bfloat16), and the relative L2 error between the
two (the yardstick of the bf16 GPU test: 3 x the reference's own bf16 error).  No weights are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_ref  # noqa: E402


def hf_model():
    from transformers import CLIPConfig, CLIPModel
    model = CLIPModel(CLIPConfig()).eval()
    sd = model.state_dict()
    names = {k: tuple(v.shape) for k, v in sd.items()
             if (k.startswith("text_model.") or k.startswith("text_projection.")) and v.is_floating_point()}
    with torch.no_grad():
        for k, v in clip_ref.hash_state(names).items():
            sd[k].copy_(v)
    return model, names


def features(model, ids, mask):
    out = model.get_text_features(input_ids=ids, attention_mask=mask)
    return out if torch.is_tensor(out) else out.pooler_output


def main():
    torch.manual_seed(0)
    model, _ = hf_model()
    ids, mask = clip_ref.prompts(30)
    with torch.no_grad():
        f32 = features(model, ids, mask).float()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            b16 = features(model, ids, mask).float()
    err = clip_ref.rel_l2(b16, f32)
    print(f"features {tuple(f32.shape)}  |f32| {float(f32.norm()):.4f}  bf16-autocast rel L2 {err:.3e}")
    np.savez_compressed(clip_ref.GOLDEN, ids=ids.numpy(), mask=mask.numpy(), features_f32=f32.numpy(),
                        features_bf16=b16.numpy(), bf16_rel_l2=np.float64(err))


if __name__ == "__main__":
    main()
