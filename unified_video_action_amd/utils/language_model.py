"""CLIP text tower on libuva_hip.so (reference: utils/language_model.py:7-33, which loads
transformers' CLIPModel and calls get_text_features inside the step -- policy:241-252 at inference,
policy:366-378 in compute_loss).

The network is fixed: CLIP ViT-B/32's text side (transformers CLIPTextTransformer): token + position
embedding, 12 pre-LN layers of width 512 (8 heads of 64, causal attention with the tokenizer's key mask,
QuickGELU MLP of width 2048), final LayerNorm, the row at the EOT token (the first maximum of the ids),
a bias-free [512, 512] projection.  `ClipTextTower` keeps the parameter names of CLIPModel's text side,
so a CLIPModel checkpoint's `text_model.*` / `text_projection.weight` entries load by name.

Kernels: uva_clip_embed, uva_clip_attn, uva_quick_gelu, uva_clip_pool (csrc/text_tower.hip) with
uva_layernorm_fwd and uva_gemm for the LayerNorms and Linears -- bf16 operands with an fp32 residual
stream as the timm Block (model/autoregressive/functional.py BlockFn), exact-f32 products under fp32
precision.  The tower is frozen: eval only, forward under no_grad, no parameter requires a gradient.
There is no torch fallback: without a GPU the forward raises.
"""
import os

import torch
import torch.nn as nn

from ..native import ops
from ..runtime import cdt

F32 = torch.float32
MAX_LENGTH = 30  # language_model.py:20


def _group(**children):
    m = nn.Module()
    for k, v in children.items():
        setattr(m, k, v)
    return m


def _invalidate(module, *args):
    module._operands = None


class ClipTextTower(nn.Module):
    """forward(input_ids [B, L], attention_mask [B, L]) -> [B, projection_dim] fp32, the value of
    CLIPModel.get_text_features (its pooler_output in transformers 5)."""

    def __init__(self, vocab_size=49408, hidden_size=512, intermediate_size=2048, num_hidden_layers=12,
                 num_attention_heads=8, max_position_embeddings=77, projection_dim=512, layer_norm_eps=1e-5):
        super().__init__()
        D = hidden_size
        if D != num_attention_heads * 64:
            raise ValueError(f"ClipTextTower: head_dim must be 64, got {D} / {num_attention_heads}")
        self.heads = num_attention_heads
        self.eps = layer_norm_eps
        layers = nn.ModuleList(
            _group(layer_norm1=nn.LayerNorm(D, eps=layer_norm_eps),
                   self_attn=_group(q_proj=nn.Linear(D, D), k_proj=nn.Linear(D, D), v_proj=nn.Linear(D, D),
                                    out_proj=nn.Linear(D, D)),
                   layer_norm2=nn.LayerNorm(D, eps=layer_norm_eps),
                   mlp=_group(fc1=nn.Linear(D, intermediate_size), fc2=nn.Linear(intermediate_size, D)))
            for _ in range(num_hidden_layers))
        self.text_model = _group(
            embeddings=_group(token_embedding=nn.Embedding(vocab_size, D),
                              position_embedding=nn.Embedding(max_position_embeddings, D)),
            encoder=_group(layers=layers), final_layer_norm=nn.LayerNorm(D, eps=layer_norm_eps))
        self.text_projection = nn.Linear(D, projection_dim, bias=False)
        for p in self.parameters():
            p.requires_grad = False
        self._operands = None
        self.register_load_state_dict_post_hook(_invalidate)
        super().train(False)

    def train(self, mode=True):
        return super().train(False)  # frozen: eval only

    def _apply(self, fn, *args, **kwargs):
        self._operands = None
        return super()._apply(fn, *args, **kwargs)

    def operands(self):
        """the GEMM operands in the compute dtype, made once (q / k / v concatenated into one [3D, D]
        weight and one [3D] bias) and reused by every step; rebuilt after a load, a move or a precision
        change."""
        c = cdt()
        dev = self.text_projection.weight.device
        if self._operands is not None and self._operands[0] == (c, dev):
            return self._operands[1]

        def w(t):
            return t.detach().to(c).contiguous()

        per_layer = []
        for lay in self.text_model.encoder.layers:
            a = lay.self_attn
            per_layer.append(dict(
                qkv_w=w(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight])),
                qkv_b=torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]).detach().float().contiguous(),
                out_w=w(a.out_proj.weight), fc1_w=w(lay.mlp.fc1.weight), fc2_w=w(lay.mlp.fc2.weight)))
        ops_ = dict(layers=per_layer, proj_w=w(self.text_projection.weight))
        self._operands = ((c, dev), ops_)
        return ops_

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None):
        tm = self.text_model
        tok, pos = tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight
        dev = tok.device
        if dev.type != "cuda":
            raise RuntimeError("ClipTextTower runs on libuva_hip.so kernels: move it to the GPU (no CPU fallback)")
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"input_ids must be an int64 / int32 [B, L] tensor, got {input_ids.dtype} "
                             f"{tuple(input_ids.shape)}")
        B, L = input_ids.shape
        if not 1 <= L <= min(ops.CLIP_MAX_L, pos.shape[0]):
            raise ValueError(f"sequence length {L} outside 1..{min(ops.CLIP_MAX_L, pos.shape[0])}")
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, L) or attention_mask.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"attention_mask must be an integer [B, L] tensor, got {attention_mask.dtype} "
                                 f"{tuple(attention_mask.shape)}")
            ops.clip_check_mask(attention_mask)
            attention_mask = attention_mask.to(dev).contiguous()
        ids = input_ids.to(dev).contiguous()
        c = cdt()
        D, H, M = tok.shape[1], self.heads, B * L
        op = self.operands()

        def empty(rows, cols, dtype):
            return torch.empty(rows, cols, dtype=dtype, device=dev)

        x = empty(M, D, F32)
        ops.clip_embed(ids, tok, pos, x)
        h, qkv, o = empty(M, D, c), empty(M, 3 * D, c), empty(M, D, c)
        Dh = tm.encoder.layers[0].mlp.fc1.weight.shape[0]
        a, g = empty(M, Dh, c), empty(M, Dh, c)
        x1 = empty(M, D, F32)
        mean, rstd = torch.empty(M, dtype=F32, device=dev), torch.empty(M, dtype=F32, device=dev)
        for lay, w in zip(tm.encoder.layers, op["layers"]):
            ops.layernorm_fwd(x, lay.layer_norm1.weight, lay.layer_norm1.bias, h, mean, rstd, self.eps)
            ops.linear(h, w["qkv_w"], qkv, bias=w["qkv_b"])
            ops.clip_attn(qkv, attention_mask, o, B, L, H)
            ops.linear(o, w["out_w"], x1, bias=lay.self_attn.out_proj.bias, residual=x)
            ops.layernorm_fwd(x1, lay.layer_norm2.weight, lay.layer_norm2.bias, h, mean, rstd, self.eps)
            ops.linear(h, w["fc1_w"], a, bias=lay.mlp.fc1.bias)
            ops.quick_gelu(a, g)
            ops.linear(g, w["fc2_w"], x, bias=lay.mlp.fc2.bias, residual=x1)
        # EOT pooling first: the final LayerNorm is per row, so it runs on the B gathered rows only
        pooled = empty(B, D, F32)
        ops.clip_pool(ids, x, pooled)
        hp = empty(B, D, c)
        ops.layernorm_fwd(pooled, tm.final_layer_norm.weight, tm.final_layer_norm.bias, hp, mean[:B].contiguous(),
                          rstd[:B].contiguous(), self.eps)
        out = empty(B, op["proj_w"].shape[0], F32)
        ops.linear(hp, op["proj_w"], out)
        return out

    def get_text_features(self, input_ids, attention_mask=None, **_):
        """CLIPModel's name for the same call (language_model.py:28)"""
        return self(input_ids, attention_mask)


def _load_clip_state(model_path):
    """the text-side tensors of a local HF CLIP directory, read without executing code from it:
    model.safetensors when the safetensors package imports, else pytorch_model.bin through
    torch.load(weights_only=True)."""
    st = os.path.join(model_path, "model.safetensors")
    pt = os.path.join(model_path, "pytorch_model.bin")
    sd = None
    if os.path.exists(st):
        try:
            from safetensors.torch import load_file
        except ImportError:
            load_file = None
        if load_file is not None:
            sd = load_file(st, device="cpu")
    if sd is None:
        if not os.path.exists(pt):
            raise FileNotFoundError(f"{model_path}: no model.safetensors readable (safetensors package needed) "
                                    "and no pytorch_model.bin")
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    return {k: v for k, v in sd.items() if k.startswith("text_model.") or k.startswith("text_projection.")}


_DIM_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
             "max_position_embeddings", "layer_norm_eps")


def _tower_dims(model_path):
    """the tower's sizes from the directory's config.json (text_config + projection_dim; settings only),
    ViT-B/32's where the file or a key is absent"""
    import json
    cfg_path = os.path.join(model_path, "config.json")
    if not os.path.exists(cfg_path):
        return {}
    with open(cfg_path) as f:
        cfg = json.load(f)
    text = cfg.get("text_config") or {}
    dims = {k: text[k] for k in _DIM_KEYS if text.get(k) is not None}
    if text.get("hidden_act", "quick_gelu") != "quick_gelu":
        raise NotImplementedError(f"{cfg_path}: text hidden_act {text['hidden_act']!r} (the tower runs QuickGELU)")
    if cfg.get("projection_dim") is not None:
        dims["projection_dim"] = cfg["projection_dim"]
    return dims


def get_text_model(task_name, language_emb_model, model_path=None):
    """language_model.py:7-22 -> (text_model, tokenizer, max_length).  Weights come from a LOCAL directory
    `model_path` only (a hub name is never resolved: no network on the training path); without one the
    tower is not built and callers pass precomputed latents.  The tokenizer is transformers' AutoTokenizer on
    the same directory when that package imports (local files only), else None."""
    text_model, tokenizer = None, None
    if language_emb_model == "clip" and model_path:
        if not os.path.isdir(model_path):
            raise FileNotFoundError(f"language_model_path {model_path!r} is not a local directory")
        sd = _load_clip_state(model_path)
        text_model = ClipTextTower(**_tower_dims(model_path))
        own = text_model.state_dict()
        missing = sorted(set(own) - set(sd))
        if missing:
            raise KeyError(f"{model_path}: CLIP text weights missing {missing[:4]}{'...' if len(missing) > 4 else ''}")
        text_model.load_state_dict({k: sd[k].float() for k in own})
        try:
            from transformers import AutoTokenizer
        except ImportError:
            AutoTokenizer = None
        has_files = any(os.path.exists(os.path.join(model_path, f)) for f in ("tokenizer.json", "vocab.json"))
        if AutoTokenizer is not None and has_files:  # a weights-only directory: tokens come from the dataset
            tokenizer = AutoTokenizer.from_pretrained(model_path, local_files_only=True)
    return text_model, tokenizer, MAX_LENGTH


def extract_text_features(text_model, text_tokens, language_emb_model):
    """language_model.py:25-33: text_tokens = {"input_ids", "attention_mask"} -> [B, 512] latents"""
    if language_emb_model != "clip":
        raise NotImplementedError(f"language_emb_model {language_emb_model!r}")
    with torch.no_grad():
        return text_model(text_tokens["input_ids"], text_tokens.get("attention_mask"))
