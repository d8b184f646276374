"""I3D feature tower on libuva_hip.so (reference: fvd/pytorch_i3d.py InceptionI3d(400, in_channels=3), the
network behind the epoch-end FVD of eval/eval.py:128-280).

Inception-v1 inflated to 3-D: a 7x7x7 / stride-2 stem, four zero-padding max pools, nine Inception modules,
an average pool over [2, 7, 7], a 1024 -> 400 logits layer and the mean over the remaining time positions.
`InceptionI3dTower` keeps the reference's parameter and buffer names, so its `i3d_pretrained_400.pt` loads by
name.  Eval-mode BatchNorm (eps 1e-5) is folded into every unit's weight and bias once, on the host, in fp32;
weights are laid out [Co][kt][kh][kw][Ci] (fp32 and a bf16 shadow).  Activations are channels-last
[N][T][H][W][C]; a module's four branches write their slices of one output buffer.

Kernels: uva_fvd_preprocess, uva_conv3d (3x3x3 units and the stem, on its 8-channel padded input),
uva_maxpool3d, uva_i3d_head (csrc/i3d.hip) and uva_gemm for the 1x1x1 units (bias + ReLU epilogue).
precision "fp32" runs the VALU parity routes, "bf16" the MFMA routes.  The tower is frozen and forward-only.
There is no torch fallback: without a GPU the forward raises.
"""
import os

import torch
import torch.nn as nn

from ..native import ops

F32 = torch.float32
BN_EPS = 1e-5
STEM_CPAD = 8  # the stem's input channels: RGB + 5 zero channels (Ci % 8 == 0 for the implicit GEMM)
MIXED = (  # name, in_channels, [b0, b1a, b1b, b2a, b2b, b3b]  (pytorch_i3d.py:291-365)
    ("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)),
    ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
    ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)),
    ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
    ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)),
    ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
    ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)),
    ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
    ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)),
)
POOLS = {  # kernel, stride (pytorch_i3d.py:255-352)
    "MaxPool3d_2a_3x3": ((1, 3, 3), (1, 2, 2)),
    "MaxPool3d_3a_3x3": ((1, 3, 3), (1, 2, 2)),
    "MaxPool3d_4a_3x3": ((3, 3, 3), (2, 2, 2)),
    "MaxPool3d_5a_2x2": ((2, 2, 2), (2, 2, 2)),
}
ENDPOINTS = ("Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2c_3x3", "MaxPool3d_3a_3x3", "Mixed_3b",
             "Mixed_3c", "MaxPool3d_4a_3x3", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f",
             "MaxPool3d_5a_2x2", "Mixed_5b", "Mixed_5c")


class _Conv(nn.Module):
    def __init__(self, ci, co, k, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(co, ci, *k))
        if bias:
            self.bias = nn.Parameter(torch.zeros(co))


class Unit3D(nn.Module):
    """the names of the reference's Unit3D: conv3d.weight (no bias) + bn.*, or conv3d.weight / .bias (logits)"""

    def __init__(self, ci, co, k=(1, 1, 1), stride=(1, 1, 1), bn=True, bias=False):
        super().__init__()
        self.kernel, self.stride = tuple(k), tuple(stride)
        self.conv3d = _Conv(ci, co, self.kernel, bias)
        if bn:
            self.bn = nn.BatchNorm3d(co, eps=BN_EPS, momentum=0.001)


class InceptionModule(nn.Module):
    def __init__(self, ci, oc):
        super().__init__()
        self.b0 = Unit3D(ci, oc[0])
        self.b1a = Unit3D(ci, oc[1])
        self.b1b = Unit3D(oc[1], oc[2], (3, 3, 3))
        self.b2a = Unit3D(ci, oc[3])
        self.b2b = Unit3D(oc[3], oc[4], (3, 3, 3))
        self.b3b = Unit3D(ci, oc[5])
        self.out_channels = oc[0] + oc[2] + oc[4] + oc[5]


def fold_unit(weight, bias, bn_weight, bn_bias, mean, var, eps=BN_EPS):
    """eval-mode BatchNorm folded into a conv, fp32: y = conv(x; w s) + (beta + (b - mean) s), s = gamma /
    sqrt(var + eps).  -> (w [Co][kt][kh][kw][Ci], bias [Co])"""
    w = weight.detach().to(F32)
    co = w.shape[0]
    b = bias.detach().to(F32) if bias is not None else torch.zeros(co, dtype=F32, device=w.device)
    if bn_weight is not None:
        s = bn_weight.detach().to(F32) / torch.sqrt(var.detach().to(F32) + eps)
        w = w * s.view(co, 1, 1, 1, 1)
        b = bn_bias.detach().to(F32) + (b - mean.detach().to(F32)) * s
    return w.permute(0, 2, 3, 4, 1).contiguous(), b.contiguous()


def _invalidate(module, *args):
    module._operands = None


class InceptionI3dTower(nn.Module):
    """forward(videos uint8 [B, T, H, W, 3]) -> logits [B, num_classes] fp32, the value of
    InceptionI3d(400)(preprocess(videos)) in eval mode (fvd.py:47-50 get_fvd_logits)."""

    def __init__(self, num_classes=400, in_channels=3, precision="fp32", clips_per_batch=16):
        super().__init__()
        if in_channels != 3:
            raise ValueError("InceptionI3dTower: RGB input (in_channels = 3) only")
        self.num_classes = num_classes
        self.clips_per_batch = clips_per_batch
        self.logits = Unit3D(1024, num_classes, bn=False, bias=True)
        self.Conv3d_1a_7x7 = Unit3D(3, 64, (7, 7, 7), (2, 2, 2))
        self.Conv3d_2b_1x1 = Unit3D(64, 64)
        self.Conv3d_2c_3x3 = Unit3D(64, 192, (3, 3, 3))
        for name, ci, oc in MIXED:
            setattr(self, name, InceptionModule(ci, oc))
        for p in self.parameters():
            p.requires_grad = False
        self.set_precision(precision)
        self._operands = None
        self.register_load_state_dict_post_hook(_invalidate)
        super().train(False)

    def set_precision(self, precision):
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"I3D precision must be 'fp32' or 'bf16', got {precision!r}")
        self.precision = precision

    def train(self, mode=True):
        return super().train(False)  # frozen: eval only (BatchNorm folded, dropout off)

    def _apply(self, fn, *args, **kwargs):
        self._operands = None
        return super()._apply(fn, *args, **kwargs)

    def units(self):
        """name -> Unit3D for every conv unit, in the reference's state-dict order"""
        out = {"logits": self.logits, "Conv3d_1a_7x7": self.Conv3d_1a_7x7, "Conv3d_2b_1x1": self.Conv3d_2b_1x1,
               "Conv3d_2c_3x3": self.Conv3d_2c_3x3}
        for name, _, _ in MIXED:
            m = getattr(self, name)
            for b in ("b0", "b1a", "b1b", "b2a", "b2b", "b3b"):
                out[f"{name}.{b}"] = getattr(m, b)
        return out

    def operands(self):
        """folded operands per unit: {"f32": (w, b), "bf16": (w, b)}, w [Co][kt][kh][kw][Ci] ([Co][Ci] for the
        1x1x1 units; the stem's Ci zero-padded to 8).  Made once after a load or a move."""
        dev = self.logits.conv3d.weight.device
        if self._operands is not None and self._operands[0] == dev:
            return self._operands[1]
        ops_ = {}
        for name, u in self.units().items():
            bn = getattr(u, "bn", None)
            w, b = fold_unit(u.conv3d.weight, getattr(u.conv3d, "bias", None),
                             bn.weight if bn is not None else None, bn.bias if bn is not None else None,
                             bn.running_mean if bn is not None else None, bn.running_var if bn is not None else None)
            if name == "Conv3d_1a_7x7":
                w = torch.nn.functional.pad(w, (0, STEM_CPAD - w.shape[-1])).contiguous()
            if u.kernel == (1, 1, 1):
                w = w.reshape(w.shape[0], w.shape[-1]).contiguous()
            ops_[name] = {"fp32": (w, b), "bf16": (w.to(torch.bfloat16), b)}
        self._operands = (dev, ops_)
        return ops_

    # ---- layers ------------------------------------------------------------------------------------------
    def _conv(self, name, x, out2d=None, coff=0):
        """3-D conv unit (+ folded bn + relu) on x [N,T,H,W,Ci]; writes channels coff.. of out2d when given"""
        u = self.units()[name]
        w, b = self.operands()[name][self.precision]
        N, T, H, W, _ = x.shape
        (pt, To), (ph, Ho), (pw, Wo) = ops.same_pad_3d((T, H, W), u.kernel, u.stride)
        co = w.shape[0]
        own = out2d is None
        if own:
            out2d = torch.empty(N * To * Ho * Wo, co, dtype=x.dtype, device=x.device)
        ops.conv3d(x, w, out2d, bias=b, stride=u.stride, pads=(pt, ph, pw), out_size=(To, Ho, Wo), coff=coff, act="relu")
        return out2d.view(N, To, Ho, Wo, co) if own else None

    def _point(self, name, x, out2d=None, coff=0):
        """1x1x1 unit: a plain product on uva_gemm, bias + ReLU, written at channel coff of out2d"""
        w, b = self.operands()[name][self.precision]
        co = w.shape[0]
        x2d = x.reshape(-1, x.shape[-1])
        own = out2d is None
        if own:
            out2d = torch.empty(x2d.shape[0], co, dtype=x.dtype, device=x.device)
        ops.linear(x2d, w, out2d[:, coff:coff + co], bias=b, act="relu")
        return out2d.view(*x.shape[:-1], co) if own else None

    def _pool(self, x, kernel, stride):
        N, T, H, W, C = x.shape
        (pt, To), (ph, Ho), (pw, Wo) = ops.same_pad_3d((T, H, W), kernel, stride)
        out = torch.empty(N, To, Ho, Wo, C, dtype=x.dtype, device=x.device)
        ops.maxpool3d(x, out, kernel, stride, (pt, ph, pw), (To, Ho, Wo))
        return out

    def _mixed(self, name, x):
        m = getattr(self, name)
        N, T, H, W, _ = x.shape
        out = torch.empty(N * T * H * W, m.out_channels, dtype=x.dtype, device=x.device)
        c0 = m.b0.conv3d.weight.shape[0]
        c1 = m.b1b.conv3d.weight.shape[0]
        c2 = m.b2b.conv3d.weight.shape[0]
        self._point(f"{name}.b0", x, out, 0)
        self._conv(f"{name}.b1b", self._point(f"{name}.b1a", x), out, c0)
        self._conv(f"{name}.b2b", self._point(f"{name}.b2a", x), out, c0 + c1)
        self._point(f"{name}.b3b", self._pool(x, (3, 3, 3), (1, 1, 1)), out, c0 + c1 + c2)
        return out.view(N, T, H, W, m.out_channels)

    def features(self, x, endpoints=None):
        """preprocessed clips x [N,T,224,224,8] -> Mixed_5c [N,T/8,7,7,1024]; endpoints: a dict that
        receives every named endpoint (channels-last tensors)"""
        for name in ENDPOINTS:
            if name in POOLS:
                x = self._pool(x, *POOLS[name])
            elif name.startswith("Mixed"):
                x = self._mixed(name, x)
            elif name == "Conv3d_2b_1x1":
                x = self._point(name, x)
            else:
                x = self._conv(name, x)
            if endpoints is not None:
                endpoints[name] = x
        return x

    @torch.no_grad()
    def forward(self, videos, endpoints=None):
        dev = self.logits.conv3d.weight.device
        if dev.type != "cuda":
            raise RuntimeError("InceptionI3dTower runs on libuva_hip.so kernels: move it to the GPU (no CPU fallback)")
        if not torch.is_tensor(videos):
            videos = torch.as_tensor(videos)
        if videos.dtype != torch.uint8 or videos.dim() != 5 or videos.shape[-1] != 3:
            raise ValueError(f"videos must be uint8 [B, T, H, W, 3], got {videos.dtype} {tuple(videos.shape)}")
        if endpoints is not None and videos.shape[0] > self.clips_per_batch:
            raise ValueError("endpoints are recorded for a single clip batch")
        c = F32 if self.precision == "fp32" else torch.bfloat16
        w, b = self.operands()["logits"]["fp32"]
        outs = []
        for i in range(0, videos.shape[0], self.clips_per_batch):
            v = videos[i:i + self.clips_per_batch].to(dev).contiguous()
            B, T = v.shape[:2]
            x = torch.empty(B, T, 224, 224, STEM_CPAD, dtype=c, device=dev)
            ops.fvd_preprocess(v, x)
            x = self.features(x, endpoints)
            out = torch.empty(B, self.num_classes, dtype=F32, device=dev)
            ops.i3d_head(x, w, b, out)
            outs.append(out)
        return outs[0] if len(outs) == 1 else torch.cat(outs)


def load_i3d_pretrained(path, device="cuda", precision="fp32"):
    """InceptionI3dTower with the weights of a LOCAL i3d_pretrained_400.pt (the reference's state-dict layout,
    fvd/download.py:39-50), read through the code-free loader of workspace/checkpoint.py.  Nothing is ever
    downloaded: a missing path raises FileNotFoundError."""
    if not path or not os.path.isfile(path):
        raise FileNotFoundError(f"I3D weights {path!r}: not a local file (training.i3d_pretrained_path must name "
                                "the reference's i3d_pretrained_400.pt; nothing is downloaded)")
    from ..workspace.checkpoint import safe_load
    sd = safe_load(path, map_location="cpu")
    tower = InceptionI3dTower(400, precision=precision)
    own = tower.state_dict()
    missing = sorted(set(own) - set(sd))
    if missing:
        raise KeyError(f"{path}: I3D weights missing {missing[:4]}{'...' if len(missing) > 4 else ''}")
    tower.load_state_dict({k: sd[k] for k in own})
    return tower.to(device)
