"""Fused attention at head_dim 80 / 128 without a GPU: the pure-host queries of the C ABI
(uva_attn_hd_supported, uva_attn_bwd_hd_part_floats) and the fake (meta) kernels + autograd formula of
uva::attention_hd / uva::attention_hd_backward (shape and dtype propagation, refusals)."""
import pytest
import torch

import unified_video_action_amd.native.torch_ops as T
from unified_video_action_amd.native.lib import lib

META = "meta"
CASES = [(80, 16), (128, 6)]  # mar_huge; mar_tiny / mar_small


def test_hd_supported_is_a_host_query():
    assert [lib().query("uva_attn_hd_supported", hd) for hd in (80, 128, 64, 96)] == [1, 1, 0, 0]
    from unified_video_action_amd.native import ops
    assert ops.attn_hd_supported(80) and ops.attn_hd_supported(128)
    assert not ops.attn_hd_supported(64) and not ops.attn_hd_supported(96)


@pytest.mark.parametrize("hd,H", CASES)
def test_bwd_part_floats_is_a_host_query(hd, H):
    """one row of 3 H head_dim floats per (batch, 128-row block); the last block may be half full"""
    q = lambda B, N: lib().query("uva_attn_bwd_hd_part_floats", B, N, H, hd)  # noqa: E731
    assert q(1, 64) == 3 * H * hd
    assert q(2, 192) == 2 * 2 * 3 * H * hd
    assert q(32, 1088) == 32 * 9 * 3 * H * hd


def test_ops_registered():
    for name in ("attention_hd", "attention_hd_backward"):
        assert hasattr(torch.ops.uva, name), name
    assert "SymInt head_dim" in str(torch.ops.uva.attention_hd.default._schema)
    # uva::attention keeps its schema
    assert "head_dim" not in str(torch.ops.uva.attention.default._schema)


@pytest.mark.parametrize("hd,H", CASES)
def test_attention_hd_meta_forward_backward(hd, H):
    qkv = torch.empty(2, 1088, 3 * H * hd, device=META, dtype=torch.bfloat16, requires_grad=True)
    out, lse = T.attention_hd(qkv, H, hd, 0.1, 3)
    assert out.shape == (2, 1088, H * hd) and out.dtype == torch.bfloat16
    assert lse.shape == (2, H, 1088) and lse.dtype == torch.float32
    out.float().sum().backward()
    assert qkv.grad.shape == qkv.shape and qkv.grad.dtype == torch.bfloat16
    d = T.attention_hd_backward(torch.empty_like(out), qkv.detach(), out.detach(), lse, H, hd, 0.1, 3)
    assert d.shape == qkv.shape and d.dtype == torch.bfloat16


@pytest.mark.parametrize("hd,H", CASES)
def test_attention_hd_meta_refusals(hd, H):
    ok = torch.empty(2, 128, 3 * H * hd, device=META, dtype=torch.bfloat16)
    out = torch.empty(2, 128, H * hd, device=META, dtype=torch.bfloat16)
    lse = torch.empty(2, H, 128, device=META)
    ragged = torch.empty(2, 72, 3 * H * hd, device=META, dtype=torch.bfloat16)
    narrow = torch.empty(2, 128, 3 * H * hd - 8, device=META, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="multiple of 64"):
        T.attention_hd(ragged, H, hd, 0.0, 0)
    with pytest.raises(ValueError, match="qkv must be"):
        T.attention_hd(narrow, H, hd, 0.0, 0)
    with pytest.raises(ValueError, match="qkv must be"):
        T.attention_hd(ok, H + 1, hd, 0.0, 0)
    with pytest.raises(ValueError, match="multiple of 64"):
        T.attention_hd_backward(out[:, :72], ragged, out[:, :72], lse[..., :72], H, hd, 0.0, 0)
    with pytest.raises(ValueError, match="qkv must be"):
        T.attention_hd_backward(out, narrow, out, lse, H, hd, 0.0, 0)
    with pytest.raises(ValueError, match="head_dim"):
        T.attention_hd(torch.empty(2, 128, 3 * H * 96, device=META, dtype=torch.bfloat16), H, 96, 0.0, 0)
    # uva::attention keeps its errors: a head_dim-128 qkv is not [B, N, 3*heads*64]
    with pytest.raises(ValueError, match=r"3\*heads\*64"):
        T.attention(torch.empty(2, 128, 3 * 5 * 128, device=META, dtype=torch.bfloat16), 6, 0.0, 0)
