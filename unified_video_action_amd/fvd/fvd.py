"""Fréchet video distance over I3D logits (reference: fvd/fvd.py:47-115).

get_fvd_logits runs the HIP tower (fvd/i3d.py; its preprocess kernel is fvd.py:7-44).  frechet_distance is the
reference's formula -- unbiased covariance, symmetric matrix square root by SVD with
where(s < 1e-10, s, sqrt(s)), trace(S1 + S2) - 2 trace_sqrt + |m1 - m2|^2 -- evaluated on the host CPU in
float64: the operands are at most a few thousand x 400, and no vendor solver enters the GPU process.
Unlike the reference's `cov`, nothing here modifies its argument.
"""
import torch


def get_fvd_logits(videos, i3d, device=None):
    """videos: uint8 [B, T, H, W, 3] (numpy or torch) -> I3D logits [B, 400] fp32 on the tower's device"""
    return i3d(torch.as_tensor(videos))


def _symmetric_matrix_square_root(mat, eps=1e-10):
    u, s, vh = torch.linalg.svd(mat)
    si = torch.where(s < eps, s, torch.sqrt(s))
    return (u * si) @ vh


def trace_sqrt_product(sigma, sigma_v):
    sqrt_sigma = _symmetric_matrix_square_root(sigma)
    return torch.trace(_symmetric_matrix_square_root(sqrt_sigma @ (sigma_v @ sqrt_sigma)))


def cov(m):
    """unbiased covariance of the rows of m [n, d] -> [d, d]; m is left as it is"""
    c = m - m.mean(dim=0, keepdim=True)
    return (c.t() @ c) / (m.shape[0] - 1)


def frechet_distance(x1, x2):
    """-> float64 scalar tensor (CPU)"""
    x1 = torch.as_tensor(x1).detach().to("cpu", torch.float64).flatten(start_dim=1)
    x2 = torch.as_tensor(x2).detach().to("cpu", torch.float64).flatten(start_dim=1)
    if x1.shape[0] < 2 or x2.shape[0] < 2:
        raise ValueError("frechet_distance needs at least 2 samples per side (unbiased covariance)")
    m, m_w = x1.mean(dim=0), x2.mean(dim=0)
    sigma, sigma_w = cov(x1), cov(x2)
    trace = torch.trace(sigma + sigma_w) - 2.0 * trace_sqrt_product(sigma, sigma_w)
    return trace + torch.sum((m - m_w) ** 2)
