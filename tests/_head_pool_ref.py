"""float64 definitions of the mean-pooled head in both orders (the tests' reference; gradients by autograd).

    norm-first  layer_norm(x[:, first:]).mean(1)        the model's `norm` on every pooled token, then the mean
    pool-first  layer_norm(x[:, first:].mean(1))        timm's fc_norm: the mean, then the LayerNorm of B rows
"""
import torch
import torch.nn.functional as TF


def head_pool(x, gamma, beta, norm_first, first=1, eps=1e-5):
    """x [B, L, D], gamma / beta [D] (any float dtype, computed in float64) -> [B, D] float64."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    D = x.shape[-1]
    if norm_first:
        return TF.layer_norm(x[:, first:], (D,), gamma, beta, eps).mean(1)
    return TF.layer_norm(x[:, first:].mean(1), (D,), gamma, beta, eps)


def head_pool_grads(x, gamma, beta, dy, norm_first, first=1, eps=1e-5):
    """(y, dx, dgamma, dbeta) in float64 for the upstream gradient dy [B, D]."""
    x = x.detach().double().requires_grad_(True)
    gamma = gamma.detach().double().requires_grad_(True)
    beta = beta.detach().double().requires_grad_(True)
    y = head_pool(x, gamma, beta, norm_first, first, eps)
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), dy.double())
    return y.detach(), dx, dg, db


def closed_form_backward(x, gamma, dy, norm_first, first=1, eps=1e-5):
    """The backward the kernels compute, written out in float64 (no autograd): (dx, dgamma, dbeta).
    norm-first: every pooled row gets the LayerNorm input gradient of dy[b] * gamma / n; dgamma = sum_b dy[b] * s[b]
    with s[b] the mean of the normalised rows; dbeta = sum_b dy[b].  pool-first: the LayerNorm backward of the pooled
    row, spread as dp[b] / n.  Rows below `first` are zero in both."""
    x, gamma, dy = x.double(), gamma.double(), dy.double()
    B, L, D = x.shape
    n = L - first
    dx = torch.zeros_like(x)

    def ln_bwd(rows, g):                                   # input gradient of LayerNorm for upstream g (pre-affine)
        mu = rows.mean(-1, keepdim=True)
        rs = (rows.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
        xh = (rows - mu) * rs
        return rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True)), xh

    if norm_first:
        g = (dy * gamma / n)[:, None, :].expand(B, n, D)
        dx[:, first:], xh = ln_bwd(x[:, first:], g)
        s = xh.mean(1)
    else:
        dp, s = ln_bwd(x[:, first:].mean(1), dy * gamma)
        dx[:, first:] = (dp / n)[:, None, :]
    return dx, (dy * s).sum(0), dy.sum(0)
