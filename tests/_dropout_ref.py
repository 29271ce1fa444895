"""Host restatement of the library's dropout draw and explicit-mask float64 attention references.

The dropout mask of every kernel is a pure function of (seed, element index, p) (csrc/common.h: favit_rand_u32,
favit_mix_u32, favit_keep, dropout_threshold).  keep_mask restates it in 32-bit-wrapped integer arithmetic on the
host, so that a test can build the mask explicitly and run plain float64 attention with it under autograd: that gives
O, dQ, dK and dV of a dropout kernel exactly, per row, without trusting any kernel's own index arithmetic.

numpy / torch only; runs on the CPU.  tests/test_dropout_ref_host.py checks this module against the golden-checked
oracle; tests/test_gpu_dropout_masks.py ties keep_mask to favit_dropout bit for bit and then leans on it."""
import numpy as np
import torch

from oracle import favit_oracle as O

_M32 = np.uint64(0xFFFFFFFF)


def _mix_u32(x):
    """favit_mix_u32 (the "lowbias32" finaliser) on uint64 arrays that hold 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def rand_u32(seed, idx):
    """favit_rand_u32(seed, idx): one 32-bit draw per 64-bit counter value (idx: array of non-negative integers)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k1 = np.uint64(((seed & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF | 1)
    k2 = np.uint64(((seed >> 32) * 0x85EBCA77) & 0xFFFFFFFF)
    idx = np.asarray(idx).astype(np.uint64)
    lo, hi = idx & _M32, idx >> np.uint64(32)
    # every product below is < 2^64 (32-bit by 32-bit), so uint64 arithmetic followed by a mask wraps as uint32 does
    x = ((lo * k1) & _M32) + k2 + ((hi * np.uint64(0xC2B2AE3D)) & _M32)
    return _mix_u32(x & _M32)


def threshold16(p):
    """dropout_threshold(p) >> 16: p is a C float; floor(p * 2^32), clamped to 32 bits, upper half."""
    t = float(np.float32(p)) * 4294967296.0
    t32 = 0 if t <= 0 else 0xFFFFFFFF if t >= 4294967295.0 else int(t)
    return t32 >> 16


def keep_scale(p):
    """1 / (1 - p) as the kernels compute it (fp32)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed, n_or_indices, p):
    """favit_keep(seed, idx, dropout_threshold(p)) for idx = 0 .. n-1 (an int) or for an array of indices (any shape):
    element idx is decided by the draw of the pair idx >> 1, its low half for even idx and its high half for odd idx,
    and is kept when that half is >= floor(p * 2^32) >> 16.  Returns a numpy bool array."""
    idx = np.arange(n_or_indices, dtype=np.uint64) if np.isscalar(n_or_indices) else np.asarray(n_or_indices).astype(np.uint64)
    h = rand_u32(seed, idx >> np.uint64(1))
    half = np.where((idx & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return half >= np.uint64(threshold16(p))


def mhla_keep(seed, B, H, L, W, p, device="cpu"):
    """The [B, H, L, W] mask of the MHLA kernels: slot index ((b*H + head)*L + i)*W + w, w = position in the window
    (pad copies of key 0 / key L-1 are slots of their own, each with its own draw)."""
    return torch.from_numpy(keep_mask(seed, B * H * L * W, p).reshape(B, H, L, W)).to(device)


def sdpa_keep(seed, B, H, Lq, Lk, p, device="cpu"):
    """The [B, H, Lq, Lk] mask of the fused dense attention: index ((b*H + h)*Lq + q)*Lk + k."""
    return torch.from_numpy(keep_mask(seed, B * H * Lq * Lk, p).reshape(B, H, Lq, Lk)).to(device)


def mhla_core(q, k, v, W, mask=None, keep=None, p=0.0):
    """The attention core in the window-gather formulation (gather the W window keys of every row, pad copies
    included, softmax over the W slots, P = softmax * keep / (1 - p) per slot).  q, k, v: float64 [B, H, L, hd];
    mask: [B, L, L] (0 = -inf) or None; keep: bool [B, H, L, W] or None.  Returns (out [B, H, L, hd], lse [B, H, L]);
    lse is that of the undropped, masked scores."""
    B, H, L, hd = q.shape
    idx = torch.from_numpy(O.window_indices(L, W)).to(q.device)
    kw, vw = k[:, :, idx], v[:, :, idx]                                       # [B, H, L, W, hd]
    s = (q.unsqueeze(3) @ kw.transpose(-2, -1)).squeeze(3) / (hd ** 0.5)      # [B, H, L, W]
    if mask is not None:
        wm = torch.gather(mask[:, None].expand(B, H, L, L), 3, idx[None, None].expand(B, H, L, W))
        s = s.masked_fill(wm == 0, float("-inf"))
    P = torch.softmax(s, -1)
    if keep is not None:
        P = P * keep.to(P.dtype) / (1.0 - p)
    return (P.unsqueeze(3) @ vw).squeeze(3), torch.logsumexp(s.detach(), -1)


def mhla_ref(qkv64, dout64, B, L, H, hd, W, mask, keep, p):
    """float64 reference of favit_mhla_attn_fwd / _bwd with an explicit dropout mask.  qkv64 [B*L, 3D] (column
    s*D + h*hd + d), dout64 [B*L, D].  Returns (out [B*L, D], dqkv [B*L, 3D], lse [B, H, L])."""
    D = H * hd
    t = qkv64.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).detach().clone().requires_grad_(True)
    o, lse = mhla_core(t[0], t[1], t[2], W, mask, keep, p)
    out = o.transpose(1, 2).reshape(B * L, D)
    out.backward(dout64.double())
    return out.detach(), t.grad.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * D), lse


def _sdpa_probs(q, k, scale, mask):
    """Masked scores and their softmax (float64); a row with every key masked has P = 0, not torch's NaN."""
    s = (q @ k.transpose(-2, -1)) * scale
    if mask is None:
        return s, torch.softmax(s, -1)
    s = s.masked_fill(~mask, float("-inf"))
    dead = ~mask.expand(s.shape).any(-1, keepdim=True)
    return s, torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead | ~mask, 0.0)


def sdpa_ref(q, k, v, dout, scale, mask, keep, p):
    """float64 reference of favit_sdpa_fwd / _bwd with an explicit dropout mask.  q, dout [B, H, Lq, hd], k, v
    [B, H, Lk, hd]; mask broadcastable to [B, H, Lq, Lk] (bool, False = -inf) or None; keep bool [B, H, Lq, Lk] or None.
    A query row with every key masked has P = 0 (output 0, no gradient), not torch's NaN.
    Returns (o, lse, dq, dk, dv); lse is that of the undropped, masked scores (-inf for a fully masked row)."""
    qr, kr, vr = (t.double().detach().clone().requires_grad_(True) for t in (q, k, v))
    s, P = _sdpa_probs(qr, kr, scale, mask)
    if keep is not None:
        P = P * keep.to(P.dtype) / (1.0 - p)
    o = P @ vr
    o.backward(dout.double())
    return o.detach(), torch.logsumexp(s.detach(), -1), qr.grad, kr.grad, vr.grad


def cross_attention_ref(q_in, kv_in, sd, H, mask=None, p=""):
    """O.cross_attention (H = 1: one head of width D, scores / D**0.5) and O.multihead_cross_attention restated around
    _sdpa_probs, so that a query row with every key masked has P = 0 where the oracle's torch.softmax gives NaN: its
    output row is out_proj.bias and it sends no gradient into q, k or v.  q_in [B, Lq, D], kv_in [B, Lk, D], mask
    [B, Lq, Lk] (0 = masked) or None; any float dtype (tests/test_head_widths_host.py ties it to the oracle in float64)."""
    B, Lq, D = q_in.shape
    Lk, hd = kv_in.shape[1], D // H
    q = O.linear(q_in, sd[f"{p}q_proj.weight"], sd[f"{p}q_proj.bias"]).reshape(B, Lq, H, hd).permute(0, 2, 1, 3)
    k = O.linear(kv_in, sd[f"{p}k_proj.weight"], sd[f"{p}k_proj.bias"]).reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
    v = O.linear(kv_in, sd[f"{p}v_proj.weight"], sd[f"{p}v_proj.bias"]).reshape(B, Lk, H, hd).permute(0, 2, 1, 3)
    _, P = _sdpa_probs(q, k, 1.0 / hd ** 0.5, None if mask is None else (mask != 0)[:, None])
    o = (P @ v).permute(0, 2, 1, 3).reshape(B, Lq, D)
    return O.linear(o, sd[f"{p}out_proj.weight"], sd[f"{p}out_proj.bias"])


def sdpa_grad_scale(q, k, v, dout, scale, mask, keep, p):
    """The size of the terms whose sum is dq and dk: dS = P (dP - delta) with |dP| + |delta| in place of the
    difference and |k|, |q| in place of k, q.  Where a gradient is identically zero by cancellation (one key:
    softmax is constant, so dq = dk = 0), a relative error against the reference is undefined and the error of a
    kernel is measured against this instead.  Returns (|dq| scale [B, H, Lq, hd], |dk| scale [B, H, Lk, hd])."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    _, P = _sdpa_probs(q, k, scale, mask)
    dP = dout @ v.transpose(-2, -1)
    if keep is not None:
        dP = dP * keep.to(dP.dtype) / (1.0 - p)
    delta = (P * dP).sum(-1, keepdim=True)
    gross = P * (dP.abs() + delta.abs()) * scale
    return gross @ k.abs(), gross.transpose(-2, -1) @ q.abs()
