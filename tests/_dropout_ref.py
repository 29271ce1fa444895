"""Host restatement of the library's dropout draw and explicit-mask float64 attention references.

The dropout mask of every kernel is a pure function of (seed, element index, p) (csrc/common.h: favit_rand_u32,
favit_mix_u32, favit_keep, dropout_threshold).  keep_mask restates it in 32-bit-wrapped integer arithmetic on the
host, so that a test can build the mask explicitly and run plain float64 attention with it under autograd: that gives
O, dQ, dK and dV of a dropout kernel exactly, per row, without trusting any kernel's own index arithmetic.

The MHLA references also carry the mask side of the contract: a query row whose window slots are all masked has P = 0
(mhla_core), mask_family builds the structured masks that produce such rows (padding, whole rows, whole images, rows that
live through pad copies alone), mhla_grad_scale gives the size of the terms that cancel in dq / dk on them, and
mhla_attention_ref is the module around that core.  tests/test_gpu_mhla_masks.py runs the kernels against them.

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
    lse is that of the undropped, masked scores.  A row whose W window slots are all masked has P = 0 (output 0, no
    gradient, lse = -inf), not torch's NaN: the construction of _sdpa_probs.  Without such a row the result is bit for
    bit what plain masked_fill + softmax gives (tests/test_dropout_ref_host.py)."""
    B, H, L, hd = q.shape
    idx = torch.from_numpy(O.window_indices(L, W)).to(q.device)
    kw, vw = k[:, :, idx], v[:, :, idx]                                       # [B, H, L, W, hd]
    s = (q.unsqueeze(3) @ kw.transpose(-2, -1)).squeeze(3) / (hd ** 0.5)      # [B, H, L, W]
    if mask is None:
        P = torch.softmax(s, -1)
    else:
        wm = torch.gather(mask[:, None].expand(B, H, L, L), 3, idx[None, None].expand(B, H, L, W)) != 0
        s = s.masked_fill(~wm, float("-inf"))
        dead = ~wm.any(-1, keepdim=True)
        P = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead | ~wm, 0.0)
    if keep is not None:
        P = P * keep.to(P.dtype) / (1.0 - p)
    return (P.unsqueeze(3) @ vw).squeeze(3), torch.logsumexp(s.detach(), -1)


def mhla_dead_rows(mask, L, W):
    """bool [B, L]: the query rows whose W window slots (pad copies included) are all masked."""
    idx = torch.from_numpy(O.window_indices(L, W)).to(mask.device)
    B = mask.shape[0]
    return ~(torch.gather(mask, 2, idx[None].expand(B, L, W)) != 0).any(-1)


MASK_FAMILIES = ("rows", "padding", "identity", "ends", "image")


def _random_mask(B, L, gen):
    """The mask of every older MHLA test: 60 % kept at random, and the diagonal."""
    return (torch.rand(B, L, L, generator=gen) > 0.4) | torch.eye(L, dtype=torch.bool)


def rows_family_dead(B, L):
    """The (b, i) rows the "rows" family zeroes: first and last row (pad copies), the seam of two 16-row tiles, the
    two-block seam of the default backward at L = 70, the 48-row block seam of the saved-statistics backward."""
    want = [(0, 0), (0, L - 1), (1, 15), (1, 16), (0, L // 2), (0, L // 2 + 1), (1, 47), (1, 48)]
    return sorted({(b, min(i, L - 1)) for b, i in want if b < B})


def mask_family(name, B, L, W, gen):
    """Structured [B, L, L] bool masks (True = keep), built on the CPU from the torch.Generator `gen`:
      rows      the random mask with the diagonal, and the rows of rows_family_dead zeroed;
      padding   mask[b, :, j] = j < n_b with n = (max(1, L // 2), 1, L, L, ...): whole key columns masked.  Row i of image
                b is dead for n_b + h <= i <= L - 1 - h; the last h rows live through the front pad copies of key 0 alone;
      identity  only the diagonal: P = 1 on one slot, out = v, dv = dout, dq = dk = 0;
      ends      only key columns 0 and L - 1: rows near the two ends live through keys 0 / L - 1 and their pad copies,
                rows h < i < L - 1 - h are dead;
      image     image 0 gets the random mask with the diagonal, every other image is all zero."""
    if name == "rows":
        m = _random_mask(B, L, gen)
        for b, i in rows_family_dead(B, L):
            m[b, i] = False
    elif name == "padding":
        n = [max(1, L // 2), 1] + [L] * B
        m = (torch.arange(L)[None, None, :] < torch.tensor(n[:B])[:, None, None]).expand(B, L, L).clone()
    elif name == "identity":
        m = torch.eye(L, dtype=torch.bool)[None].expand(B, L, L).clone()
    elif name == "ends":
        m = torch.zeros(B, L, L, dtype=torch.bool)
        m[:, :, 0] = True
        m[:, :, L - 1] = True
    elif name == "image":
        m = torch.zeros(B, L, L, dtype=torch.bool)
        m[0] = _random_mask(1, L, gen)[0]
    else:
        raise ValueError(name)
    return m


def mask_family_dead_count(name, B, L, W):
    """The number of dead (b, i) rows of mask_family(name, B, L, W, .) in closed form (the host test ties it to
    mhla_dead_rows, the GPU tests assert it, so that a case cannot lose its dead rows unnoticed)."""
    h = W // 2
    if name == "rows":
        return len(rows_family_dead(B, L))
    if name == "padding":
        n = ([max(1, L // 2), 1] + [L] * B)[:B]
        return sum(max(0, L - nb - 2 * h) for nb in n)
    if name == "identity":
        return 0
    if name == "ends":
        return B * max(0, L - 2 - 2 * h)
    if name == "image":
        return (B - 1) * L
    raise ValueError(name)


def mask_to_u8(name, mask, gen):
    """The uint8 form the kernels read.  Any non-zero byte keeps: the "rows" family stores its kept entries as 1, 2 or
    255 at random, every other family as 1."""
    m = mask.to(torch.uint8)
    if name == "rows":
        m = m * torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, mask.shape, generator=gen)]
    return m.contiguous()


def mhla_ref(qkv64, dout64, B, L, H, hd, W, mask, keep, p):
    """float64 reference of favit_mhla_attn_fwd / _bwd with an explicit dropout mask.  qkv64 [B*L, 3D] (column
    s*D + h*hd + d), dout64 [B*L, D].  Returns (out [B*L, D], dqkv [B*L, 3D], lse [B, H, L])."""
    D = H * hd
    t = qkv64.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).detach().clone().requires_grad_(True)
    o, lse = mhla_core(t[0], t[1], t[2], W, mask, keep, p)
    out = o.transpose(1, 2).reshape(B * L, D)
    out.backward(dout64.double())
    return out.detach(), t.grad.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * D), lse


def mhla_grad_scale(qkv64, dout64, B, L, H, hd, W, mask, keep, p):
    """The size of the terms whose sum is dq and dk of the MHLA core, the analogue of sdpa_grad_scale: per window slot
    P (|dP| + |delta|) / sqrt(hd), times |k| of the slot's key summed over the row's slots (dq), and times |q| of the row
    scattered onto the slot's key (dk).  Rows with one or two surviving keys cancel (one key: dq = dk = 0 identically),
    so the error of a kernel on them is measured against this, not against the difference.  Returns [B*L, 3D] in the
    layout of dqkv; the dv part is zero (dv is a plain sum: its reference is its own scale)."""
    D = H * hd
    t = qkv64.double().reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    g = dout64.double().reshape(B, L, H, hd).permute(0, 2, 1, 3)
    idx = torch.from_numpy(O.window_indices(L, W)).to(q.device)
    kw, vw = k[:, :, idx], v[:, :, idx]
    s = (q.unsqueeze(3) @ kw.transpose(-2, -1)).squeeze(3) / (hd ** 0.5)
    if mask is None:
        P = torch.softmax(s, -1)
    else:
        wm = torch.gather(mask[:, None].expand(B, H, L, L), 3, idx[None, None].expand(B, H, L, W)) != 0
        dead = ~wm.any(-1, keepdim=True)
        P = torch.softmax(s.masked_fill(~wm, float("-inf")).masked_fill(dead, 0.0), -1).masked_fill(dead | ~wm, 0.0)
    dP = (g.unsqueeze(3) @ vw.transpose(-2, -1)).squeeze(3)
    if keep is not None:
        dP = dP * keep.to(dP.dtype) / (1.0 - p)
    delta = (P * dP).sum(-1, keepdim=True)
    gross = P * (dP.abs() + delta.abs()) / (hd ** 0.5)                        # [B, H, L, W]
    dq = (gross.unsqueeze(3) @ kw.abs()).squeeze(3)                           # [B, H, L, hd]
    contrib = (gross.unsqueeze(-1) * q.abs().unsqueeze(3)).reshape(B, H, L * W, hd)
    dk = torch.zeros_like(dq).index_add_(2, idx.reshape(-1), contrib)
    out = torch.zeros(B, L, 3, H, hd, dtype=torch.float64, device=q.device)
    out[:, :, 0] = dq.permute(0, 2, 1, 3)
    out[:, :, 1] = dk.permute(0, 2, 1, 3)
    return out.reshape(B * L, 3 * D)


def row_error(got, ref, denom, rows):
    """Per-row error of a [rows, D] result, |got - ref| of a row over |denom row| + 1e-3 |denom| / sqrt(rows): the
    denominator of test_mhla_saved_statistics_backward_sweep with `denom` = ref (out, dv), or the gross-term rows of
    mhla_grad_scale (dq, dk: rows with one or two surviving keys cancel).  Returns the [rows] errors."""
    a, b, d = (t.double().reshape(rows, -1) for t in (got, ref, denom))
    return (a - b).norm(dim=-1) / (d.norm(dim=-1) + 1e-3 * d.norm() / rows ** 0.5).clamp_min(1e-300)


def mhla_attention_ref(x, sd, p, H, W, mask=None):
    """oracle.favit_oracle.mhla_attention restated around mhla_core, as cross_attention_ref restates the cross modules:
    a query row whose window keys are all masked has P = 0 where the oracle's torch.softmax gives NaN, so its output row
    is proj.bias and it sends no gradient into q, k or v.  x [B, L, D], mask [B, L, L] (0 = masked) or None; any float
    dtype (tests/test_dropout_ref_host.py ties it to the oracle in float64)."""
    B, L, D = x.shape
    hd = D // H
    qkv = O.linear(x, sd[f"{p}qkv.weight"], sd[f"{p}qkv.bias"]).reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    wl, bl = sd[f"{p}latent_proj.weight"], sd[f"{p}latent_proj.bias"]
    o, _ = mhla_core(qkv[0], O.linear(qkv[1], wl, bl), O.linear(qkv[2], wl, bl), W, mask)
    return O.linear(o.transpose(1, 2).reshape(B, L, D), sd[f"{p}proj.weight"], sd[f"{p}proj.bias"])


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
