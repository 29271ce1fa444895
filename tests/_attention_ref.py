"""Float64 restatement of the attention maps for the tests: window / dense probabilities from a
stored qkv tensor, attention rollout as a scatter over (row, slot), and whole-model passes that keep every block's
probabilities.  Built on the oracle's pieces (window_indices, layer_norm, linear, patch_embed, ...), never on the
package under test."""
import numpy as np
import torch

from oracle import favit_oracle as O


def _split_qk(qkv, B, L, H, hd):
    """q, k float64 [B, H, L, hd] of a stored [B*L, 3*H*hd] tensor (column = s*D + h*hd + d), upcast exactly."""
    t = qkv.detach().cpu().to(torch.float64).reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _masked_softmax(s, keep):
    """softmax over the last dim of float64 s with keep (bool, broadcastable) or None; rows without a kept entry are 0."""
    if keep is None:
        return torch.softmax(s, dim=-1)
    keep = keep.expand_as(s)
    s = s.masked_fill(~keep, float("-inf"))
    m = s.max(dim=-1, keepdim=True)[0]
    e = torch.where(keep, torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))), torch.zeros_like(s))
    z = e.sum(dim=-1, keepdim=True)
    return torch.where(z > 0, e / torch.where(z > 0, z, torch.ones_like(z)), torch.zeros_like(e))


def mhla_probs(qkv, B, L, H, hd, W, mask=None):
    """float64 [B, H, L, W]: softmax over the W slots of q_i . k~[idx[i, w]] / sqrt(hd), by explicit gather.
    mask: [B, L, L], non-zero keeps key j for row i."""
    q, k, _ = _split_qk(qkv, B, L, H, hd)
    idx = torch.from_numpy(O.window_indices(L, W))                       # [L, W]
    kw = k[:, :, idx, :]                                                 # [B, H, L, W, hd]
    s = (q[:, :, :, None, :] * kw).sum(-1) / (hd ** 0.5)
    keep = None
    if mask is not None:
        keep = (mask.cpu() != 0)[:, torch.arange(L)[:, None], idx][:, None]          # [B, 1, L, W]
    return _masked_softmax(s, keep)


def dense_probs(qkv, B, L, H, hd, key_keep=None, scale=None):
    """float64 [B, H, L, L]: softmax(scale q k^T); key_keep [B, L], 0 masks the key."""
    q, k, _ = _split_qk(qkv, B, L, H, hd)
    s = (q @ k.transpose(-2, -1)) * (hd ** -0.5 if scale is None else scale)
    keep = None if key_keep is None else (key_keep.cpu() != 0)[:, None, None, :]
    return _masked_softmax(s, keep)


def per_key(P, W):
    """[..., L, L] from slot form [..., L, W]: a key's weight is the sum of its slots."""
    L = P.shape[-2]
    idx = torch.from_numpy(O.window_indices(L, W))
    out = torch.zeros(P.shape[:-1] + (L,), dtype=P.dtype)
    return out.scatter_add_(-1, idx.expand(P.shape), P)


def rollout(probs, widths, cls_row=0, residual=0.5):
    """float64 [B, L].  probs[k]: [B, L, W_k] (widths[k] = W_k) or [B, L, L] (widths[k] = 0), in block order.
    r = e_cls_row; for k = n-1 .. 0: r'[j] = residual r[j] + (1 - residual) sum_i r[i] P_k[i -> j], the banded sum as
    the double loop over (i, w) that scatters r[i] * P[i, w] onto idx[i, w]."""
    B, L = probs[0].shape[:2]
    r = np.zeros((B, L))
    r[:, cls_row] = 1.0
    for P, W in reversed(list(zip(probs, widths))):
        P = P.detach().cpu().to(torch.float64).numpy()
        acc = np.zeros((B, L))
        if W == 0:
            for b in range(B):
                acc[b] = r[b] @ P[b]
        else:
            idx = O.window_indices(L, W)
            for w in range(W):                   # (np.add.at is the loop over i: unbuffered, so repeated keys add up)
                np.add.at(acc, (slice(None), idx[:, w]), r * P[:, :, w])
        r = residual * r + (1.0 - residual) * acc
    return torch.from_numpy(r)


def _f64(sd):
    return {k: v.detach().cpu().to(torch.float64) for k, v in sd.items()}


def _mhla_block(x, sd, p, H, W):
    """One vit_mhla.TransformerBlock with use_mhla=True in float64 -> (x_out, P [B, H, L, W])."""
    B, L, D = x.shape
    hd = D // H
    xn = O.layer_norm(x, sd[f"{p}norm1.weight"], sd[f"{p}norm1.bias"])
    a = f"{p}attn."
    qkv = O.linear(xn, sd[f"{a}qkv.weight"], sd[f"{a}qkv.bias"]).reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    q = qkv[0]
    k = O.linear(qkv[1], sd[f"{a}latent_proj.weight"], sd[f"{a}latent_proj.bias"])
    v = O.linear(qkv[2], sd[f"{a}latent_proj.weight"], sd[f"{a}latent_proj.bias"])
    idx = torch.from_numpy(O.window_indices(L, W))
    s = (q[:, :, :, None, :] * k[:, :, idx, :]).sum(-1) / (hd ** 0.5)
    P = torch.softmax(s, dim=-1)
    o = (P[..., None] * v[:, :, idx, :]).sum(3).transpose(1, 2).reshape(B, L, D)
    x = x + O.linear(o, sd[f"{a}proj.weight"], sd[f"{a}proj.bias"])
    return x + O.mlp(O.layer_norm(x, sd[f"{p}norm2.weight"], sd[f"{p}norm2.bias"]), sd, f"{p}mlp."), P


def _dense_block(x, sd, p, H, torch_mha):
    """A block with dense self-attention (nn.MultiheadAttention names, or vit.MultiHeadAttention's) -> (x_out, P)."""
    B, L, D = x.shape
    hd = D // H
    xn = O.layer_norm(x, sd[f"{p}norm1.weight"], sd[f"{p}norm1.bias"])
    a = f"{p}attn."
    wi, bi, wo, bo = ((f"{a}in_proj_weight", f"{a}in_proj_bias", f"{a}out_proj.weight", f"{a}out_proj.bias") if torch_mha
                      else (f"{a}qkv.weight", f"{a}qkv.bias", f"{a}proj.weight", f"{a}proj.bias"))
    qkv = O.linear(xn, sd[wi], sd[bi]).reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    P = torch.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * (hd ** -0.5), dim=-1)
    o = (P @ qkv[2]).transpose(1, 2).reshape(B, L, D)
    x = x + O.linear(o, sd[wo], sd[bo])
    return x + O.mlp(O.layer_norm(x, sd[f"{p}norm2.weight"], sd[f"{p}norm2.bias"]), sd, f"{p}mlp."), P


def model_maps(kind, x, sd, P, H, W=7, segmaps=None, S=16, residual=0.5):
    """A whole model in float64 that keeps every block's probabilities.  kind: "vit" (VisionTransformer),
    "vit_mhla" / "vit_mhla_dense" (VisionTransformerMHLA with use_mhla True / False), "sppp_mhla" (SPPPViTMHLA with
    use_mhla=True on the label maps `segmaps`).  Returns a dict: logits [B, C], layers (head-mean maps), window,
    rollout [B, L], cls_attention [B, L]."""
    sd = _f64(sd)
    x = x.detach().cpu().to(torch.float64)
    B = x.shape[0]
    emb = O.patch_embed(x, sd, "patch_embed.", P)
    if kind == "sppp_mhla":
        img = x.shape[-1]
        pooled = torch.stack([O.pool(emb[b], O.map_patches(segmaps[b], img, P), "mean") for b in range(B)])
        t = torch.cat((sd["cls_token"].expand(B, -1, -1), pooled), dim=1)
        t = O.dynamic_posenc(t, O.superpixel_centroids(segmaps, S).to(torch.float64))
    else:
        t = torch.cat((sd["cls_token"].expand(B, -1, -1), emb), dim=1) + sd["pos_embed"]
    layers, window = [], []
    for i in range(O._depth(sd)):
        p = f"blocks.{i}."
        if kind in ("vit_mhla", "sppp_mhla"):
            t, Pk = _mhla_block(t, sd, p, H, W)
            window.append(W)
        else:
            t, Pk = _dense_block(t, sd, p, H, torch_mha=(kind == "vit_mhla_dense"))
            window.append(0)
        layers.append(Pk.mean(dim=1))
    logits = O.linear(O.layer_norm(t, sd["norm.weight"], sd["norm.bias"])[:, 0], sd["head.weight"], sd["head.bias"])
    last = layers[-1] if window[-1] == 0 else per_key(layers[-1], window[-1])
    return {"logits": logits, "layers": layers, "window": window, "rollout": rollout(layers, window, 0, residual),
            "cls_attention": last[:, 0, :]}
