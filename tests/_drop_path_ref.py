"""Host side of the stochastic depth (DropPath) tests: the per-sample draw, the seeds a forward draws, and a float64
encoder with an explicit per-sample scale on every residual branch.

The draw is the library's dropout draw (tests/_dropout_ref.py restates it) with the SAMPLE number as its index, and
functional.EncoderOp documents which seeds a forward takes from torch's CPU generator and in which order, so a test
can rebuild every mask of a training forward on the host and run plain float64 autograd with them.

numpy / torch only; runs on the CPU.  tests/test_drop_path_host.py checks expected_seeds against functional._seed."""
import numpy as np
import torch

from oracle import favit_oracle as O

from _dropout_ref import keep_mask, keep_scale


def sample_keep(seed, B, p):
    """Which of the B samples keep a residual branch drawn with (seed, p): favit_keep(seed, b, threshold(p))."""
    return keep_mask(seed, B, p)


def sample_scale(seed, B, p):
    """float64 [B]: keep(b) / (1 - p), with 1 / (1 - p) as the kernels compute it (fp32); ones where p == 0."""
    if p <= 0:
        return torch.ones(B, dtype=torch.float64)
    return torch.from_numpy(sample_keep(seed, B, p).astype(np.float64)) * keep_scale(p)


def expected_seeds(torch_seed, n):
    """The first n values functional._seed() returns after torch.manual_seed(torch_seed).  Re-seeds torch."""
    torch.manual_seed(torch_seed)
    return [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(n)]


def linear_rates(rate, depth):
    """timm's linear rule: block i of depth gets rate * i / max(1, depth - 1)."""
    return [rate * i / max(1, depth - 1) for i in range(depth)]


def element_keep(seed, M, N, p):
    """float64 [M, N]: the element dropout factor keep / (1 - p) of a GEMM epilogue, element index m * N + n."""
    return torch.from_numpy(keep_mask(seed, M * N, p).reshape(M, N).astype(np.float64)) * keep_scale(p)


def block_forward(x, sd, p, H, kind, scale_a, scale_m, W=7, mlp_drop=None):
    """One pre-LN block in the dtype of x with a [B] scale on each residual branch.
    kind: "mhla" (vit_mhla.TransformerBlock, use_mhla) or "dense" (vit.TransformerBlock).
    mlp_drop = (d1 [B*L, hidden], d2 [B*L, D]): the element dropout factors behind GELU and behind fc2, or None."""
    B, L, D = x.shape
    xn = O.layer_norm(x, sd[f"{p}norm1.weight"], sd[f"{p}norm1.bias"])
    a = O.mhla_attention(xn, sd, f"{p}attn.", H, W) if kind == "mhla" else O.dense_mha(xn, sd, f"{p}attn.", H)
    x = x + a * scale_a.to(x.dtype)[:, None, None]
    xn = O.layer_norm(x, sd[f"{p}norm2.weight"], sd[f"{p}norm2.bias"])
    if mlp_drop is None:
        m = O.mlp(xn, sd, f"{p}mlp.")
    else:
        d1, d2 = mlp_drop
        h = O.gelu(O.linear(xn, sd[f"{p}mlp.fc1.weight"], sd[f"{p}mlp.fc1.bias"])) * d1.reshape(B, L, -1).to(x.dtype)
        m = O.linear(h, sd[f"{p}mlp.fc2.weight"], sd[f"{p}mlp.fc2.bias"]) * d2.reshape(B, L, D).to(x.dtype)
    return x + m * scale_m.to(x.dtype)[:, None, None]


def model_forward(x, sd, P, H, kind, scales, W=7, mlp_drops=None):
    """VisionTransformer(MHLA).forward (oracle.favit_oracle.vit_forward / vit_mhla_forward) with scales[i] =
    (scale_a [B], scale_m [B]) for block i and mlp_drops[i] as in block_forward.  Returns the logits."""
    B = x.shape[0]
    t = O.patch_embed(x, sd, "patch_embed.", P)
    t = torch.cat((sd["cls_token"].expand(B, -1, -1), t), dim=1) + sd["pos_embed"]
    for i, (sa, sm) in enumerate(scales):
        t = block_forward(t, sd, f"blocks.{i}.", H, kind, sa, sm, W, None if mlp_drops is None else mlp_drops[i])
    t = O.layer_norm(t, sd["norm.weight"], sd["norm.bias"])[:, 0]
    return O.linear(t, sd["head.weight"], sd["head.bias"])


def reference(model, x, y, P, H, kind, scales, W=7, mlp_drops=None):
    """float64 logits and parameter gradients of mean cross-entropy under the explicit masks.
    Returns (logits [B, C] float64, {name: gradient float64})."""
    sd = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    logits = model_forward(x.detach().cpu().double(), sd, P, H, kind, scales, W, mlp_drops)
    O.cross_entropy(logits, y.cpu()).backward()
    return logits.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
