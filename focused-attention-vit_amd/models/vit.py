"""Mirror of the reference's models/vit.py (PatchEmbedding, MultiHeadAttention, MLP,
TransformerBlock, VisionTransformer): identical constructors, forward signatures,
attribute names, state_dict keys and weight-init RNG order; the math runs in the HIP
kernels of libfavit (no aten compute ops on the path)."""
import torch
import torch.nn as nn

from ._backend import F, params


class PatchRearrange(nn.Module):
    """Parameter-free placeholder for einops' Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)')
    at index 0 of ``PatchEmbedding.projection`` (reference models/vit.py:38-39); the gather is
    fused into favit_patchify_fwd."""

    def __init__(self, patch_size):
        super().__init__()
        self.patch_size = patch_size

    def extra_repr(self):
        return f"'b c (h p1) (w p2) -> b (h w) (p1 p2 c)', p1=p2={self.patch_size}"

    def forward(self, x):  # pragma: no cover - the fused path never calls this
        raise RuntimeError("PatchRearrange is fused into PatchEmbedding.forward")


class PatchEmbedding(nn.Module):
    """reference models/vit.py:19-53"""

    def __init__(self, img_size=224, patch_size=16, in_channels=3, embed_dim=768):
        super().__init__()
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = (img_size // patch_size) ** 2
        self.projection = nn.Sequential(
            PatchRearrange(patch_size),
            nn.Linear(patch_size * patch_size * in_channels, embed_dim),
        )

    def forward(self, x):
        lin = self.projection[1]
        return F.run(F.PatchEmbedOp(self.patch_size), [x], [lin.weight, lin.bias])


class MultiHeadAttention(nn.Module):
    """Dense multi-head self-attention, reference models/vit.py:56-104."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.qkv = nn.Linear(embed_dim, embed_dim * 3)
        self.attn_dropout = nn.Dropout(dropout)
        self.proj = nn.Linear(embed_dim, embed_dim)
        self.proj_dropout = nn.Dropout(dropout)

    def _chain(self):
        return F.DenseChain(self.num_heads, self.attn_dropout.p, self.proj_dropout.p)

    def forward(self, x):
        ch = self._chain()
        return F.run(F.AttnOp(ch, None, self.training), [x], params(self, ch.names))


class MLP(nn.Module):
    """reference models/vit.py:107-139"""

    def __init__(self, in_features, hidden_features, out_features, dropout=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.dropout = nn.Dropout(dropout)

    def _chain(self):
        return F.MLPChain(self.dropout.p)

    def forward(self, x):
        ch = self._chain()
        return F.run(F.MLPOp(ch, self.training), [x], params(self, ch.names))


class TransformerBlock(nn.Module):
    """Pre-LN encoder block, reference models/vit.py:142-179."""

    def __init__(self, embed_dim, num_heads, mlp_ratio=4.0, dropout=0.0, attn_dropout=0.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(embed_dim)
        self.attn = MultiHeadAttention(embed_dim, num_heads, attn_dropout)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.mlp = MLP(in_features=embed_dim, hidden_features=int(embed_dim * mlp_ratio), out_features=embed_dim,
                       dropout=dropout)
        self.drop_path = 0.0                   # stochastic depth rate of both residual branches (set_drop_path_rate)

    def _spec(self):
        return F.BlockSpec(self.attn._chain(), self.mlp._chain(), drop_path=self.drop_path)

    def forward(self, x):
        spec = self._spec()
        return F.run(F.EncoderOp([spec], None, self.training), [x], params(self, spec.names))


def drop_path_rates(drop_path_rate: float, depth: int):
    """Stochastic depth rates of a stack of `depth` blocks, timm's linear rule: block i gets
    drop_path_rate * i / max(1, depth - 1), so block 0 gets 0 and the last block the full rate."""
    return [float(drop_path_rate) * i / max(1, depth - 1) for i in range(depth)]


def set_drop_path_rate(model, drop_path_rate: float = 0.0):
    """Stochastic depth (DropPath) for a model that owns a block stack (`model.blocks`): in training mode, block i
    drops each of its two residual branches per sample with probability drop_path_rates(...)[i] and scales the
    survivors by 1 / (1 - p) (functional.EncoderOp).  The rate is a plain float attribute `drop_path` of every block,
    read by its _spec(): no parameter, no buffer, no state_dict key.  It is set here and not by a constructor keyword
    because the constructors mirror the reference's signatures exactly.  Every model class with a block stack has this
    function as a method; returns the model, so `Model(...).set_drop_path_rate(0.1)` reads as one expression."""
    if not 0.0 <= float(drop_path_rate) < 1.0:
        raise ValueError("drop_path_rate must lie in [0, 1)")
    blocks = list(model.blocks)
    for blk, p in zip(blocks, drop_path_rates(drop_path_rate, len(blocks))):
        blk.drop_path = p
    model.drop_path_rate = float(drop_path_rate)
    return model


def set_pos_antialias(model, antialias: bool = True):
    """How a model with a learned grid `pos_embed` resamples it when the input's patch grid is not the parameter's
    (functional.PrologueOp): antialiased bicubic (True, the default, timm's rule) or torch's plain bicubic (False).
    A plain attribute `pos_antialias`, handled like drop_path: no parameter, no buffer, no state_dict key.  Returns
    the model."""
    model.pos_antialias = bool(antialias)
    return model


def set_global_pool(model, pool: str = "token", norm: str = "before"):
    """What the classification head of a model that ends in `norm` + `head` reads: the CLS row ("token", the default and
    the reference's rule: functional.FinalNormOp) or the mean over the other token rows ("avg", timm's
    global_pool="avg": functional.HeadPoolOp).  With "avg", `norm` says where the final LayerNorm sits: "before" the
    mean (the model's `norm` on every token) or "after" it (timm's fc_norm, which checkpoints trained that way carry;
    pretrained.Report's pool_hint tells).  The mean reads every row, so a windowed MHLA encoder then runs all its rows
    instead of the few the CLS row can see.  Plain attributes `global_pool` / `pool_norm`, handled like drop_path: no
    parameter, no buffer, no state_dict key.  Returns the model."""
    if pool not in ("token", "avg"):
        raise ValueError(f"global pool must be 'token' or 'avg', got {pool!r}")
    if norm not in ("before", "after"):
        raise ValueError(f"pool norm must be 'before' or 'after', got {norm!r}")
    model.global_pool, model.pool_norm = pool, norm
    return model


def run_encoder(blocks, x, mask, training, cls_only=False):
    """All blocks of a model as ONE autograd node (no per-block fp32<->bf16 gradient casts) -- or, while
    functional.encoder_segments(n) is active (train.GraphedStep with backward segments), as n consecutive nodes cut
    apart at detached boundary tensors, so that backward can be run, and captured, segment by segment.
    cls_only: the caller reads nothing but row 0 of the result (FinalNormOp).  Where functional.cls_only_cuts allows
    it, every block then computes only the token rows that row can see, and the result is [B, n, D] with the last
    block's n rows (row 0 first) instead of [B, L, D]."""
    blocks = list(blocks)
    nseg = max(1, min(F.get_encoder_segments(), len(blocks)))
    m = F._mask_u8(mask)
    per = (len(blocks) + nseg - 1) // nseg
    all_specs = [b._spec() for b in blocks]
    cuts = F.cls_only_cuts(all_specs, x.shape[1], m, training) if cls_only else None
    for i in range(0, len(blocks), per):
        grp = blocks[i:i + per]
        specs = all_specs[i:i + per]
        prm = []
        for b, s in zip(grp, specs):
            prm += params(b, s.names)
        if i:
            x = F.note_segment_boundary(x)        # the next node starts a fresh autograd graph at a leaf copy of x
        seg = mseg = None
        if cuts is not None:
            seg = cuts[i:i + per]
            if F.mlp_narrow_on():
                # each block's MLP half runs on the rows the next block reads; the node's last block learns them here
                mseg = F.mlp_narrow_plan(seg, after=cuts[i + per] if i + per < len(cuts) else None)
        x = F.run(F.EncoderOp(specs, m, training, cuts=seg, mlp_cuts=mseg), [x], prm)
    return x


def embed_dropout(x, p, training):
    if not training or p <= 0.0:
        return x
    return F.run(F.DropoutOp(p), [x], [])


class VisionTransformer(nn.Module):
    """reference models/vit.py:182-331"""

    def __init__(self, img_size=224, patch_size=4, in_channels=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4.0, dropout=0.0, attn_dropout=0.0, embed_dropout=0.0):
        super().__init__()
        self.img_size = img_size
        self.patch_size = patch_size
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.embed_dim = embed_dim
        self.depth = depth
        self.num_heads = num_heads
        self.patch_embed = PatchEmbedding(img_size=img_size, patch_size=patch_size, in_channels=in_channels,
                                          embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.pos_antialias = True              # resampling rule at another input resolution (set_pos_antialias)
        self.pos_drop = nn.Dropout(embed_dropout)
        self.blocks = nn.ModuleList([
            TransformerBlock(embed_dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, dropout=dropout,
                             attn_dropout=attn_dropout) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes)
        self._init_weights()

    def _init_weights(self):
        nn.init.normal_(self.cls_token, std=0.02)
        nn.init.normal_(self.pos_embed, std=0.02)
        self.apply(self._init_weights_recursive)

    def _init_weights_recursive(self, m):
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    def forward_features(self, x):
        tok = self.patch_embed(x)
        x = F.run(F.PrologueOp(True, self.pos_antialias), [tok], [self.cls_token, self.pos_embed])
        x = embed_dropout(x, self.pos_drop.p, self.training)
        x = run_encoder(self.blocks, x, None, self.training)
        if self.global_pool == "avg":
            return F.run(F.HeadPoolOp(self.pool_norm == "before"), [x], [self.norm.weight, self.norm.bias])
        return F.run(F.FinalNormOp(), [x], [self.norm.weight, self.norm.bias])

    def forward(self, x):
        x = self.forward_features(x)
        return F.run(F.LinearOp(), [x], [self.head.weight, self.head.bias])

    def get_num_parameters(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    set_drop_path_rate = set_drop_path_rate
    set_pos_antialias = set_pos_antialias
    global_pool, pool_norm = "token", "before"     # what the head reads (set_global_pool)
    set_global_pool = set_global_pool
