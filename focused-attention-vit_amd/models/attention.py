"""Mirror of the reference's models/attention.py (CrossAttention, MultiHeadCrossAttention,
CrossAttentionTransformerBlock, CrossAttentionViT, CrossAttentionSPPPViT)."""
from typing import Optional

import torch
import torch.nn as nn

from ._backend import F, params
from .vit import embed_dropout, set_global_pool


class CrossAttention(nn.Module):
    """Single-head cross-attention, scores / embed_dim**0.5 (reference models/attention.py:17-78)."""

    def __init__(self, embed_dim: int, dropout: float = 0.0):
        super().__init__()
        self.embed_dim = embed_dim
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        self.dropout = nn.Dropout(dropout)

    def _chain(self):
        return F.CrossChain(1, self.dropout.p)

    def forward(self, query: torch.Tensor, key_value: torch.Tensor,
                attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        ch = self._chain()
        return F.run(F.CrossAttnOp(ch, F._mask_u8(attention_mask), self.training), [query, key_value],
                     params(self, ch.names))


class MultiHeadCrossAttention(nn.Module):
    """reference models/attention.py:81-148"""

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        self.dropout = nn.Dropout(dropout)

    def _chain(self):
        return F.CrossChain(self.num_heads, self.dropout.p)

    def forward(self, query: torch.Tensor, key_value: torch.Tensor,
                attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        ch = self._chain()
        return F.run(F.CrossAttnOp(ch, F._mask_u8(attention_mask), self.training), [query, key_value],
                     params(self, ch.names))


class CrossAttentionTransformerBlock(nn.Module):
    """reference models/attention.py:151-219"""

    def __init__(self, embed_dim: int, num_heads: int, mlp_ratio: float = 4.0, dropout: float = 0.0,
                 attn_dropout: float = 0.0, use_multi_head: bool = False):
        super().__init__()
        self.norm1_query = nn.LayerNorm(embed_dim)
        self.norm1_kv = nn.LayerNorm(embed_dim)
        if use_multi_head:
            self.attn = MultiHeadCrossAttention(embed_dim, num_heads, attn_dropout)
        else:
            self.attn = CrossAttention(embed_dim, attn_dropout)
        self.norm2 = nn.LayerNorm(embed_dim)
        mlp_hidden_dim = int(embed_dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(embed_dim, mlp_hidden_dim), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(mlp_hidden_dim, embed_dim), nn.Dropout(dropout))

    def _op(self, mask):
        return F.CrossBlockOp(self.attn._chain(), F.MLPChain(self.mlp[2].p, "0", "3"), F._mask_u8(mask), self.training)

    def forward(self, query: torch.Tensor, key_value: torch.Tensor,
                attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        op = self._op(attention_mask)
        return F.run(op, [query, key_value], params(self, op.names))


class _ConvPatchEmbed(nn.Module):
    """The reference builds ``nn.Sequential(Conv2d, Flatten(2), nn.Transpose(1, 2))`` and crashes
    on ``nn.Transpose`` (models/attention.py:275,454).  Evident intent: a stride-P conv patch
    embedding -> [B, N, D].  A stride-P, kernel-P conv IS a patch-row GEMM, so the Conv2d weight
    [D, C, P, P] (kept under the reference's key ``patch_embed.0.*``) is fed to the same
    patchify + GEMM kernels with its (c, p1, p2) axes permuted to the kernels' (p1, p2, c) order."""

    def __init__(self, in_channels, embed_dim, patch_size):
        super().__init__()
        self.add_module("0", nn.Conv2d(in_channels, embed_dim, kernel_size=patch_size, stride=patch_size))
        self.patch_size = patch_size

    def forward(self, x):
        conv = getattr(self, "0")
        D = conv.weight.shape[0]
        w = conv.weight.permute(0, 2, 3, 1).reshape(D, -1)     # [D, P*P*C], c fastest (view/copy only)
        return F.run(F.PatchEmbedOp(self.patch_size), [x], [w, conv.bias])


class CrossAttentionViT(nn.Module):
    """reference models/attention.py:222-380 (its constructor raises on nn.Transpose; this keeps the
    signature and implements the evident intent; forward calls block(x, x), attention.py:350)."""

    def __init__(self, img_size: int = 224, patch_size: int = 16, in_channels: int = 3, num_classes: int = 1000,
                 embed_dim: int = 768, depth: int = 12, num_heads: int = 12, mlp_ratio: float = 4.0,
                 dropout: float = 0.0, attn_dropout: float = 0.0, embed_dropout: float = 0.0,
                 use_multi_head: bool = False):
        super().__init__()
        self.img_size = img_size
        self.patch_size = patch_size
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.embed_dim = embed_dim
        self.depth = depth
        self.num_heads = num_heads
        self.use_multi_head = use_multi_head
        self.num_patches = (img_size // patch_size) ** 2
        self.patch_embed = _ConvPatchEmbed(in_channels, embed_dim, patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches + 1, embed_dim))
        self.pos_drop = nn.Dropout(embed_dropout)
        self.blocks = nn.ModuleList([
            CrossAttentionTransformerBlock(embed_dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                           dropout=dropout, attn_dropout=attn_dropout,
                                           use_multi_head=use_multi_head) for _ in range(depth)])
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

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        tok = self.patch_embed(x)
        x = F.run(F.PrologueOp(True), [tok], [self.cls_token, self.pos_embed])
        x = embed_dropout(x, self.pos_drop.p, self.training)
        for block in self.blocks:
            x = block(x, x)
        if self.global_pool == "avg":
            return F.run(F.HeadPoolOp(self.pool_norm == "before"), [x], [self.norm.weight, self.norm.bias])
        return F.run(F.FinalNormOp(), [x], [self.norm.weight, self.norm.bias])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.forward_features(x)
        return F.run(F.LinearOp(), [x], [self.head.weight, self.head.bias])

    def get_num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    global_pool, pool_norm = "token", "before"     # what the head reads (set_global_pool)
    set_global_pool = set_global_pool


class CrossAttentionSPPPViT(nn.Module):
    """reference models/attention.py:383-609 (constructor raises on nn.Transpose there; evident
    intent implemented: SPPP front end + cross-attention blocks called as block(x, x))."""

    def __init__(self, img_size: int = 224, patch_size: int = 16, in_channels: int = 3, num_classes: int = 1000,
                 embed_dim: int = 768, depth: int = 12, num_heads: int = 12, mlp_ratio: float = 4.0,
                 dropout: float = 0.0, attn_dropout: float = 0.0, embed_dropout: float = 0.0,
                 num_superpixels: int = 16, compactness: float = 0.1, pooling_type: str = 'mean',
                 use_multi_head: bool = False):
        super().__init__()
        from .sppp import (SuperpixelSegmentation, PatchToSuperpixelMapper, SuperpixelPooling,
                           DynamicPositionalEncoding)
        self.img_size = img_size
        self.patch_size = patch_size
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.embed_dim = embed_dim
        self.depth = depth
        self.num_heads = num_heads
        self.num_superpixels = num_superpixels
        self.use_multi_head = use_multi_head
        self.segmentation = SuperpixelSegmentation(num_segments=num_superpixels, compactness=compactness)
        self.patch_mapper = PatchToSuperpixelMapper(patch_size=patch_size)
        self.pooling = SuperpixelPooling(pooling_type=pooling_type)
        self.patch_embed = _ConvPatchEmbed(in_channels, embed_dim, patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = DynamicPositionalEncoding(embed_dim, embed_dropout)
        self.blocks = nn.ModuleList([
            CrossAttentionTransformerBlock(embed_dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                           dropout=dropout, attn_dropout=attn_dropout,
                                           use_multi_head=use_multi_head) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes)
        self.assume_num_tokens = None
        nn.init.normal_(self.cls_token, std=0.02)
        self.apply(self._init_weights_recursive)

    _init_weights_recursive = CrossAttentionViT._init_weights_recursive

    def _calculate_superpixel_centroids(self, segmentation_maps):
        from .sppp import calculate_superpixel_centroids
        return calculate_superpixel_centroids(self, segmentation_maps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from .sppp import sppp_tokens
        t = sppp_tokens(self, x)
        for block in self.blocks:
            t = block(t, t)
        if self.global_pool == "avg":
            t = F.run(F.HeadPoolOp(self.pool_norm == "before"), [t], [self.norm.weight, self.norm.bias])
        else:
            t = F.run(F.FinalNormOp(), [t], [self.norm.weight, self.norm.bias])
        return F.run(F.LinearOp(), [t], [self.head.weight, self.head.bias])

    def get_num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    global_pool, pool_norm = "token", "before"     # what the head reads (set_global_pool)
    set_global_pool = set_global_pool
