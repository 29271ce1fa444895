"""Source models and key layouts for the checkpoint-import tests, written from the public key names of torchvision's
VisionTransformer, timm's VisionTransformer and Hugging Face's ViTForImageClassification (none of the three packages
is needed): a small float64 torchvision-layout ViT in plain torch, and functions that respell its state dict in the
other layouts."""
from collections import OrderedDict

import torch
import torch.nn as nn

D, C, P, H, DEPTH, IMG, CLASSES = 32, 3, 4, 4, 2, 16, 5


class _Block(nn.Module):
    def __init__(self, d, heads, old_mlp_names):
        super().__init__()
        self.ln_1 = nn.LayerNorm(d, eps=1e-5)
        self.self_attention = nn.MultiheadAttention(d, heads, batch_first=True)
        self.ln_2 = nn.LayerNorm(d, eps=1e-5)
        if old_mlp_names:
            self.mlp = nn.Sequential(OrderedDict(linear_1=nn.Linear(d, 4 * d), act=nn.GELU(), linear_2=nn.Linear(4 * d, d)))
        else:
            self.mlp = nn.Sequential(nn.Linear(d, 4 * d), nn.GELU(), nn.Dropout(0.0), nn.Linear(4 * d, d), nn.Dropout(0.0))

    def forward(self, x):
        y = self.ln_1(x)
        x = x + self.self_attention(y, y, y, need_weights=False)[0]
        return x + self.mlp(self.ln_2(x))


class _Encoder(nn.Module):
    def __init__(self, rows, d, heads, depth, old_mlp_names):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.randn(1, rows, d) * 0.5)
        self.layers = nn.Sequential(OrderedDict((f"encoder_layer_{i}", _Block(d, heads, old_mlp_names)) for i in range(depth)))
        self.ln = nn.LayerNorm(d, eps=1e-5)

    def forward(self, x):
        return self.ln(self.layers(x + self.pos_embedding))


class TorchvisionLayoutViT(nn.Module):
    """Conv2d patches, nn.MultiheadAttention, exact GELU, eps 1e-5, under torchvision's attribute names."""

    def __init__(self, img=IMG, patch=P, d=D, heads=H, depth=DEPTH, classes=CLASSES, channels=C, old_mlp_names=False):
        super().__init__()
        self.class_token = nn.Parameter(torch.randn(1, 1, d) * 0.5)
        self.conv_proj = nn.Conv2d(channels, d, kernel_size=patch, stride=patch)
        self.encoder = _Encoder((img // patch) ** 2 + 1, d, heads, depth, old_mlp_names)
        self.heads = nn.Sequential(OrderedDict(head=nn.Linear(d, classes)))

    def forward(self, x):
        t = self.conv_proj(x).flatten(2).transpose(1, 2)
        t = torch.cat((self.class_token.expand(t.shape[0], -1, -1), t), dim=1)
        return self.heads(self.encoder(t)[:, 0])


def source_model(seed=0, **kw):
    """A float64 instance with random (not default-initialised) weights everywhere, biases and norms included."""
    torch.manual_seed(seed)
    m = TorchvisionLayoutViT(**kw).double().eval()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() > 1 else 0.5) + (1.0 if p.dim() == 1 else 0.0))
    return m


_TIMM_BLOCK = {"ln_1": "norm1", "self_attention.in_proj_weight": "attn.qkv.weight", "self_attention.in_proj_bias": "attn.qkv.bias",
               "self_attention.out_proj": "attn.proj", "ln_2": "norm2", "mlp.0": "mlp.fc1", "mlp.3": "mlp.fc2"}
_TIMM_TOP = {"class_token": "cls_token", "encoder.pos_embedding": "pos_embed", "conv_proj": "patch_embed.proj",
             "encoder.ln": "norm", "heads.head": "head"}


def _respell(sd, top, block, block_prefix):
    out = OrderedDict()
    for k, v in sd.items():
        if k.startswith("encoder.layers.encoder_layer_"):
            i, rest = k[len("encoder.layers.encoder_layer_"):].split(".", 1)
            for old, new in block.items():
                if rest == old or rest.startswith(old + "."):
                    out[f"{block_prefix}{i}.{new}{rest[len(old):]}"] = v
                    break
            else:
                raise KeyError(k)
        else:
            for old, new in top.items():
                if k == old or k.startswith(old + "."):
                    out[new + k[len(old):]] = v
                    break
            else:
                raise KeyError(k)
    return out


def as_timm(sd):
    return _respell(sd, _TIMM_TOP, _TIMM_BLOCK, "blocks.")


def as_hf(sd, in_memory, prefix="vit."):
    """Hugging Face's two spellings: as written to files (in_memory=False) or as transformers >= 5 holds it."""
    d = sd[next(k for k in sd if k.endswith("in_proj_bias"))].shape[0] // 3
    if in_memory:
        blk = {"ln_1": "layernorm_before", "self_attention.out_proj": "attention.o_proj", "ln_2": "layernorm_after",
               "mlp.0": "mlp.fc1", "mlp.3": "mlp.fc2"}
        qkv, bp = ("attention.q_proj", "attention.k_proj", "attention.v_proj"), "layers."
    else:
        blk = {"ln_1": "layernorm_before", "self_attention.out_proj": "attention.output.dense", "ln_2": "layernorm_after",
               "mlp.0": "intermediate.dense", "mlp.3": "output.dense"}
        qkv, bp = ("attention.attention.query", "attention.attention.key", "attention.attention.value"), "encoder.layer."
    top = {"class_token": "embeddings.cls_token", "encoder.pos_embedding": "embeddings.position_embeddings",
           "conv_proj": "embeddings.patch_embeddings.projection", "encoder.ln": "layernorm"}
    out = OrderedDict()
    for k, v in sd.items():
        if k.startswith("heads.head."):
            out["classifier." + k[len("heads.head."):]] = v
        elif "in_proj_" in k:
            i = k[len("encoder.layers.encoder_layer_"):].split(".", 1)[0]
            leaf = k.rsplit("_", 1)[1]
            for j, name in enumerate(qkv):
                out[f"{prefix}{bp}{i}.{name}.{leaf}"] = v[j * d:(j + 1) * d].clone()
        else:
            (nk, nv), = _respell({k: v}, top, blk, bp).items()
            out[prefix + nk] = nv
    return out
