"""Import of standard ViT checkpoints: torchvision, timm and Hugging Face key layouts mapped onto this package's
models, from files the user already has (nothing is ever fetched).

    report = pretrained.load_pretrained(model, "vit_b_16.pth")          # or an HF directory, .safetensors, .npz, a dict
    print(report.summary())

What the mapping does (convert_state_dict): renames the keys; turns a convolutional patch weight [D, C, P, P] into the
Linear over (p1 p2 c) that favit_patchify_fwd feeds (w.permute(0, 2, 3, 1).reshape(D, P*P*C)); concatenates separate q, k
and v in that order; writes the attention under the names the model owns (attn.qkv / attn.proj, or the in_proj_* /
out_proj.* of an nn.MultiheadAttention container) and the MLP under fc1 / fc2 or the 0 / 3 of an nn.Sequential.
latent_proj has no source and stays as it is.  timm's avg-pooled checkpoints carry fc_norm.* in place of norm.*: it
becomes the model's norm, and the report's pool_hint says how such a model pools (nothing here changes the model's
pooling: models.vit.set_global_pool does).  A head of another shape is skipped (the reference re-initialises it);
another patch size, width or depth is an error.  A pos_embed on another grid is resampled on the device
(functional.pos_resample) by load_pretrained, or refused with pos_embed="strict".

The models keep the reference's LayerNorm eps = 1e-5; torchvision and timm train with 1e-6 and Hugging Face's default
is 1e-12.  The report carries the source's value where a config.json states it; no code changes eps.
"""
from __future__ import annotations

import json
import math
import os
import re
from typing import Dict, Optional, Tuple

import numpy as np
import torch

__all__ = ["convert_state_dict", "load_pretrained", "read_state_dict", "detect_layout", "Report"]

_BLOCK = {          # canonical block-level names
    "torchvision": [(r"ln_1", "ln1"), (r"self_attention\.in_proj", "qkv"),
                    (r"self_attention\.out_proj", "proj"), (r"ln_2", "ln2"), (r"mlp\.(?:0|linear_1)", "fc1"),
                    (r"mlp\.(?:3|linear_2)", "fc2")],
    "timm": [(r"norm1", "ln1"), (r"attn\.qkv", "qkv"), (r"attn\.proj", "proj"), (r"norm2", "ln2"),
             (r"mlp\.fc1", "fc1"), (r"mlp\.fc2", "fc2")],
    "hf": [(r"layernorm_before", "ln1"), (r"attention\.attention\.query", "q"), (r"attention\.attention\.key", "k"),
           (r"attention\.attention\.value", "v"), (r"attention\.output\.dense", "proj"), (r"layernorm_after", "ln2"),
           (r"intermediate\.dense", "fc1"), (r"output\.dense", "fc2")],
    "hf5": [(r"layernorm_before", "ln1"), (r"attention\.q_proj", "q"), (r"attention\.k_proj", "k"),
            (r"attention\.v_proj", "v"), (r"attention\.o_proj", "proj"), (r"layernorm_after", "ln2"),
            (r"mlp\.fc1", "fc1"), (r"mlp\.fc2", "fc2")],
}
_BLOCK_PREFIX = {"torchvision": r"encoder\.layers\.encoder_layer_(\d+)\.", "timm": r"blocks\.(\d+)\.",
                 "hf": r"encoder\.layer\.(\d+)\.", "hf5": r"layers\.(\d+)\."}
_TOP = {            # canonical top-level names; a name without a dot is a whole tensor, the others take .weight / .bias
    "torchvision": {"class_token": "cls", "encoder.pos_embedding": "pos", "conv_proj": "patch", "encoder.ln": "norm",
                    "heads.head": "head"},
    "timm": {"cls_token": "cls", "pos_embed": "pos", "patch_embed.proj": "patch", "norm": "norm", "head": "head"},
    "hf": {"embeddings.cls_token": "cls", "embeddings.position_embeddings": "pos",
           "embeddings.patch_embeddings.projection": "patch", "layernorm": "norm", "classifier": "head"},
}
_TOP["hf5"] = _TOP["hf"]


class Report(dict):
    """What a conversion did.  Keys: layout ('native', 'torchvision', 'timm', 'hf' = Hugging Face as written to files,
    'hf5' = Hugging Face as transformers >= 5 holds it in memory), loaded (model keys that received a tensor), skipped
    ({model key: reason}), unused (source keys nothing was made of), missing (model keys without a source), source_grid
    (side of the source pos_embed's grid, or None), model_grid, pos_embed ('copied', 'resampled' or None),
    layer_norm_eps (the source's, from a config.json, or None), pool_hint (('avg', 'after') when the model's norm was
    taken from timm's fc_norm, the LayerNorm behind the token mean: the set_global_pool arguments such a checkpoint was
    trained with; otherwise None)."""

    def summary(self) -> str:
        s = (f"{self['layout']} layout: {len(self['loaded'])} tensors loaded, {len(self['skipped'])} skipped, "
             f"{len(self['unused'])} source keys unused, {len(self['missing'])} model keys without a source")
        if self.get("pos_embed") == "resampled":
            s += f"; pos_embed resampled {self['source_grid']}x{self['source_grid']} -> {self['model_grid']}x{self['model_grid']}"
        for k, why in self["skipped"].items():
            s += f"\n  skipped {k}: {why}"
        if self["missing"]:
            s += "\n  without a source: " + ", ".join(self["missing"][:8]) + (" ..." if len(self["missing"]) > 8 else "")
        if self.get("pool_hint") is not None:
            s += ("\n  norm.* comes from the source's fc_norm: it was trained with set_global_pool"
                  f"{self['pool_hint']!r}; loading leaves the model's pooling as it is")
        if self.get("layer_norm_eps") is not None:
            s += f"\n  the source was trained with LayerNorm eps = {self['layer_norm_eps']:g}; the model computes with 1e-5"
        return s


def _unwrap(obj, what):
    for _ in range(2):
        if isinstance(obj, dict) and len(obj) and not any(torch.is_tensor(v) for v in obj.values()):
            for k in ("state_dict", "model"):
                if isinstance(obj.get(k), dict):
                    obj = obj[k]
                    break
    if not isinstance(obj, dict) or not obj or not all(torch.is_tensor(v) for v in obj.values()):
        raise ValueError(f"{what}: not a state dict (a mapping of names to tensors, possibly under 'state_dict' or 'model')")
    return dict(obj)


def _read_safetensors(path):
    try:
        from safetensors.torch import load_file
    except ImportError as e:
        raise ImportError(f"{path}: reading .safetensors files needs the `safetensors` package, which is not installed; "
                          "convert the file to .pt or .npz, or install the package") from e
    return load_file(path, device="cpu")


def read_state_dict(path: str) -> Tuple[Dict[str, torch.Tensor], Optional[float]]:
    """(state dict on the host, the source's layer_norm_eps or None) of a local file: .pt / .pth / .bin through
    torch.load(weights_only=True), a {'state_dict': ...} or {'model': ...} wrapper removed; .npz without pickle;
    .safetensors; or a Hugging Face directory (its model.safetensors or pytorch_model.bin; config.json only tells
    layer_norm_eps)."""
    path = os.fspath(path)
    eps = None
    if os.path.isdir(path):
        cfg = os.path.join(path, "config.json")
        if os.path.exists(cfg):
            with open(cfg) as f:
                eps = json.load(f).get("layer_norm_eps")
        for name in ("model.safetensors", "pytorch_model.bin"):
            if os.path.exists(os.path.join(path, name)):
                return read_state_dict(os.path.join(path, name))[0], (None if eps is None else float(eps))
        raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin in this directory")
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npz":
        with np.load(path, allow_pickle=False) as arc:
            return {k: torch.from_numpy(arc[k]) for k in arc.files}, None
    if ext == ".safetensors":
        return _read_safetensors(path), None
    if ext in (".pt", ".pth", ".bin"):
        return _unwrap(torch.load(path, map_location="cpu", weights_only=True), path), None
    raise ValueError(f"{path}: unknown checkpoint format {ext!r} (.pt, .pth, .bin, .npz, .safetensors or an HF directory)")


def detect_layout(keys, model_keys=()) -> str:
    """The layout a set of source keys is written in; ValueError when it is none of those this module knows."""
    keys = set(keys)
    if "conv_proj.weight" in keys or "class_token" in keys or any(k.startswith("encoder.layers.encoder_layer_") for k in keys):
        return "torchvision"
    bare = {k[4:] if k.startswith("vit.") else k for k in keys}
    if any(k.startswith("encoder.layer.") for k in bare):
        return "hf"
    if any(k.startswith("layers.") for k in bare):
        return "hf5"
    if any(k.startswith("embeddings.") for k in bare):
        return "hf"
    if "patch_embed.proj.weight" in keys:
        return "timm"
    if keys & set(model_keys):
        return "native"
    raise ValueError("unknown checkpoint layout: the keys are neither this package's nor torchvision's, timm's or Hugging "
                     f"Face's ViT names (first keys: {sorted(keys)[:5]})")


def _canonical(src, layout):
    """{canonical name: tensor} and the unused source keys.  Canonical: cls, pos, patch.weight, blocks.<i>.<part>.weight
    with part in ln1, qkv, proj, ln2, fc1, fc2 (q, k, v before they are joined), norm.*, head.*"""
    out, unused = {}, []
    blk = re.compile(_BLOCK_PREFIX[layout] + r"(.+)")
    for key, v in src.items():
        k = key[4:] if layout in ("hf", "hf5") and key.startswith("vit.") else key
        name = None
        m = blk.fullmatch(k)
        if m:
            for pat, part in _BLOCK[layout]:
                r = re.fullmatch(pat + r"[._](weight|bias)", m.group(2))
                if r:
                    name = f"blocks.{int(m.group(1))}.{part}.{r.group(1)}"
                    break
        elif _TOP[layout].get(k) in ("cls", "pos"):
            name = _TOP[layout][k]
        else:
            stem, _, leaf = k.rpartition(".")
            if leaf in ("weight", "bias") and _TOP[layout].get(stem) in ("patch", "norm", "head"):
                name = f"{_TOP[layout][stem]}.{leaf}"
        if name is None:
            unused.append(key)
        else:
            out[name] = v
    # q, k, v -> qkv, in that order along dim 0
    for name in [n for n in out if re.fullmatch(r"blocks\.\d+\.q\.(weight|bias)", n)]:
        i, leaf = name.split(".")[1], name.rsplit(".", 1)[1]
        parts = [out.pop(f"blocks.{i}.{p}.{leaf}", None) for p in "qkv"]
        if any(p is None for p in parts):
            raise ValueError(f"block {i}: the source has a separate query {leaf} but not key and value")
        out[f"blocks.{i}.qkv.{leaf}"] = torch.cat(parts, dim=0)
    for n in [n for n in out if re.fullmatch(r"blocks\.\d+\.[kv]\.(weight|bias)", n)]:
        raise ValueError(f"the source has {n} without a query")
    return out, unused


def _target_names(model_sd):
    """canonical part -> the model's key stem, per block index; found from the keys the model owns."""
    def pick(i, *cands):
        for c in cands:
            if f"blocks.{i}.{c}" in model_sd:
                return c
        return None
    depth = 1 + max((int(k.split(".")[1]) for k in model_sd if re.match(r"blocks\.\d+\.", k)), default=-1)
    names = {}
    for i in range(depth):
        names[i] = {
            "ln1.weight": "norm1.weight", "ln1.bias": "norm1.bias", "ln2.weight": "norm2.weight", "ln2.bias": "norm2.bias",
            "qkv.weight": pick(i, "attn.qkv.weight", "attn.in_proj_weight"),
            "qkv.bias": pick(i, "attn.qkv.bias", "attn.in_proj_bias"),
            "proj.weight": pick(i, "attn.proj.weight", "attn.out_proj.weight"),
            "proj.bias": pick(i, "attn.proj.bias", "attn.out_proj.bias"),
            "fc1.weight": pick(i, "mlp.fc1.weight", "mlp.0.weight"), "fc1.bias": pick(i, "mlp.fc1.bias", "mlp.0.bias"),
            "fc2.weight": pick(i, "mlp.fc2.weight", "mlp.3.weight"), "fc2.bias": pick(i, "mlp.fc2.bias", "mlp.3.bias")}
    return depth, names


def _grid(rows: int) -> Optional[int]:
    g = math.isqrt(rows - 1) if rows >= 2 else 0
    return g if g >= 1 and g * g == rows - 1 else None


def convert_state_dict(src: Dict[str, torch.Tensor], model: torch.nn.Module) -> Tuple[Dict[str, torch.Tensor], Report]:
    """(converted, report): `src` (any of the layouts of this module, detected by its keys) under the key names and in
    the shapes of `model`'s state dict.  Values keep their dtype; nothing is copied into the model.  pos_embed stays on
    the SOURCE's grid (report['source_grid']; load_pretrained resamples it).  Raises ValueError for an unknown layout,
    another patch size, width or depth (naming the key and both shapes) and a pos_embed that is no CLS row plus a
    square grid."""
    msd = model.state_dict()
    layout = detect_layout(src.keys(), msd.keys())
    rep = Report(layout=layout, loaded=[], skipped={}, unused=[], missing=[], source_grid=None, model_grid=None,
                 pos_embed=None, layer_norm_eps=None, pool_hint=None)
    conv: Dict[str, torch.Tensor] = {}
    if layout == "native":
        for k, v in src.items():
            if k in msd:
                conv[k] = v
            else:
                rep["unused"].append(k)
    else:
        canon, rep["unused"] = _canonical(src, layout)
        fc_norm = [k for k in ("fc_norm.weight", "fc_norm.bias") if k in src] if layout == "timm" else []
        if fc_norm and any(n.startswith("norm.") for n in canon):
            rep["unused"] = [f"{k} (the source has norm.*, which the model's norm takes)" if k in fc_norm else k
                             for k in rep["unused"]]
        elif fc_norm:
            for k in fc_norm:
                canon["norm." + k.split(".")[1]] = src[k]
                rep["unused"].remove(k)
            rep["pool_hint"] = ("avg", "after")
        rep["unused"] = sorted(rep["unused"])
        depth, names = _target_names(msd)
        src_depth = 1 + max((int(n.split(".")[1]) for n in canon if n.startswith("blocks.")), default=-1)
        if src_depth != depth:
            last = max((n for n in canon if n.startswith("blocks.")), key=lambda n: int(n.split(".")[1]), default="-")
            raise ValueError(f"depth differs: the source has {src_depth} blocks (up to {last}), the model {depth}")
        top = {"cls": "cls_token", "pos": "pos_embed", "patch.weight": "patch_embed.projection.1.weight",
               "patch.bias": "patch_embed.projection.1.bias", "norm.weight": "norm.weight", "norm.bias": "norm.bias",
               "head.weight": "head.weight", "head.bias": "head.bias"}
        for name, v in canon.items():
            if name.startswith("blocks."):
                _, i, part = name.split(".", 2)
                stem = names[int(i)].get(part)
                key = None if stem is None else f"blocks.{i}.{stem}"
            else:
                key = top[name] if top[name] in msd else None
            if key is None:
                rep["unused"].append(f"{name} (the model owns no such tensor)")
                continue
            if name == "patch.weight" and v.dim() == 4:
                want = msd[key].shape
                D, C, P, P2 = v.shape
                if P != P2 or (D, P * P * C) != tuple(want):
                    raise ValueError(f"{key}: the source's patch convolution {tuple(v.shape)} (D, C, P, P) gives a Linear "
                                     f"of shape {(D, P * P2 * C)}, the model's is {tuple(want)} (patch size or width differ)")
                v = v.permute(0, 2, 3, 1).reshape(D, P * P * C)          # (p1 p2 c), the order favit_patchify_fwd writes
            conv[key] = v
    # shapes against the model; the head may differ, pos_embed may sit on another grid, everything else is an error
    head_differs = [k for k in ("head.weight", "head.bias") if k in conv and tuple(conv[k].shape) != tuple(msd[k].shape)]
    for k in list(conv):
        v, want = conv[k], tuple(msd[k].shape)
        if k in ("head.weight", "head.bias") and head_differs:
            rep["skipped"][k] = (f"the source's head is {tuple(v.shape)}, the model's {want}: left as initialised" if k in
                                 head_differs else "skipped with the other half of the head")
            del conv[k]
        elif k == "pos_embed":
            if v.dim() != 3 or v.shape[0] != 1 or v.shape[2] != want[2]:
                raise ValueError(f"pos_embed: the source's shape {tuple(v.shape)} does not fit the model's {want} (width differs)")
            g = _grid(v.shape[1])
            if g is None:
                raise ValueError(f"pos_embed: the source's {v.shape[1]} rows are not a CLS row plus a square grid "
                                 f"(shape {tuple(v.shape)}, the model's {want})")
            rep["source_grid"], rep["model_grid"] = g, _grid(want[1])
        elif tuple(v.shape) != want:
            raise ValueError(f"{k}: the source's shape {tuple(v.shape)} differs from the model's {want}")
    rep["loaded"] = sorted(conv)
    rep["missing"] = sorted(k for k in msd if k not in conv and k not in rep["skipped"])
    return conv, rep


def load_pretrained(model: torch.nn.Module, path_or_state_dict, pos_embed: str = "resample",
                    antialias: bool = True) -> Report:
    """Load a checkpoint in any of this module's layouts into `model` and return the report (see Report).
    path_or_state_dict: a local file or Hugging Face directory (read_state_dict) or a state dict.  A pos_embed on
    another grid than the model's is resampled on the GPU by the kernel behind functional.pos_resample
    (pos_embed='resample'; antialias as there; needs a GPU, the model may live on the host or on the device) or is a
    ValueError (pos_embed='strict').  Everything is converted and checked before the first tensor of the model is
    written: a refused load leaves the model as it was."""
    if pos_embed not in ("resample", "strict"):
        raise ValueError("pos_embed must be 'resample' or 'strict'")
    eps = None
    if isinstance(path_or_state_dict, (str, os.PathLike)):
        src, eps = read_state_dict(path_or_state_dict)
    else:
        src = _unwrap(path_or_state_dict, "load_pretrained")
    conv, rep = convert_state_dict(src, model)
    rep["layer_norm_eps"] = eps
    msd = model.state_dict()
    if "pos_embed" in conv:
        rep["pos_embed"] = "copied"
        if rep["source_grid"] != rep["model_grid"]:
            if rep["model_grid"] is None:
                raise ValueError(f"pos_embed: the model's {msd['pos_embed'].shape[1]} rows are not a CLS row plus a square grid")
            if pos_embed == "strict":
                raise ValueError(f"pos_embed: the source's grid is {rep['source_grid']}x{rep['source_grid']} "
                                 f"{tuple(conv['pos_embed'].shape)}, the model's {rep['model_grid']}x{rep['model_grid']} "
                                 f"{tuple(msd['pos_embed'].shape)}, and pos_embed='strict'")
            from . import functional as F
            if not torch.cuda.is_available():
                raise RuntimeError("pos_embed: resampling to the model's grid runs on the GPU and none is available "
                                   "(there is no host fallback)")
            dev = msd["pos_embed"].device if msd["pos_embed"].is_cuda else torch.device("cuda", torch.cuda.current_device())
            with torch.no_grad(), torch.cuda.device(dev):
                p = conv["pos_embed"].to(device=dev, dtype=torch.float32)
                conv["pos_embed"] = F.pos_resample(p, rep["model_grid"], antialias=antialias, n_prefix=1)
            rep["pos_embed"] = "resampled"
    with torch.no_grad():
        for k, v in conv.items():
            msd[k].copy_(v)
    return rep
