#!/usr/bin/env python3
"""Where a model looks: attention rollout and the CLS attention of the last block for the first images of a test set
(harness.attention_maps).  Takes run_experiment.py's --experiment / --weights / --data /
--data_dir and model geometry arguments and writes into --out:

    rollout.npy        fp32 [N, L]        attention rollout of the CLS row through all blocks
    cls_attention.npy  fp32 [N, L]        the last block's CLS row, head mean, per key
    grid.npy           fp32 [N, gh, gw]   rollout on the patch grid (a superpixel model: every patch of a superpixel
                                          carries its token's value)
    logits.npy         fp32 [N, classes]
    layer_XX.npy       with --per_head, the per-head map of every block
    image_XXXX.png     if Pillow imports: the input with the grid upsampled (nearest) over it

    python tools/attention_maps.py --experiment mhla --img_size 32 --patch_size 4 --embed_dim 192 --depth 12 \\
        --num_heads 3 --weights model.npz --data cifar.npz --num_images 8 --out maps/
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import run_experiment as RE


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Attention rollout and CLS attention maps of a trained model")
    ap.add_argument("--experiment", required=True,
                    choices=["traditional", "mhla", "sppp_mhla", "mhla_pretrained", "sppp_mhla_pretrained"])
    ap.add_argument("--data", default=None, help=".npz dataset with x_test / y_test (default: synthetic)")
    ap.add_argument("--data_dir", default=None, help="dataset directory (--dataset cifar10 or imagenet)")
    ap.add_argument("--subset_size", type=int, default=None)
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--weights", default=None, help="a checkpoint as run_experiment.py's --weights takes (default: the seeded initialisation)")
    ap.add_argument("--dataset", default="cifar10", choices=["cifar10", "imagenet", "default"], help="transform stack")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--img_size", type=int, default=224)
    ap.add_argument("--patch_size", type=int, default=16)
    ap.add_argument("--embed_dim", type=int, default=768)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--num_heads", type=int, default=12)
    ap.add_argument("--num_superpixels", type=int, default=16)
    ap.add_argument("--compactness", type=float, default=0.1)
    ap.add_argument("--pooling_type", default="mean", choices=["mean", "max", "attention"])
    ap.add_argument("--window_size", type=int, default=7)
    ap.add_argument("--compute_dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--num_images", type=int, default=8)
    ap.add_argument("--per_head", action="store_true", help="also write every block's per-head map (layer_XX.npy)")
    ap.add_argument("--residual", type=float, default=0.5, help="weight of the identity in every rollout step")
    a = ap.parse_args(argv)
    if a.num_images < 1:
        ap.error("--num_images must be >= 1")
    a.dropout, a.drop_path, a.batch_size = 0.0, 0.0, a.num_images
    return a


def test_images(pkg, a):
    """(host batches of the test side, number of classes): num_images images as ONE batch."""
    if a.data_dir:
        _, test_src, classes = RE.disk_dataset(pkg, a)
        return test_src, classes
    if a.data:
        d = np.load(a.data, allow_pickle=False)
        x, y = d["x_test"], d["y_test"]
        classes = int(max(d["y_train"].max(), y.max())) + 1 if "y_train" in d.files else int(y.max()) + 1
    else:
        src = 32 if a.dataset == "cifar10" else a.img_size
        grid = int(round(a.num_superpixels ** 0.5))
        if a.experiment.startswith("sppp_mhla") and grid * grid == a.num_superpixels:
            x, y = RE.synthetic_blocks_dataset(max(a.num_images, 16), 10, src, grid, a.seed, sample_seed=a.seed + 1)
            if a.compactness == 0.1:
                a.compactness = 200.0              # (as run_experiment.py: every block image then yields grid^2 regions)
        else:
            x, y = RE.synthetic_dataset(max(a.num_images, 16), 10, src, a.seed)
        classes = 10
    if len(x) < a.num_images:
        raise SystemExit(f"the test set holds {len(x)} images, --num_images asks for {a.num_images}")
    return [(x[:a.num_images], y[:a.num_images])], classes


def write_pngs(out_dir, images, grid):
    """image_XXXX.png: the input, min-max scaled per image, with the grid (nearest upsampling, scaled by its maximum)
    as brightness.  Returns the number written; 0 without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return 0
    img = images.float().cpu().numpy().transpose(0, 2, 3, 1)
    g = grid.float().cpu().numpy()
    for i in range(img.shape[0]):
        lo, hi = img[i].min(), img[i].max()
        base = (img[i] - lo) / (hi - lo if hi > lo else 1.0)
        ry, rx = -(-base.shape[0] // g.shape[1]), -(-base.shape[1] // g.shape[2])
        heat = np.repeat(np.repeat(g[i], ry, axis=0), rx, axis=1)[:base.shape[0], :base.shape[1]]
        heat = heat / (heat.max() if heat.max() > 0 else 1.0)
        over = base[..., :3] * (0.25 + 0.75 * heat[..., None])
        Image.fromarray((over * 255).clip(0, 255).astype(np.uint8).squeeze()).save(
            os.path.join(out_dir, f"image_{i:04d}.png"))
    return img.shape[0]


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("focused-attention-vit_amd")
    pkg.set_compute_dtype(a.compute_dtype)
    torch.manual_seed(a.seed)
    test_src, classes = test_images(pkg, a)
    model = RE.build_model(pkg, a, classes)
    if a.experiment.endswith("_pretrained"):
        loaded = RE.prepare_pretrained(model, a.weights)
    else:
        loaded = RE.load_flat_weights(model, a.weights) if a.weights else []
    print(f"{a.experiment}: {len(loaded)} tensors loaded from {a.weights}")
    model = model.cuda().eval()
    seg = getattr(model, "segmentation", None)
    loader = pkg.data.DeviceLoader(test_src, pkg.data.get_transforms(a.dataset, a.img_size, seed=a.seed)["test"],
                                   segmenter=seg)
    work = loader.compute_stream if seg is not None else torch.cuda.current_stream()
    work.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(work):
        images, _ = next(iter(loader))
        images = images[:a.num_images]
        res = pkg.harness.attention_maps(model, images, per_head=a.per_head, residual=a.residual)
    torch.cuda.current_stream().wait_stream(work)
    torch.cuda.synchronize()
    os.makedirs(a.out, exist_ok=True)
    for name in ("rollout", "cls_attention", "logits", "grid"):
        if res[name] is not None:
            np.save(os.path.join(a.out, name + ".npy"), res[name].float().cpu().numpy())
    if a.per_head:
        for k, p in enumerate(res["layers"]):
            np.save(os.path.join(a.out, f"layer_{k:02d}.npy"), p.cpu().numpy())
    n_png = write_pngs(a.out, images, res["grid"]) if res["grid"] is not None else 0
    r = res["rollout"]
    print(f"{r.shape[0]} images, {r.shape[1]} tokens, windows {res['window']}: rollout mass on CLS "
          f"{r[:, 0].mean().item():.4f}, tokens holding any mass {(r > 0).sum(1).float().mean().item():.1f} of {r.shape[1]}")
    print(f"wrote rollout.npy, cls_attention.npy, logits.npy{', grid.npy' if res['grid'] is not None else ''}"
          f"{f', {n_png} PNG files' if n_png else ''} to {a.out}")


if __name__ == "__main__":
    main()
