#!/usr/bin/env python3
"""main.py-equivalent runner (the reference's main.py:64-149 cannot even be imported: three wrong
import names, main.py:41-43).  Same argument names for the settings that concern the path; the dataset is an on-disk
one (--data_dir: CIFAR-10's binary distribution, or an ImageNet-style train/ + val/ image folder), a .npz file
{x_train uint8 [N,H,W,3], y_train, x_test, y_test} or a synthetic one.  Nothing is ever downloaded.

    python tools/run_experiment.py --experiment mhla --img_size 32 --patch_size 4 --embed_dim 64 --depth 2 \
        --num_heads 4 --epochs 3 --batch_size 64 --results_dir gpurun_out/exp
    python tools/run_experiment.py --experiment mhla_pretrained --dataset imagenet --data_dir /data/imagenet \
        --weights vit_b_16.npz --freeze_layers --epochs 5
"""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def synthetic_dataset(n, classes, size, seed):
    rs = np.random.RandomState(seed)
    protos = rs.randint(0, 256, size=(classes, size, size, 3))
    y = rs.randint(0, classes, size=n)
    x = np.clip(protos[y] + rs.randint(-40, 41, size=(n, size, size, 3)), 0, 255).astype(np.uint8)
    return x, y


def synthetic_blocks_dataset(n, classes, size, grid, seed, sample_seed=None):
    """Synthetic images for the SPPP experiment: a grid x grid board of flat colour blocks (a class-specific palette,
    per-sample brightness jitter per block).  SLIC finds exactly grid^2 superpixels on such an image, which is what the
    reference's forward needs from every image of a batch (torch.stack, models/sppp_mhla.py:300; the positional
    encoding accepts num_superpixels or num_superpixels - 1 regions, models/sppp.py:299) -- random-noise prototypes give
    1..16 regions per image and the reference's forward (and this one) raises on the first batch."""
    rs = np.random.RandomState(seed)
    # block colours well apart from their neighbours: a coarse lattice of base colours shuffled per class
    base = np.array([[r, g, b] for r in (40, 128, 215) for g in (40, 128, 215) for b in (40, 128, 215)], dtype=np.int32)
    pal = np.stack([base[rs.permutation(len(base))[:grid * grid]] for _ in range(classes)])        # [classes, g*g, 3]
    if sample_seed is not None:                          # (same palettes, other samples: the test split)
        rs = np.random.RandomState(sample_seed)
    y = rs.randint(0, classes, size=n)
    jit = rs.randint(-12, 13, size=(n, grid * grid, 1))
    blocks = np.clip(pal[y] + jit, 0, 255).astype(np.uint8).reshape(n, grid, grid, 3)
    cell = size // grid
    x = np.repeat(np.repeat(blocks, cell, axis=1), cell, axis=2)
    if x.shape[1] != size:                               # size not a multiple of the grid: pad by edge replication
        pad = size - x.shape[1]
        x = np.pad(x, ((0, 0), (0, pad), (0, pad), (0, 0)), mode="edge")
    return x, y


def batches(x, y, bs, shuffle, rs):
    idx = rs.permutation(len(x)) if shuffle else np.arange(len(x))
    return [(x[idx[i:i + bs]], y[idx[i:i + bs]]) for i in range(0, len(x) - bs + 1, bs)]


SPPP_TRAINABLE = ("head", "latent_proj", "segmentation", "patch_mapper", "pooling")


def build_model(pkg, a, classes):
    """The experiment's model (on the host).  The caller seeds torch first: the model is built seeded."""
    M = pkg.models
    kw = dict(img_size=a.img_size, patch_size=a.patch_size, num_classes=classes, embed_dim=a.embed_dim, depth=a.depth,
              num_heads=a.num_heads, dropout=a.dropout)
    rate = getattr(a, "drop_path", 0.0)
    pool = (getattr(a, "global_pool", "token"), getattr(a, "pool_norm", "before"))
    if a.experiment == "traditional":
        return M.vit.VisionTransformer(**kw).set_drop_path_rate(rate).set_global_pool(*pool)
    if a.experiment in ("mhla", "mhla_pretrained"):
        return M.vit_mhla.VisionTransformerMHLA(window_size=a.window_size, use_mhla=True,
                                                **kw).set_drop_path_rate(rate).set_global_pool(*pool)
    model = M.sppp_mhla.SPPPViTMHLA(num_superpixels=a.num_superpixels, pooling_type=a.pooling_type,
                                    window_size=a.window_size, use_mhla=True, **kw)
    model.segmentation.compactness = a.compactness
    return model.set_drop_path_rate(rate).set_global_pool(*pool)


def load_flat_weights(model, weights, antialias=True, what="weights"):
    """Load a checkpoint the user already has into the model through pretrained.load_pretrained and print its report:
    this project's own flat state-dict .npz (opened without pickle; a key the archive lacks stays as initialised, a key
    with another shape is an error, as ever), or a torchvision / timm / Hugging Face ViT checkpoint (.pt, .pth, .bin,
    .npz, .safetensors, an HF directory), whose pos_embed is resampled on the GPU when its grid is not the model's.
    Returns the names of the keys that were loaded."""
    pretrained = importlib.import_module("focused-attention-vit_amd").pretrained
    report = pretrained.load_pretrained(model, weights, pos_embed="resample", antialias=antialias)
    print(f"{what} {weights}: {report.summary()}")
    has = (getattr(model, "global_pool", "token"), getattr(model, "pool_norm", "before"))
    hint = report.get("pool_hint")
    if hint is not None and hint != has:
        print(f"{what} {weights}: the checkpoint was trained with --global_pool {hint[0]} --pool_norm {hint[1]}, "
              f"this run uses --global_pool {has[0]} --pool_norm {has[1]}")
    return report["loaded"]


def build_teacher(pkg, a, classes):
    """--teacher_experiment: a frozen model of the student's dimensions with dropout 0 and no drop path, in eval mode,
    with --teacher_weights loaded (any checkpoint --weights takes; for mhla_pretrained the same archive serves both:
    the dense model the student's weights came from supervises it).  On the host, like build_model."""
    ta = argparse.Namespace(**vars(a))
    ta.experiment, ta.dropout, ta.drop_path = a.teacher_experiment, 0.0, 0.0
    teacher = build_model(pkg, ta, classes)
    loaded = (load_flat_weights(teacher, a.teacher_weights, not a.no_pos_antialias, "teacher weights")
              if a.teacher_weights else [])
    for p in teacher.parameters():
        p.requires_grad = False
    print(f"teacher: {a.teacher_experiment}, {len(loaded)} tensors loaded from {a.teacher_weights}")
    return teacher.eval()


def prepare_pretrained(model, weights=None, freeze_layers=False, antialias=True):
    """The set-up of the reference's two pre-trained experiments (experiments/mhla_pretrained.py:224-247,
    experiments/sppp_mhla_pretrained.py:236-259).  weights: whatever load_flat_weights takes.  Every latent_proj becomes the
    identity (eye weight, zero bias).  freeze_layers: every parameter whose name contains none of head / latent_proj /
    segmentation / patch_mapper / pooling stops training (the last three only occur in the SPPP models, so this is
    both experiments' rule).  Returns the names of the keys that were loaded."""
    loaded = load_flat_weights(model, weights, antialias) if weights else []
    with torch.no_grad():
        for n, mod in model.named_modules():
            if n.endswith("latent_proj") and isinstance(mod, torch.nn.Linear):
                torch.nn.init.eye_(mod.weight)
                torch.nn.init.zeros_(mod.bias)
    if freeze_layers:
        for n, p in model.named_parameters():
            if not any(x in n for x in SPPP_TRAINABLE):
                p.requires_grad = False
    return loaded


def disk_dataset(pkg, a):
    """--data_dir: (train batches, test batches, number of classes) from the on-disk readers of datasets.py."""
    DS = pkg.datasets
    sub, sub5 = a.subset_size, (None if a.subset_size is None else a.subset_size // 5)
    if a.dataset == "cifar10":
        tr, te = DS.Cifar10Binary(a.data_dir, True, sub, a.seed), DS.Cifar10Binary(a.data_dir, False, sub5, a.seed)
    elif a.dataset == "imagenet":
        tr_dir, va_dir = os.path.join(a.data_dir, "train"), os.path.join(a.data_dir, "val")
        if not os.path.isdir(tr_dir) or not os.path.isdir(va_dir):
            raise FileNotFoundError(f"ImageNet train or validation directory not found in {a.data_dir}")
        tr, te = DS.ImageFolder(tr_dir, sub, a.seed), DS.ImageFolder(va_dir, sub5, a.seed)
    else:
        raise SystemExit("--data_dir needs --dataset cifar10 or imagenet")
    return (DS.batches(tr, a.batch_size, True, a.seed, num_workers=a.num_workers),
            DS.batches(te, a.batch_size, False, a.seed, num_workers=a.num_workers), len(tr.classes))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Vision Transformer experiments on the MI355X hot path")
    ap.add_argument("--experiment", required=True,
                    choices=["traditional", "mhla", "sppp_mhla", "mhla_pretrained", "sppp_mhla_pretrained"])
    ap.add_argument("--data", default=None, help=".npz dataset (default: synthetic)")
    ap.add_argument("--data_dir", default=None,
                    help="on-disk dataset: with --dataset cifar10 the binary distribution (data_batch_*.bin, test_batch.bin), "
                         "with --dataset imagenet a directory with train/ and val/ image folders")
    ap.add_argument("--subset_size", type=int, default=None, help="--data_dir: seeded random subset (test side: a fifth)")
    ap.add_argument("--num_workers", type=int, default=4, help="--data_dir: image decoding threads (at most 16)")
    ap.add_argument("--weights", default=None,
                    help="*_pretrained: a checkpoint on this machine: this project's flat state-dict .npz (keys it lacks stay as "
                         "initialised), or a torchvision / timm / Hugging Face ViT checkpoint (.pt, .pth, .bin, .npz, "
                         ".safetensors, an HF directory); a pos_embed of another grid is resampled to --img_size")
    ap.add_argument("--eval_img_size", type=int, default=None, metavar="S",
                    help="validate and test at S x S while training stays at --img_size: the models resample pos_embed to "
                         "the input's patch grid (default: --img_size; S must be a multiple of --patch_size; not for the "
                         "superpixel experiments)")
    ap.add_argument("--no_pos_antialias", action="store_true",
                    help="resample pos_embed with torch's plain bicubic instead of the antialiased one (timm's default), "
                         "at load time and at another input resolution")
    ap.add_argument("--freeze_layers", action="store_true",
                    help="*_pretrained: train only head, latent_proj and the SPPP components")
    ap.add_argument("--dataset", default="cifar10", choices=["cifar10", "imagenet", "default"], help="transform stack")
    ap.add_argument("--results_dir", default="./results")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--img_size", type=int, default=224)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--patch_size", type=int, default=16)
    ap.add_argument("--embed_dim", type=int, default=768)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--num_heads", type=int, default=12)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--drop_path", type=float, default=0.0, metavar="RATE",
                    help="stochastic depth: the last block drops each residual branch per sample with this probability, "
                         "block i of depth with RATE * i / (depth - 1) (set_drop_path_rate; not fp8)")
    ap.add_argument("--global_pool", default="token", choices=["token", "avg"],
                    help="what the head reads: the CLS row, or the mean over the other tokens (set_global_pool; student "
                         "and teacher alike).  avg reads every row, so the MHLA models run the dense step")
    ap.add_argument("--pool_norm", default="before", choices=["before", "after"],
                    help="--global_pool avg: the final LayerNorm before the mean, or after it (timm's fc_norm)")
    ap.add_argument("--num_superpixels", type=int, default=16)
    ap.add_argument("--compactness", type=float, default=0.1)
    ap.add_argument("--pooling_type", default="mean", choices=["mean", "max", "attention"])
    ap.add_argument("--window_size", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--learning_rate", type=float, default=1e-4)
    ap.add_argument("--weight_decay", type=float, default=0.05)
    ap.add_argument("--head_learning_rate", type=float, default=1e-3)
    ap.add_argument("--compute_dtype", default="bf16", choices=["bf16", "fp32", "fp8"])
    ap.add_argument("--clip_grad_norm", type=float, default=None,
                    help="clip the global gradient norm to this value in front of every update (default: no clipping)")
    ap.add_argument("--skip_nonfinite", action="store_true",
                    help="do not apply an update whose gradient norm is inf / NaN (counted, reported at the end)")
    ap.add_argument("--label_smoothing", type=float, default=0.0, help="training loss only; evaluation keeps plain cross-entropy")
    ap.add_argument("--mixup_alpha", type=float, default=0.0,
                    help="Mixup of every training batch with its flip, lam ~ Beta(a, a) (default 0: off; timm uses 0.8)")
    ap.add_argument("--cutmix_alpha", type=float, default=0.0,
                    help="CutMix of every training batch with its flip (default 0: off; timm uses 1.0)")
    ap.add_argument("--mix_prob", type=float, default=1.0, help="--mixup_alpha / --cutmix_alpha: probability of mixing a draw")
    ap.add_argument("--mix_switch_prob", type=float, default=0.5,
                    help="with both alphas > 0: probability that a draw is CutMix rather than Mixup")
    ap.add_argument("--mix_mode", default="batch", choices=["batch", "elem"],
                    help="one draw per batch, or one per image")
    ap.add_argument("--ra_num_ops", type=int, default=0,
                    help="RandAugment ops per training image, on the device (default 0: off; the usual recipe is 2)")
    ap.add_argument("--ra_magnitude", type=int, default=9, help="--ra_num_ops: magnitude bin of 31")
    ap.add_argument("--erase_prob", type=float, default=0.0,
                    help="Random Erasing probability per training image (default 0: off; the usual recipe is 0.25)")
    ap.add_argument("--erase_value", default="zero", choices=["zero", "normal"],
                    help="--erase_prob: fill the box with 0 or with one standard-normal value per element")
    ap.add_argument("--lr_schedule", default="constant", choices=["constant", "cosine"],
                    help="cosine: linear warm-up over --warmup_epochs, then half a cosine to zero over the remaining epochs")
    ap.add_argument("--warmup_epochs", type=float, default=0.0, help="--lr_schedule cosine: length of the linear warm-up")
    ap.add_argument("--ema_decay", type=float, default=None,
                    help="keep an exponential moving average of the trainable weights with this decay, inside the AdamW "
                         "launch (default: none)")
    ap.add_argument("--ema_warmup", action="store_true", help="--ema_decay: decay min(d, (1 + n) / (10 + n)) at update n")
    ap.add_argument("--eval_ema", action="store_true", help="--ema_decay: validate and test with the averaged weights")
    ap.add_argument("--checkpoint", default=None, metavar="PATH",
                    help="write the resumable training state here (train.save_checkpoint) and, at the end, the model-only "
                         "file PATH.ema with the averaged weights (the plain weights without --ema_decay)")
    ap.add_argument("--checkpoint_every", type=int, default=1, metavar="N", help="--checkpoint: every N epochs")
    ap.add_argument("--resume", action="store_true", help="--checkpoint: continue from PATH if it exists")
    ap.add_argument("--layer_decay", type=float, default=None, metavar="F",
                    help="layer-wise learning-rate decay: block i trains at F ** (depth - i) of the top rate "
                         "(train.param_groups(layer_decay=F)); builds the optimizer with fuse_groups=True")
    ap.add_argument("--no_wd_norm_bias", action="store_true",
                    help="no weight decay on biases, LayerNorm weights, cls_token and pos_embed "
                         "(train.param_groups(no_weight_decay='auto')); builds the optimizer with fuse_groups=True")
    ap.add_argument("--fuse_groups", action="store_true",
                    help="one arena and one AdamW launch for all parameter groups (train.FusedAdamW(fuse_groups=True))")
    ap.add_argument("--bucket_tokens", action="store_true",
                    help="sppp_mhla: run batches that mix images with num_superpixels and num_superpixels - 1 tokens group by "
                         "group (models.sppp.TokenBucketed; the reference -- and this tool without the flag -- fails on "
                         "such a batch in torch.stack, models/sppp_mhla.py:300; any other count fails in the "
                         "positional encoding, there and here)")
    ap.add_argument("--teacher_experiment", default=None, choices=["traditional", "mhla"],
                    help="knowledge distillation: a frozen teacher of this kind with the student's dimensions and dropout 0 "
                         "(default: no teacher)")
    ap.add_argument("--teacher_weights", default=None,
                    help="--teacher_experiment: a checkpoint as --weights takes (mhla_pretrained: the same file)")
    ap.add_argument("--distill_alpha", type=float, default=0.0,
                    help="training loss = (1 - a) * cross-entropy + a * teacher term (default 0: off; needs a teacher)")
    ap.add_argument("--distill_tau", type=float, default=1.0, help="--distill_type soft: the temperature")
    ap.add_argument("--distill_type", default="soft", choices=["soft", "hard"],
                    help="soft: tau^2 * KL(teacher || student) at temperature tau; hard: cross-entropy against the teacher's argmax")
    ap.add_argument("--eval_topk", type=int, nargs="+", default=None, metavar="K",
                    help="validate and test through the device metrics (harness.EvalMetrics) and report top-K accuracy for "
                         "up to 4 values, e.g. 1 5; 1 is always included; a K above the class count always hits; the CSV "
                         "gains test_top{K} columns (default: the evaluation and the columns of before)")
    ap.add_argument("--eval_per_class", action="store_true", help="print the per-class test accuracy (device metrics)")
    ap.add_argument("--eval_confusion", default=None, metavar="PATH",
                    help="write the test confusion matrix (row = label, column = prediction) as .npy (device metrics)")
    ap.add_argument("--eval_graph", action="store_true",
                    help="replay every evaluation batch as one HIP graph (harness.GraphedEval; device metrics)")
    a = ap.parse_args(argv)
    if a.eval_topk is not None:
        if any(k < 1 for k in a.eval_topk):
            ap.error("--eval_topk: every K must be >= 1")
        a.eval_topk = sorted(set(a.eval_topk) | {1})
        if len(a.eval_topk) > 4:
            ap.error("--eval_topk takes at most 4 values (1 included)")
    if not 0.0 <= a.distill_alpha <= 1.0:
        ap.error("--distill_alpha must be in [0, 1]")
    if a.distill_alpha > 0 and a.teacher_experiment is None:
        ap.error("--distill_alpha > 0 needs --teacher_experiment")
    if a.teacher_weights is not None and a.teacher_experiment is None:
        ap.error("--teacher_weights needs --teacher_experiment")
    if a.eval_img_size is not None:
        if a.eval_img_size < a.patch_size or a.eval_img_size % a.patch_size:
            ap.error("--eval_img_size must be a positive multiple of --patch_size")
        if a.experiment.startswith("sppp_mhla"):
            ap.error("--eval_img_size: the superpixel models carry no grid pos_embed to resample")
    if not (a.distill_tau > 0 and a.distill_tau != float("inf")):
        ap.error("--distill_tau must be a finite number > 0")
    return a


def main(argv=None):
    a = parse_args(argv)
    pretrained = a.experiment.endswith("_pretrained")
    sppp = a.experiment.startswith("sppp_mhla")

    pkg = importlib.import_module("focused-attention-vit_amd")
    pkg.set_compute_dtype(a.compute_dtype)
    torch.manual_seed(a.seed)
    rs = np.random.RandomState(a.seed)
    train_src = test_src = None
    if a.data_dir:
        train_src, test_src, classes = disk_dataset(pkg, a)
    elif a.data:
        d = np.load(a.data, allow_pickle=False)
        xtr, ytr, xte, yte = d["x_train"], d["y_train"], d["x_test"], d["y_test"]
    else:
        src = 32 if a.dataset == "cifar10" else a.img_size
        grid = int(round(a.num_superpixels ** 0.5))
        if sppp and grid * grid == a.num_superpixels:
            xtr, ytr = synthetic_blocks_dataset(2048, 10, src, grid, a.seed)
            xte, yte = synthetic_blocks_dataset(512, 10, src, grid, a.seed, sample_seed=a.seed + 1)
            if a.compactness == 0.1:
                # with the reference's colour-dominated default, blocks of similar colour merge and an image yields
                # 10..17 regions (measured); a spatially dominated SLIC returns the board's grid^2 cells for every image
                a.compactness = 200.0
                print("synthetic block images: SLIC compactness set to 200 (every image then yields "
                      f"{a.num_superpixels} superpixels; pass --compactness to override)")
        else:
            xtr, ytr = synthetic_dataset(2048, 10, src, a.seed)
            xte, yte = synthetic_dataset(512, 10, src, a.seed)       # same prototypes (same seed), fresh noise below
            xte = np.clip(xte.astype(np.int32) + rs.randint(-10, 11, size=xte.shape), 0, 255).astype(np.uint8)
    if train_src is None:
        classes = int(max(ytr.max(), yte.max())) + 1
    model = build_model(pkg, a, classes)
    if a.no_pos_antialias and hasattr(model, "set_pos_antialias"):
        model.set_pos_antialias(False)
    if pretrained:
        loaded = prepare_pretrained(model, a.weights, a.freeze_layers, not a.no_pos_antialias)
        n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
        print(f"pretrained set-up: {len(loaded)} tensors loaded from {a.weights}; trainable parameters {n_train:,} of "
              f"{sum(p.numel() for p in model.parameters()):,}")
    model = model.cuda()
    teacher = distill = None
    if a.teacher_experiment is not None and a.distill_alpha > 0:
        teacher = build_teacher(pkg, a, classes).cuda()
        distill = pkg.train.Distill(a.distill_alpha, a.distill_tau, a.distill_type)
    tfs = pkg.data.get_transforms(a.dataset, a.img_size, seed=a.seed)
    if a.eval_img_size is not None and a.eval_img_size != a.img_size:
        tfs["test"] = pkg.data.get_transforms(a.dataset, a.eval_img_size, seed=a.seed)["test"]
    group_kw, opt_kw = {}, {}          # (none of the three flags: exactly the groups and the optimizer of before)
    if a.layer_decay is not None:
        group_kw["layer_decay"] = a.layer_decay
    if a.no_wd_norm_bias:
        group_kw["no_weight_decay"] = "auto"
    if group_kw or a.fuse_groups:
        opt_kw["fuse_groups"] = True
    opt = pkg.train.FusedAdamW(pkg.train.param_groups(model, lr=a.learning_rate, head_lr=a.head_learning_rate, **group_kw),
                               lr=a.learning_rate, weight_decay=a.weight_decay, distributed=False,
                               max_grad_norm=a.clip_grad_norm, skip_nonfinite=a.skip_nonfinite, ema_decay=a.ema_decay,
                               ema_warmup=a.ema_warmup, **opt_kw)
    if a.eval_ema and a.ema_decay is None:
        raise SystemExit("--eval_ema needs --ema_decay")
    if (a.resume or a.checkpoint_every != 1) and a.checkpoint is None:
        raise SystemExit("--resume / --checkpoint_every need --checkpoint")

    class Epochs:            # a fresh shuffle per epoch
        def __init__(self, x, y, shuffle):
            self.x, self.y, self.shuffle = x, y, shuffle
        def __len__(self):
            return len(self.x) // a.batch_size
        def __iter__(self):
            return iter(batches(self.x, self.y, a.batch_size, self.shuffle, rs))
    # SPPP: the loaders segment batch k + 1 (device SLIC on a CU-masked stream) under the step of batch k; the steps
    # then run on the loader's compute stream, because a CU-masked stream synchronises with the default stream
    seg = getattr(model, "segmentation", None)
    if train_src is None:
        train_src, test_src = Epochs(xtr, ytr, True), Epochs(xte, yte, False)
    mix = None
    if a.mixup_alpha > 0 or a.cutmix_alpha > 0:           # training batches only; seeded like the transforms
        mix = pkg.data.BatchMix(a.mixup_alpha, a.cutmix_alpha, a.mix_prob, a.mix_switch_prob, a.mix_mode, seed=a.seed)
    augment = erase = None                                # training batches only, seeded like the transforms
    if a.ra_num_ops > 0:
        augment = pkg.data.RandAugment(a.ra_num_ops, a.ra_magnitude, seed=a.seed)
    if a.erase_prob > 0:
        erase = pkg.data.RandomErasing(p=a.erase_prob, value="normal" if a.erase_value == "normal" else 0, seed=a.seed)
    train_loader = pkg.data.DeviceLoader(train_src, tfs["train"], segmenter=seg, mix=mix, augment=augment, erase=erase)
    test_loader = pkg.data.DeviceLoader(test_src, tfs["test"], segmenter=seg)
    work = train_loader.compute_stream if seg is not None else torch.cuda.current_stream()
    work.wait_stream(torch.cuda.current_stream())
    run = pkg.models.sppp.TokenBucketed(model) if (a.bucket_tokens and seg is not None) else model
    schedule = None
    if a.lr_schedule == "cosine":
        per_epoch = max(1, len(train_src))
        schedule = pkg.train.WarmupCosine(opt, int(round(a.warmup_epochs * per_epoch)), max(1, a.epochs * per_epoch))
    metrics, fit_kw, eval_kw = None, {}, {}          # (none of the four flags: exactly the evaluation of before)
    if a.eval_topk is not None or a.eval_per_class or a.eval_confusion is not None or a.eval_graph:
        metrics = pkg.harness.EvalMetrics(classes, topk=a.eval_topk or (1,), per_class=a.eval_per_class,
                                          confusion=a.eval_confusion is not None)
        fit_kw = {"eval_metrics": metrics, "eval_graph": a.eval_graph}
        eval_kw = {"metrics": metrics, "graph": a.eval_graph, "opt": opt}
    with torch.cuda.stream(work):
        res = pkg.harness.fit(run, train_loader, test_loader, opt, a.epochs, label_smoothing=a.label_smoothing,
                              schedule=schedule, checkpoint=a.checkpoint, checkpoint_every=a.checkpoint_every,
                              resume=a.resume, eval_ema=a.eval_ema, teacher=teacher, distill=distill, **fit_kw)
        if metrics is not None:
            metrics.reset()
        if a.eval_ema:
            with opt.ema_weights():
                ev = pkg.harness.evaluate(run, test_loader, a.batch_size, **eval_kw)
        else:
            ev = pkg.harness.evaluate(run, test_loader, a.batch_size, **eval_kw)
        if a.checkpoint is not None:
            # the model a user takes away: the averaged weights when there is an average, in a model-only file
            if a.ema_decay is not None:
                with opt.ema_weights():
                    pkg.train.save_checkpoint(a.checkpoint + ".ema", model)
            else:
                pkg.train.save_checkpoint(a.checkpoint + ".ema", model)
            print(f"Model weights saved to {a.checkpoint}.ema")
    torch.cuda.current_stream().wait_stream(work)
    row = {"model": a.experiment, "img_size": a.img_size, "patch_size": a.patch_size, "embed_dim": a.embed_dim, "depth": a.depth,
           "num_heads": a.num_heads, "window_size": a.window_size, "total_parameters": sum(p.numel() for p in model.parameters()),
           "avg_epoch_time": res["avg_epoch_time"], "total_training_time": res["total_training_time"],
           "final_val_acc": res["final_val_acc"], "final_val_loss": res["final_val_loss"], "test_acc": ev["test_acc"],
           "test_loss": ev["test_loss"], "avg_inference_time_per_image": ev["avg_inference_time_per_image"],
           "peak_gpu_memory_mb": res["peak_gpu_memory_mb"]}
    if a.eval_topk is not None:
        row.update({f"test_top{k}": ev[f"test_top{k}"] for k in a.eval_topk})
        print("Test " + " | ".join(f"top-{k}: {ev[f'test_top{k}']:.2f}%" for k in a.eval_topk))
    if a.eval_per_class:
        print("Per-class test accuracy: " + " ".join(f"{v:.1f}" for v in ev["test_per_class_acc"]))
    if a.eval_confusion is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.eval_confusion)), exist_ok=True)
        np.save(a.eval_confusion, ev["test_confusion"].numpy())
        print(f"Confusion matrix saved to {a.eval_confusion}")
    if opt.skipped_steps is not None:
        print(f"updates skipped for a non-finite gradient norm: {int(opt.skipped_steps)}")
    path = os.path.join(a.results_dir, f"exp_{a.experiment}.csv")
    pkg.harness.save_results_csv(path, row)
    print(f"Results saved to {path}")


if __name__ == "__main__":
    main()
