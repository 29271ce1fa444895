#!/usr/bin/env python3
"""Device time of the input pipeline with and without RandAugment + Random Erasing, at the cfg2 batch (256 images of
224 x 224 from 256 x 256 uint8 sources).

Times, with HIP events around every repetition (5 warm-up repetitions, median of --reps = 30 timed ones, the two
formulations alternating so that both see the same machine state):
  (a) the plain transform: favit_image_transform (resample_h + resample_v), fp32 output only;
  (b) the augmented path: the same transform also writing its resized bytes, then favit_randaugment with a fresh
      RandAugment(2, 9) table per repetition set and the erase boxes of RandomErasing(p = 0.25) in its final write;
  (c) favit_randaugment alone on fixed bytes (b minus the transform), and favit_random_erase alone (the stand-alone
      form) on the fp32 batch.
The op tables and boxes are drawn and uploaded outside the timed windows (the loader uploads them asynchronously).
Prints one JSON line.

    python tools/augment_bench.py [--reps 30] [--batch 256] [--size 224]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch


def timed_alternating(fns, reps, warmup=5):
    """Median / min / max device time (us) of each callable, the callables taking turns within every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--source", type=int, default=256, help="side of the square uint8 source images")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU: nothing here can be measured on the host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("focused-attention-vit_amd")
    D, K = pkg.data, pkg.kernels
    dev = torch.device("cuda", 0)
    B, S, H = a.batch, a.size, a.source
    rs = np.random.RandomState(1234)
    # smooth images with noise on top: histograms and filters see something like a photograph, not white noise
    yy, xx = np.mgrid[0:H, 0:H]
    base = np.stack([(yy + xx) // 2 % 256, 255 - yy % 256, (xx * 3) % 256], 2)
    src = np.clip(base[None] + rs.randint(-24, 25, (B, H, H, 3)), 0, 255).astype(np.uint8)
    x = torch.from_numpy(src).to(dev)
    tf = D.DeviceTransform("imagenet_train", S, D.IMAGENET_MEAN, D.IMAGENET_STD, seed=0)
    prm = tf.params(B, H, H)
    ra, er = D.RandAugment(2, 9, seed=1), D.RandomErasing(p=0.25, seed=2)
    tables = [torch.from_numpy(ra.params(B, S)).to(dev) for _ in range(8)]
    boxes = [torch.from_numpy(er.params(B, S, S)[0]).to(dev) for _ in range(8)]
    _, u8 = tf(x, params=prm, want_bytes=True)
    fp32 = tf(x, params=prm)
    turn = [0]

    def plain():
        tf(x, params=prm)

    def augmented():
        k = turn[0] = (turn[0] + 1) % len(tables)
        _, b8 = tf(x, params=prm, want_bytes=True)
        K.randaugment(b8, tables[k], tf.mean, tf.std, boxes[k], 0.0)

    def randaugment_alone():
        k = turn[0] % len(tables)
        K.randaugment(u8, tables[k], tf.mean, tf.std, boxes[k], 0.0)

    def erase_alone():
        K.random_erase(fp32, boxes[turn[0] % len(boxes)], 0.0)

    res = {"tool": "augment_bench", "batch": [B, 3, S, S], "source": [H, H], "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "randaugment": [2, 9, 31], "erase_p": 0.25}
    res.update(timed_alternating({"a_plain_transform": plain, "b_transform_randaugment_erase": augmented,
                                  "c_randaugment_alone": randaugment_alone, "c_random_erase_alone": erase_alone}, a.reps))
    res["b_minus_a_us"] = round(res["b_transform_randaugment_erase"]["median_us"] - res["a_plain_transform"]["median_us"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
