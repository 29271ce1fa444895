#!/usr/bin/env python3
"""Measurements for the mixed-size input path ("Dataset readers and ragged batches"):

1. favit_image_transform_ragged against favit_image_transform on the SAME uniform batch (256 images of 375x500,
   imagenet_test, S = 224): bare library calls on preallocated buffers, HIP events, the two entry points alternating
   inside one loop so that clock drift hits both alike; medians and the 10th..90th percentile spread.
2. Host decode rate of datasets.ImageFolder + datasets.batches on a JPEG tree of 500x375 files that this script writes
   itself, with 4 and with 16 decoding threads.
3. The same tree through data.DeviceLoader (decode -> pinned staging -> H2D -> ragged transform), images per second.

    python tools/ragged_bench.py [--reps 30] [--files 512] [--out ragged_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def transform_timing(pkg, reps, warmup):
    D, K, abi = pkg.data, pkg.kernels, pkg._abi
    B, H, W, S = 256, 375, 500, 224
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randint(0, 256, size=(B, H, W, 3), dtype=np.uint8)).cuda()
    tf = D.DeviceTransform("imagenet_test", S, D.IMAGENET_MEAN, D.IMAGENET_STD)
    prm_h = tf.params(B, H, W)
    prm = torch.from_numpy(prm_h).cuda()
    desc = torch.from_numpy(np.stack([np.arange(B, dtype=np.int64) * H * W * 3, np.full(B, H, dtype=np.int64),
                                      np.full(B, W, dtype=np.int64)], axis=1)).cuda()
    ch_max = int(prm_h[:, 2].max())
    tmp = torch.empty((B, ch_max, S, 3), dtype=torch.uint8, device="cuda")
    out_u = torch.empty((B, 3, S, S), dtype=torch.float32, device="cuda")
    out_r = torch.empty_like(out_u)
    lib = abi.lib()
    flat = x.view(-1)

    def uniform():
        abi.check(lib.favit_image_transform(K._p(x), K._p(tmp), K._p(out_u), None, K._p(prm), B, H, W, 3, ch_max, S, tf.mean,
                                            tf.std, K._st()), "favit_image_transform")

    def ragged():
        abi.check(lib.favit_image_transform_ragged(K._p(flat), K._p(desc), K._p(tmp), K._p(out_r), None, K._p(prm), B, 3,
                                                   ch_max, S, tf.mean, tf.std, K._st()), "favit_image_transform_ragged")
    for _ in range(warmup):
        uniform()
        ragged()
    torch.cuda.synchronize()
    assert torch.equal(out_u, out_r)
    t = {"uniform": [], "ragged": []}
    for _ in range(reps):
        for name, fn in (("uniform", uniform), ("ragged", ragged)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    res = {k: {"median_ms": pct(v, 50), "p10_ms": pct(v, 10), "p90_ms": pct(v, 90), "min_ms": min(v), "max_ms": max(v)}
           for k, v in t.items()}
    res["ragged_over_uniform"] = res["ragged"]["median_ms"] / res["uniform"]["median_ms"]
    res["shape"] = f"{B} x {H}x{W}x3 -> {S}, imagenet_test, reps {reps}, warm-up {warmup}"
    return res


def write_jpeg_tree(root, n, classes=8):
    from PIL import Image
    rs = np.random.RandomState(1)
    for i in range(n):
        d = os.path.join(root, f"class{i % classes:02d}")
        os.makedirs(d, exist_ok=True)
        low = rs.randint(0, 256, size=(24, 32, 3), dtype=np.uint8)           # photograph-like: smooth, with some texture
        im = np.asarray(Image.fromarray(low).resize((500, 375), Image.BICUBIC)).astype(np.int16)
        im = np.clip(im + rs.randint(-12, 13, size=im.shape), 0, 255).astype(np.uint8)
        Image.fromarray(im).save(os.path.join(d, f"img{i:05d}.jpg"), quality=90)


def decode_rates(pkg, root, workers_list, batch):
    DS = pkg.datasets
    ds = DS.ImageFolder(root)
    out = {}
    for w in workers_list:
        rates = []
        for _ in range(3):
            t0 = time.perf_counter()
            n = sum(len(y) for _, y in DS.batches(ds, batch, True, 0, num_workers=w))
            rates.append(n / (time.perf_counter() - t0))
        out[f"workers_{w}"] = {"images_per_s_median": pct(rates, 50), "runs": rates}
    return out


def loader_rate(pkg, root, workers, batch):
    D, DS = pkg.data, pkg.datasets
    ds = DS.ImageFolder(root)
    tf = D.DeviceTransform("imagenet_train", 224, D.IMAGENET_MEAN, D.IMAGENET_STD)
    loader = D.DeviceLoader(DS.batches(ds, batch, True, 0, num_workers=workers), tf)
    rates = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for x, y in loader:
            n += y.numel()
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    return {"workers": workers, "images_per_s_median": pct(rates, 50), "runs": rates}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("focused-attention-vit_amd")
    res = {"transform": transform_timing(pkg, a.reps, a.warmup)}
    print(json.dumps(res["transform"]), flush=True)
    with tempfile.TemporaryDirectory() as root:
        write_jpeg_tree(root, a.files)
        res["decode"] = decode_rates(pkg, root, (4, 16), a.batch)
        print(json.dumps(res["decode"]), flush=True)
        res["loader"] = loader_rate(pkg, root, 16, a.batch)
        print(json.dumps(res["loader"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
