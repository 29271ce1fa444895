#!/usr/bin/env python
"""What does looking cost?  One eval batch of the cfg2 and cfg3 sizes in bf16, three ways:

  shipped    model(images) in eval mode under torch.no_grad(): the CLS-only pruned, native block path where it applies
  unpruned   the same with FAVIT_NO_PRUNE=1: every block on all rows
  captured   harness.attention_maps(model, images): the unpruned Python chains with the probability kernel on every
             block's qkv, plus the rollout launch and the torch gathers of the result

    python tools/attention_maps_bench.py [--configs cfg2 cfg3] [--iters 10] [--rounds 5] [--warmup 2] [--out FILE]

Per round and mode: HIP events around `iters` calls give the device time, time.perf_counter() around the same calls and
a final synchronisation the wall time; both per call.  The rounds alternate between the modes in ONE process, so all
three see the same machine state.  The two kernels are also timed alone (one block's head-mean map on a random qkv of
the configuration's size; the rollout of `depth` such maps), back to back, events around `iters` launches.  There is no
pass mark.  Writes one JSON line per configuration to --out (default
profiles/attention_maps_bench.json) and prints it."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the configurations and the model builder of the benchmark)


def run_config(pkg, cfg, args, dev):
    c = bench.CONFIGS[cfg]
    torch.manual_seed(1234)
    model = bench.build_model(pkg, cfg, dev)
    B = c["batch"]
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(B, 3, c["img"], c["img"], device=dev, generator=g)
    if cfg == "cfg3":                                # label maps are input data here, as in bench.py
        maps = bench.synthetic_label_maps(8, 224, 16, seed=100)
        model.segmentation.set_label_maps(torch.from_numpy(np.stack([maps[i % 8] for i in range(B)])).to(dev))
        model.assume_num_tokens = 16
    model.eval()
    knobs = bench.active_knobs()

    def call(mode):
        if mode == "captured":
            return pkg.harness.attention_maps(model, images)["rollout"]
        if mode == "unpruned":
            os.environ["FAVIT_NO_PRUNE"] = "1"
        try:
            with torch.no_grad():
                return model(images)
        finally:
            if mode == "unpruned":
                del os.environ["FAVIT_NO_PRUNE"]

    modes = ["shipped", "unpruned", "captured"]
    res = {m: {"device_ms": [], "wall_ms": []} for m in modes}
    for m in modes:
        for _ in range(args.warmup):
            call(m)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for m in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.iters):
                call(m)
            e1.record()
            torch.cuda.synchronize()
            res[m]["wall_ms"].append(1e3 * (time.perf_counter() - t0) / args.iters)
            res[m]["device_ms"].append(e0.elapsed_time(e1) / args.iters)
    f = c["flops"]
    L, D, W, depth = f["L"], f["D"], f["W"], f["depth"]
    # the two kernels alone, on a random qkv of the configuration's size: one block's head-mean map, the whole rollout
    K = pkg.kernels
    H = D // f["hd"]
    qkv = torch.randn(B * L, 3 * D, device=dev, generator=g).to(torch.bfloat16)
    maps = [K.mhla_attn_probs(qkv, B, L, H, f["hd"], W, head_mean=True) for _ in range(depth)]
    alone = {"probs_kernel_ms": lambda: K.mhla_attn_probs(qkv, B, L, H, f["hd"], W, head_mean=True),
             "rollout_kernel_ms": lambda: K.attn_rollout(maps, [W] * depth)}
    for name, fn in alone.items():
        fn()
        vals = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            vals.append(e0.elapsed_time(e1) / args.iters)
        alone[name] = round(statistics.median(vals), 4)
    out = {"tool": "attention_maps_bench", "config": cfg, "batch": B, "tokens": L, "iters": args.iters,
           "rounds": args.rounds, "knobs": knobs,
           # per block: the q and k thirds of the bf16 qkv read once, B * L * W fp32 written
           "probs_bytes_estimate": depth * (B * L * 2 * D * 2 + B * L * W * 4)}
    out.update(alone)
    for m in modes:
        out[m] = {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                  for k, v in res[m].items()}
    out["captured_over_unpruned_device"] = round(out["captured"]["device_ms"]["median"] /
                                                 out["unpruned"]["device_ms"]["median"], 3)
    out["captured_over_unpruned_wall"] = round(out["captured"]["wall_ms"]["median"] /
                                               out["unpruned"]["wall_ms"]["median"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2", "cfg3"], choices=["cfg2", "cfg3"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pkg = importlib.import_module("focused-attention-vit_amd")
    pkg._abi.lib()
    pkg.set_compute_dtype("bf16")
    lines = []
    for cfg in args.configs:
        lines.append(run_config(pkg, cfg, args, dev))
        pkg.functional.clear_lp_mirrors()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
