#!/usr/bin/env python
"""Host side of an eager training step: how long does Python need to ENQUEUE a step, against how long the GPU needs to
run it?  

    python tools/host_enqueue.py [--config cfg2] [--steps 10] [--rounds 5] [--warmup 5]

Per round: time.perf_counter() around `steps` calls of train.train_step WITHOUT a synchronise in between (the host
runs ahead of the device), then one synchronise; HIP events around the same calls give the device time.  Where the
enqueue time per step is below the device time the step is GPU-bound and the host has slack; where the two agree the
host is the limit (the device waits for launches).  With the native block chains available, the rounds alternate
between them and the Python chains (functional.set_native_blocks) in ONE process, so both see the same machine state.
Prints one JSON line.  Keep steps * launches per step well below the depth of the HIP queue (a full queue blocks the
host, and the enqueue time then reads as the device time): 10 steps of a few hundred launches are safe."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the configurations and the model builder of the benchmark)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=["cfg2", "cfg4"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    c = bench.CONFIGS[args.config]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pkg = importlib.import_module("focused-attention-vit_amd")
    pkg._abi.lib()
    F = pkg.functional
    pkg.set_compute_dtype("bf16")
    torch.manual_seed(1234)
    model = bench.build_model(pkg, args.config, dev)
    model.train()
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(c["batch"], 3, c["img"], c["img"], device=dev, generator=g)
    labels = torch.randint(0, c["classes"], (c["batch"],), device=dev, generator=g)
    opt = pkg.train.FusedAdamW(pkg.train.param_groups(model, lr=1e-4), lr=1e-4, weight_decay=0.05)
    step = lambda: pkg.train.train_step(model, images, labels, opt)
    modes = ["native", "python"] if hasattr(F, "set_native_blocks") else ["python"]
    res = {m: {"enqueue_ms": [], "device_ms": [], "wall_ms": []} for m in modes}
    for m in modes:                                   # warm both paths (allocator, lazy kernel attributes, plans)
        if len(modes) > 1:
            F.set_native_blocks(m == "native")
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for m in modes:
            if len(modes) > 1:
                F.set_native_blocks(m == "native")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res[m]["enqueue_ms"].append(1e3 * (t1 - t0) / args.steps)
            res[m]["wall_ms"].append(1e3 * (t2 - t0) / args.steps)
            res[m]["device_ms"].append(e0.elapsed_time(e1) / args.steps)
    out = {"tool": "host_enqueue", "config": args.config, "steps": args.steps, "rounds": args.rounds,
           "knobs": bench.active_knobs()}
    for m in modes:
        out[m] = {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                  for k, v in res[m].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
