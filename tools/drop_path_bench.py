#!/usr/bin/env python3
"""What stochastic depth costs on the bench model: the cfg2 training step (ViT-MHLA-Small, bf16, 256 images, the pruned
CLS-only path bench.py times by default) at drop-path rate 0 -- the path of before: native block chains, no new kernel --
and at --rate (default 0.1: every block but the first leaves the native chain and adds favit_drop_path_add /
favit_drop_path_bwd per half), each as an eager step (train.train_step) and as a HIP-graph replayed one
(train.GraphedStep).

The four arms live in ONE process, each on its own seeded copy of the model and optimizer.  A repeat times every arm in
turn (--warmup = 10 steps, then HIP events around --steps = 50 consecutive steps, host launch path included);
--repeats = 3 repeats alternate the arms, and the spread of an arm over its repeats is the yardstick for the difference
between two arms.  Prints one JSON line: per arm the per-step time of every repeat, the median and the spread, and the
two differences rate - 0.

    python tools/drop_path_bench.py [--rate 0.1] [--steps 50] [--repeats 3] [--batch 256]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="images per step (default: cfg2's 256)")
    a = ap.parse_args()
    if not 0.0 < a.rate < 1.0:
        raise SystemExit("--rate: in (0, 1)")
    if not torch.cuda.is_available():
        raise SystemExit("drop_path_bench needs the GPU: nothing here can be measured on the host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("focused-attention-vit_amd")
    import bench
    dev = torch.device("cuda", 0)
    pkg.set_compute_dtype("bf16")
    c = bench.CONFIGS["cfg2"]
    B = a.batch or c["batch"]
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(B, 3, c["img"], c["img"], device=dev, generator=g)
    labels = torch.randint(0, c["classes"], (B,), device=dev, generator=g)

    def arm(rate, graphed):
        torch.manual_seed(1234)
        model = bench.build_model(pkg, "cfg2", dev, 0.0).train().set_drop_path_rate(rate)
        opt = pkg.train.FusedAdamW(pkg.train.param_groups(model, lr=1e-4), lr=1e-4, weight_decay=0.05)
        if graphed:
            gs = pkg.train.GraphedStep(model, opt, images, labels, static_inputs=True)
            step = lambda: gs(images, labels)
        else:
            gs = None
            step = lambda: pkg.train.train_step(model, images, labels, opt)
        return {"step": step, "keep": (model, opt, gs), "ms_per_step": [], "loss": None}

    arms = {}
    for graphed in (False, True):
        for rate in (0.0, a.rate):
            arms[("graph" if graphed else "eager") + ("_rate0" if rate == 0.0 else "_rate")] = arm(rate, graphed)
    for _ in range(a.repeats):
        for r in arms.values():
            step = r["step"]
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                loss = step()
            e1.record()
            e1.synchronize()
            r["ms_per_step"].append(round(e0.elapsed_time(e1) / a.steps, 4))
            r["loss"] = float(loss.detach())
    res = {"tool": "drop_path_bench", "device": torch.cuda.get_device_name(0), "config": "cfg2", "dtype": "bf16",
           "batch": B, "rate": a.rate, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "arms": {}}
    for name, r in arms.items():
        res["arms"][name] = {"ms_per_step": r["ms_per_step"], "median_ms": round(statistics.median(r["ms_per_step"]), 4),
                             "spread_ms": round(max(r["ms_per_step"]) - min(r["ms_per_step"]), 4), "last_loss": r["loss"]}
    for kind in ("eager", "graph"):
        res[kind + "_rate_minus_rate0_ms"] = round(res["arms"][kind + "_rate"]["median_ms"] -
                                                   res["arms"][kind + "_rate0"]["median_ms"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
