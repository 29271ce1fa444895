#!/usr/bin/env python3
"""One optimizer step at the cfg2 parameter count (ViT-MHLA-Small, the ~22.1 M floats of tools/ema_bench.py): what
the one-arena optimizer (train.FusedAdamW(fuse_groups=True), one favit_adamw_multi launch) costs or buys against one
launch per parameter group.

Four arms in ONE process, each on its own copy of the model:
  (A) per-group, train.param_groups' three groups           -- the path of before
  (B) fused, the same three groups
  (C) fused, the groups of layer_decay + no_weight_decay="auto"
  (D) per-group, those groups (no guard: the per-group norm takes at most 16 groups)
each plain and, where the arm allows it, with max_grad_norm + ema_decay.  A repeat times every arm in turn (10 warm-up
steps, then HIP events around --steps = 200 consecutive step() calls, host launch path included); --repeats = 3
repeats alternate the arms, and the spread of an arm over its repeats is the yardstick for the differences between arms.
Prints one JSON line: per arm the groups, the kernel launches per step, the per-step time of every repeat, the median,
and the achieved bytes / s at 30 B per element (38 with the average) next to the 8 TB / s peak.

    python tools/adamw_groups_bench.py [--steps 200] [--repeats 3] [--layer_decay 0.75]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

PEAK_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layer_decay", type=float, default=0.75)
    a = ap.parse_args()
    if a.steps < 200 or a.repeats < 3:
        raise SystemExit("--steps: at least 200, --repeats: at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("adamw_groups_bench needs the GPU: nothing here can be measured on the host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("focused-attention-vit_amd")
    import bench
    dev = torch.device("cuda", 0)
    pkg.set_compute_dtype("bf16")
    T, K = pkg.train, pkg.kernels

    def arm(fuse, recipe, guard):
        torch.manual_seed(1234)
        model = bench.build_model(pkg, "cfg2", dev, 0.0).train()
        kw = dict(layer_decay=a.layer_decay, no_weight_decay="auto") if recipe else {}
        groups = T.param_groups(model, lr=1e-4, head_lr=1e-3, **kw)
        if guard and not fuse and len(groups) > K.GRAD_NORM_MAX_BUFS:
            return None
        okw = dict(max_grad_norm=1.0, ema_decay=0.999) if guard else {}
        o = T.FusedAdamW(groups, lr=1e-4, weight_decay=0.05, distributed=False, fuse_groups=fuse, **okw)
        g = torch.Generator(device=dev).manual_seed(1)
        for grp in o.groups:                 # a gradient in every parameter's slot; the padding stays zero
            for p in grp["flat"].params:
                p.grad.copy_(torch.randn(p.shape, device=dev, generator=g) * 1e-3)
        launches = (-(-len(groups) // K.ADAMW_MAX_SEGMENTS) if fuse else len(groups)) + (2 if guard else 0)
        return {"model": model, "opt": o, "groups": len(groups), "launches_per_step": launches,
                "floats": sum(p.numel() for grp in o.groups for p in grp["flat"].params),
                "bytes_per_float": 38 if guard else 30, "us_per_step": []}

    arms = {}
    for guard in (False, True):
        for name, fuse, recipe in (("A_per_group_3", False, False), ("B_fused_3", True, False),
                                   ("C_fused_recipe", True, True), ("D_per_group_recipe", False, True)):
            built = arm(fuse, recipe, guard)
            if built is not None:
                arms[name + ("_clip_ema" if guard else "")] = built
    for _ in range(a.repeats):
        for r in arms.values():
            step = r["opt"].step
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            e1.synchronize()
            r["us_per_step"].append(round(e0.elapsed_time(e1) * 1e3 / a.steps, 2))
    res = {"tool": "adamw_groups_bench", "device": torch.cuda.get_device_name(0), "steps": a.steps, "repeats": a.repeats,
           "layer_decay": a.layer_decay, "peak_bytes_per_s": PEAK_BYTES_PER_S, "arms": {}}
    for name, r in arms.items():
        med = statistics.median(r["us_per_step"])
        rate = r["floats"] * r["bytes_per_float"] / (med * 1e-6)
        res["arms"][name] = {"groups": r["groups"], "launches_per_step": r["launches_per_step"], "floats": r["floats"],
                             "us_per_step": r["us_per_step"], "median_us": med,
                             "spread_us": round(max(r["us_per_step"]) - min(r["us_per_step"]), 2),
                             "bytes_per_s": round(rate, -9), "of_peak": round(rate / PEAK_BYTES_PER_S, 3)}
    out = res["arms"]
    for tag in ("", "_clip_ema"):
        a_, b_, c_ = out["A_per_group_3" + tag], out["B_fused_3" + tag], out["C_fused_recipe" + tag]
        res["B_minus_A_us" + tag] = round(b_["median_us"] - a_["median_us"], 2)
        res["C_minus_B_us" + tag] = round(c_["median_us"] - b_["median_us"], 2)
        res["A_spread_us" + tag] = a_["spread_us"]
    res["D_over_C"] = round(out["D_per_group_recipe"]["median_us"] / out["C_fused_recipe"]["median_us"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
