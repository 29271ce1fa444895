#!/usr/bin/env python3
"""Cost of the weight EMA fused into AdamW at the cfg2 parameter count (the ~22.1 M floats of train.param_groups'
groups).

Times, with HIP events around every repetition (5 warm-up repetitions, median of --reps = 30 timed ones):
  (a) FusedAdamW.step() with ema_decay (one favit_adamw_ema launch per group: 38 B / element);
  (b) FusedAdamW.step() without it (today's favit_adamw launches: 30 B / element);
  (d) (b) followed by torch._foreach_lerp_ over per-parameter EMA tensors: the average kept outside the optimizer;
  (e) one ema_weights() enter-and-exit pair (two favit_swap_params launches per group: 2 x 18 B / element);
and prints one JSON line.  The byte ratio predicts (a) = 38 / 30 = 1.27 x (b).

    python tools/ema_bench.py [--reps 30] [--tree DIR]
--tree: import the package (and bench.py) from another checkout that has been built, e.g. the parent commit; a tree
whose FusedAdamW knows no ema_decay is timed for (b) only: row (c), the baseline on the same box.  Run it three
times: the spread of those medians is what (b) is compared against."""
import argparse
import importlib
import inspect
import json
import os
import statistics
import sys

import torch


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs the GPU: nothing here can be measured on the host")
    sys.path.insert(0, os.path.abspath(a.tree))
    pkg = importlib.import_module("focused-attention-vit_amd")
    import bench
    dev = torch.device("cuda", 0)
    pkg.set_compute_dtype("bf16")
    torch.manual_seed(1234)
    model = bench.build_model(pkg, "cfg2", dev, 0.0).train()
    T = pkg.train
    has_ema = "ema_decay" in inspect.signature(T.FusedAdamW.__init__).parameters

    def optimizer(**kw):
        pkg.functional.clear_lp_mirrors()
        o = T.FusedAdamW(T.param_groups(model, lr=1e-4), lr=1e-4, weight_decay=0.05, distributed=False, **kw)
        g = torch.Generator(device=dev).manual_seed(1)
        for grp in o.groups:
            grp["flat"].flat_g.copy_(torch.randn(grp["flat"].numel, device=dev, generator=g) * 1e-3)
        return o

    opt = optimizer()
    n = sum(g["flat"].numel for g in opt.groups)
    res = {"tool": "ema_bench", "tree": os.path.abspath(a.tree), "floats": n, "groups": [g["flat"].numel for g in opt.groups],
           "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    res["b_step_plain"] = timed(opt.step, a.reps)
    if has_ema:
        params = [p for g in opt.groups for p in g["flat"].params]
        avg = [p.detach().clone() for p in params]

        def step_then_lerp():
            opt.step()
            torch._foreach_lerp_(avg, [p.detach() for p in params], 1.0 - 0.999)
        res["d_step_then_foreach_lerp"] = timed(step_then_lerp, a.reps)
        res["d_tensors"] = len(params)
        del avg, opt
        opte = optimizer(ema_decay=0.999)
        res["a_step_ema"] = timed(opte.step, a.reps)

        def swap_pair():
            with opte.ema_weights():
                pass
        res["e_ema_weights_pair"] = timed(swap_pair, a.reps)
        res["a_over_b"] = round(res["a_step_ema"]["median_us"] / res["b_step_plain"]["median_us"], 3)
        res["d_over_b"] = round(res["d_step_then_foreach_lerp"]["median_us"] / res["b_step_plain"]["median_us"], 3)
        res["a_over_b_predicted"] = round(38.0 / 30.0, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
