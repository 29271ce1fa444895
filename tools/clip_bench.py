#!/usr/bin/env python3
"""Cost of global-norm clipping at the cfg2 parameter count (the ~22.1 M floats of train.param_groups' groups).

Times, with HIP events around every repetition (warm-up first, median of --reps >= 20 repetitions):
  (a) the favit_grad_norm launch pair alone -- "warm": the gradients were just read (they fit the 256 MiB
      Infinity Cache), "evicted": a 1 GiB fill runs (untimed) in front of every repetition;
  (b) FusedAdamW.step() with max_grad_norm (norm pair + one favit_adamw_clip launch per group);
  (c) FusedAdamW.step() without it (today's launches).
and prints one JSON line.  The floor quoted for (a) is its 4 B / element over the HBM rate.

    python tools/clip_bench.py [--reps 30] [--tree DIR]
--tree: import the package (and bench.py) from another checkout that has been built, e.g. the parent commit, and time
(c) only when that tree's FusedAdamW knows no max_grad_norm: the baseline on the same box."""
import argparse
import importlib
import inspect
import json
import os
import statistics
import sys

import torch

HBM_BYTES_PER_S = 6.29e12          # the rate membw.py's copy reaches on this part


def timed(fn, reps, warmup=5, before=None):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        if before is not None:
            before()
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
        raise SystemExit("clip_bench needs the GPU: nothing here can be measured on the host")
    sys.path.insert(0, os.path.abspath(a.tree))
    pkg = importlib.import_module("focused-attention-vit_amd")
    import bench
    dev = torch.device("cuda", 0)
    pkg.set_compute_dtype("bf16")
    torch.manual_seed(1234)
    model = bench.build_model(pkg, "cfg2", dev, 0.0).train()
    T, K = pkg.train, pkg.kernels
    has_clip = "max_grad_norm" in inspect.signature(T.FusedAdamW.__init__).parameters

    def optimizer(**kw):
        pkg.functional.clear_lp_mirrors()
        o = T.FusedAdamW(T.param_groups(model, lr=1e-4), lr=1e-4, weight_decay=0.05, distributed=False, **kw)
        g = torch.Generator(device=dev).manual_seed(1)
        for grp in o.groups:
            grp["flat"].flat_g.copy_(torch.randn(grp["flat"].numel, device=dev, generator=g) * 1e-3)
        return o

    opt = optimizer()
    n = sum(g["flat"].numel for g in opt.groups)
    res = {"tool": "clip_bench", "tree": os.path.abspath(a.tree), "floats": n, "groups": [g["flat"].numel for g in opt.groups],
           "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    res["c_step_plain"] = timed(opt.step, a.reps)
    if has_clip:
        bufs = [g["flat"].flat_g for g in opt.groups]
        out, ws = torch.empty(2, device=dev), K.grad_norm_workspace(dev)
        norm = float(K.grad_norm(bufs, out=out, ws=ws)[0])
        ref = float(torch.sqrt(sum((b.double() ** 2).sum() for b in bufs)))
        res["norm"], res["norm_rel_err_vs_float64"] = norm, abs(norm - ref) / ref
        res["a_floor_us"] = round(4.0 * n / HBM_BYTES_PER_S * 1e6, 2)
        res["a_norm_pair_warm"] = timed(lambda: K.grad_norm(bufs, out=out, ws=ws), a.reps)
        big = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        res["a_norm_pair_evicted"] = timed(lambda: K.grad_norm(bufs, out=out, ws=ws), a.reps, before=lambda: big.fill_(1.0))
        del big
        del opt
        optc = optimizer(max_grad_norm=norm / 4)
        res["b_step_clipped"] = timed(optc.step, a.reps)
        res["b_over_c"] = round(res["b_step_clipped"]["median_us"] / res["c_step_plain"]["median_us"], 3)
        res["a_over_floor"] = round(res["a_norm_pair_evicted"]["median_us"] / res["a_floor_us"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
