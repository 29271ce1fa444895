#!/usr/bin/env python3
"""What resampling pos_embed in every step costs on the bench model: forward plus backward of the cfg2 model
(ViT-MHLA-Small, bf16, 256 images of 224 x 224, the pruned CLS-only path bench.py times by default) with its own
14 x 14 pos_embed -- the path of before: PrologueOp never reaches the new code -- and with a 10 x 10 pos_embed that
functional.PrologueOp resamples to 14 x 14 in front of the prologue kernel and whose gradient comes back through the
adjoint (two favit_pos_resample launches per step more).  Also the two launches alone, back to back.

The two arms live in ONE process on seeded copies of the model.  A repeat times every arm in turn (--warmup steps, then
HIP events around --steps consecutive forward + backward passes, host launch path included); --repeats repeats
alternate the arms, and the spread of an arm over its repeats is the yardstick for the difference between the two.
Prints one JSON line.

    python tools/pos_resample_bench.py [--steps 50] [--repeats 5] [--batch 256] [--grid 10]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="images per step (default: cfg2's 256)")
    ap.add_argument("--grid", type=int, default=10, help="side of the stored pos_embed grid of the resampling arm")
    ap.add_argument("--launches", type=int, default=500, help="back-to-back launches per timing of the kernel alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pos_resample_bench needs the GPU: nothing here can be measured on the host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("focused-attention-vit_amd")
    import bench
    K = pkg.kernels
    dev = torch.device("cuda", 0)
    pkg.set_compute_dtype("bf16")
    c = bench.CONFIGS["cfg2"]
    B = a.batch or c["batch"]
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(B, 3, c["img"], c["img"], device=dev, generator=g)
    labels = torch.randint(0, c["classes"], (B,), device=dev, generator=g)

    def arm(grid):
        torch.manual_seed(1234)
        model = bench.build_model(pkg, "cfg2", dev, 0.0).train()
        D = model.pos_embed.shape[2]
        if grid is not None:
            model.pos_embed = torch.nn.Parameter(torch.randn(1, 1 + grid * grid, D, device=dev) * 0.02)

        def step():
            for p in model.parameters():
                p.grad = None
            loss = pkg.train.cross_entropy(model(images), labels)
            loss.backward()
            return loss
        return {"step": step, "keep": model, "ms_per_step": [], "loss": None}

    arms = {"native_14": arm(None), f"resampled_{a.grid}_to_14": arm(a.grid)}
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

    # the two launches alone: 10 x 10 -> 14 x 14 rows of D = 384 and the adjoint, back to back on one stream
    D = 384
    x = torch.randn(1 + a.grid * a.grid, D, device=dev)
    dy = torch.randn(1 + 14 * 14, D, device=dev)
    alone = {}
    for name, fn in (("forward_us", lambda: K.pos_resample(x, a.grid, 14, True)),
                     ("adjoint_us", lambda: K.pos_resample(dy, a.grid, 14, True, adjoint=True))):
        times = []
        for _ in range(a.repeats):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            times.append(round(1e3 * e0.elapsed_time(e1) / a.launches, 3))
        alone[name] = {"per_launch": times, "median": statistics.median(times)}
    res = {"tool": "pos_resample_bench", "device": torch.cuda.get_device_name(0), "config": "cfg2", "dtype": "bf16",
           "batch": B, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "what": "forward + backward, no optimizer",
           "arms": {}, "launch_alone_back_to_back_host_issue_included": alone}
    for name, r in arms.items():
        res["arms"][name] = {"ms_per_step": r["ms_per_step"], "median_ms": round(statistics.median(r["ms_per_step"]), 4),
                             "spread_ms": round(max(r["ms_per_step"]) - min(r["ms_per_step"]), 4), "last_loss": r["loss"]}
    names = list(arms)
    res["resampled_minus_native_ms"] = round(res["arms"][names[1]]["median_ms"] - res["arms"][names[0]]["median_ms"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
