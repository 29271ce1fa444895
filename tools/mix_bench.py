#!/usr/bin/env python3
"""Cost of batch mixing at the cfg2 batch (256 x 3 x 224 x 224 fp32, 154 MB).

Times, with HIP events around every repetition (5 warm-up repetitions, median of --reps = 30 timed ones):
  (a) favit_batch_mix as a full Mixup (every row blended with lam = 0.3: one read and one write of the batch, 308 MB);
  (b) favit_batch_mix as a typical CutMix (every row, the 158 x 158 box of lam = 0.5 at the centre: only the 16-byte
      groups the box meets are read and written);
  (c) the torch formulation x.mul_(lam).add_(x.flip(0), alpha=1 - lam): three launches and a temporary;
and, with --step, the cfg2 training step (bench.py's model, eager, bf16) with and without mixing in front of it and the
mixed-target loss behind it.  Prints one JSON line; TB/s is the bytes each formulation has to move (a: 2 x batch;
b: 2 x the groups of the box; c: the same 2 x batch as a, i.e. its useful traffic) over the median.

    python tools/mix_bench.py [--reps 30] [--step]"""
import argparse
import importlib
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--step", action="store_true", help="also time the cfg2 training step with and without mixing")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench needs the GPU: nothing here can be measured on the host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("focused-attention-vit_amd")
    K = pkg.kernels
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    torch.manual_seed(1234)
    x = torch.randn(B, 3, S, S, device=dev)
    nbytes = x.numel() * 4
    res = {"tool": "mix_bench", "batch": [B, 3, S, S], "batch_mb": round(nbytes / 1e6, 1), "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}

    def tbs(moved, t):
        return round(moved / (t["median_us"] * 1e-6) / 1e12, 3)

    # (a) full Mixup.  (Values stay bounded under repetition: every call is a convex combination of the rows.)
    lam_mix = torch.full((B,), 0.3, device=dev)
    box0 = torch.zeros(B, 4, dtype=torch.int32, device=dev)
    res["a_mixup"] = timed(lambda: K.batch_mix(x, lam_mix, box0), a.reps)
    res["a_mixup"]["tb_per_s"] = tbs(2 * nbytes, res["a_mixup"])

    # (b) typical CutMix: lam = 0.5 -> a box of int(S sqrt(0.5)) pixels a side at the centre
    side = int(S * (0.5 ** 0.5))
    lo, hi = S // 2 - side // 2, S // 2 + side // 2
    box = torch.tensor([[lo, hi, lo, hi]] * B, dtype=torch.int32, device=dev)
    lam_cut = torch.full((B,), 1.0 - (hi - lo) ** 2 / float(S * S), device=dev)
    groups = (hi - 1) // 4 - lo // 4 + 1 if S % 4 == 0 else (hi - lo + 3) // 4      # 16-byte groups a box line meets
    moved = 2 * B * 3 * (hi - lo) * groups * 16
    res["b_cutmix"] = timed(lambda: K.batch_mix(x, lam_cut, box), a.reps)
    res["b_cutmix"]["box"] = [lo, hi, lo, hi]
    res["b_cutmix"]["moved_mb"] = round(moved / 1e6, 1)
    res["b_cutmix"]["tb_per_s"] = tbs(moved, res["b_cutmix"])

    # (c) the torch formulation
    res["c_torch_mixup"] = timed(lambda: x.mul_(0.3).add_(x.flip(0), alpha=0.7), a.reps)
    res["c_torch_mixup"]["tb_per_s_useful"] = tbs(2 * nbytes, res["c_torch_mixup"])
    res["a_over_c"] = round(res["a_mixup"]["median_us"] / res["c_torch_mixup"]["median_us"], 3)
    res["b_over_c"] = round(res["b_cutmix"]["median_us"] / res["c_torch_mixup"]["median_us"], 3)

    if a.step:
        import bench
        pkg.set_compute_dtype("bf16")
        model = bench.build_model(pkg, "cfg2", dev, 0.0).train()
        T = pkg.train
        opt = T.FusedAdamW(T.param_groups(model, lr=1e-4), lr=1e-4, weight_decay=0.05, distributed=False)
        x.normal_()
        y = torch.randint(0, 10, (B,), device=dev)
        res["step_plain"] = timed(lambda: T.train_step(model, x, y, opt), a.reps, warmup=3)

        def mixed_step():
            K.batch_mix(x, lam_mix, box0)
            T.train_step(model, x, y, opt, mix_lam=lam_mix)
        res["step_mixup"] = timed(mixed_step, a.reps, warmup=3)
        res["step_mixup_minus_plain_us"] = round(res["step_mixup"]["median_us"] - res["step_plain"]["median_us"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
