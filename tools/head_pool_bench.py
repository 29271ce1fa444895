#!/usr/bin/env python3
"""What the mean-pooled head costs.

1. The head alone, forward + backward, fused (csrc/head_pool.hip) against the composition the library offered before it
   -- norm-first: favit_layernorm_fwd on all rows, a torch mean, an expand and favit_layernorm_bwd on all rows;
   pool-first: a torch mean, the LayerNorm pair on the B pooled rows and an expand -- at the cfg2 size (B = 256, L = 197,
   D = 384) and the cfg4 size (B = 64, L = 577, D = 768).  The arms alternate inside every repeat; a window is --iters
   back-to-back calls between two HIP events, after --warmup calls.  Both arms read the same resident x (77 / 113 MB:
   it fits the 256 MB last-level cache, as the encoder's freshly written output largely does in a real step).
2. The cfg2 training step (ViT-MHLA-Small, bf16, 256 images, HIP-graph replayed) with the CLS head as bench.py times it
   (pruned), with the CLS head and FAVIT_NO_PRUNE=1 (all rows computed), and with set_global_pool('avg') (all rows
   computed AND read by the head).

Prints one JSON line.

    python tools/head_pool_bench.py [--iters 1000] [--steps 30] [--repeats 3] [--no-step]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters, out


def summary(xs, digits):
    return {"runs": [round(v, digits) for v in xs], "median": round(statistics.median(xs), digits),
            "spread": round(max(xs) - min(xs), digits)}


def head_arms(K, B, L, D, dev):
    g = torch.Generator(device=dev).manual_seed(B + L + D)
    x = torch.randn((B, L, D), device=dev, generator=g) * 1.7 + 0.3
    gamma = 1 + 0.2 * torch.randn(D, device=dev, generator=g)
    beta = 0.3 * torch.randn(D, device=dev, generator=g)
    dy = torch.randn((B, D), device=dev, generator=g)
    n, x2 = L - 1, x.view(B * L, D)

    def fused_norm_first():
        y, s, mu, rs = K.ln_meanpool_fwd(x, gamma, beta)
        return K.ln_meanpool_bwd(dy, x, gamma, s, mu, rs)[0]

    def composed_norm_first():
        rows, mu, rs = K.layernorm_fwd(x2, D, gamma, beta, B * L, D, torch.float32)
        y = rows.view(B, L, D)[:, 1:].mean(1)
        up = torch.zeros((B, L, D), device=dev)
        up[:, 1:] = (dy / n)[:, None, :]
        return K.layernorm_bwd(up.view(B * L, D), x2, D, gamma, mu, rs, B * L, D)[0]

    def fused_pool_first():
        p = K.meanpool_fwd(x)
        y, mu, rs = K.layernorm_fwd(p, D, gamma, beta, B, D, torch.float32)
        return K.meanpool_bwd(K.layernorm_bwd(dy, p, D, gamma, mu, rs, B, D)[0], L)

    def composed_pool_first():
        p = x[:, 1:].mean(1)
        y, mu, rs = K.layernorm_fwd(p, D, gamma, beta, B, D, torch.float32)
        dp = K.layernorm_bwd(dy, p, D, gamma, mu, rs, B, D)[0]
        dx = torch.zeros((B, L, D), device=dev)
        dx[:, 1:] = (dp / n)[:, None, :]
        return dx

    return {"norm_first_fused": fused_norm_first, "norm_first_composed": composed_norm_first,
            "pool_first_fused": fused_pool_first, "pool_first_composed": composed_pool_first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--step_warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="time the head only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_pool_bench needs the GPU: nothing here can be measured on the host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("focused-attention-vit_amd")
    import bench
    K, dev = pkg.kernels, torch.device("cuda", 0)
    res = {"tool": "head_pool_bench", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "repeats": a.repeats, "head_us": {}, "step_ms": {}}
    for name, (B, L, D) in (("cfg2", (256, 197, 384)), ("cfg4", (64, 577, 768))):
        arms = head_arms(K, B, L, D, dev)
        runs = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, fn in arms.items():
                runs[k].append(1e3 * timed(fn, a.warmup, a.iters)[0])
        out = {k: summary(v, 2) for k, v in runs.items()}
        # bytes the algorithm has to move per direction pair (x read twice, dx written once) over the fused time
        gb = 3 * B * L * D * 4 / 1e9
        out["shape"] = [B, L, D]
        out["norm_first_fused_GBps"] = round(gb / (out["norm_first_fused"]["median"] * 1e-6), 1)
        res["head_us"][name] = out
        del arms
        torch.cuda.empty_cache()
    if not a.no_step:
        pkg.set_compute_dtype("bf16")
        c = bench.CONFIGS["cfg2"]
        g = torch.Generator(device=dev).manual_seed(1234)
        images = torch.randn(c["batch"], 3, c["img"], c["img"], device=dev, generator=g)
        labels = torch.randint(0, c["classes"], (c["batch"],), device=dev, generator=g)

        def arm(pool, no_prune):
            torch.manual_seed(1234)
            model = bench.build_model(pkg, "cfg2", dev, 0.0).train().set_global_pool(pool)
            opt = pkg.train.FusedAdamW(pkg.train.param_groups(model, lr=1e-4), lr=1e-4, weight_decay=0.05)
            if no_prune:
                os.environ["FAVIT_NO_PRUNE"] = "1"             # read while the step is captured
            try:
                gs = pkg.train.GraphedStep(model, opt, images, labels, static_inputs=True)
            finally:
                os.environ.pop("FAVIT_NO_PRUNE", None)
            return gs, (model, opt)

        steps = {"token_pruned": arm("token", False), "token_no_prune": arm("token", True), "avg": arm("avg", False)}
        runs, loss = {k: [] for k in steps}, {}
        for _ in range(a.repeats):
            for k, (gs, _) in steps.items():
                ms, last = timed(lambda: gs(images, labels), a.step_warmup, a.steps)
                runs[k].append(ms)
                loss[k] = float(last.detach())
        res["step_ms"] = {k: dict(summary(v, 3), last_loss=loss[k]) for k, v in runs.items()}
        res["step"] = {"config": "cfg2", "dtype": "bf16", "batch": c["batch"], "steps": a.steps, "graphed": True}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
