#!/usr/bin/env python
"""A validation pass three ways: how long does the host need to ISSUE a batch, and how long does the device need to run
it?  

    python tools/eval_bench.py [--configs cfg2 cfg3] [--batches 10] [--rounds 5] [--warmup 2]

The pass is `batches` batches resident on the device (one synthetic batch of the configuration's size, repeated), in
bf16, through
  today     harness.evaluate(model, loader): three torch launches and a loss launch per batch for the statistics, and
            one host sync per batch
  eager     harness.evaluate(model, loader, metrics=EvalMetrics): the forward and the two launches of
            favit_eval_metrics per batch, one sync per pass
  graphed   the same with graph=: one HIP-graph replay per batch (harness.GraphedEval, captured once, outside the timing)
Conventions of tools/host_enqueue.py.  Per round and mode: time.perf_counter() around the pass up to its last launch
gives the host-issue time (for `today` the host is blocked once per batch, so this IS its wall time; for the other two
the loop of the pass is run here without its final read), HIP events around the same launches the device time, and
perf_counter around the whole pass with its read-out the wall time; all per batch.  The rounds alternate between the
modes in ONE process, so all three see the same machine state.  Prints one JSON line per configuration."""
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
    H = pkg.harness
    c = bench.CONFIGS[cfg]
    torch.manual_seed(1234)
    model = bench.build_model(pkg, cfg, dev)
    B = c["batch"]
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(B, 3, c["img"], c["img"], device=dev, generator=g)
    labels = torch.randint(0, c["classes"], (B,), device=dev, generator=g)
    if cfg in ("cfg3", "cfg5"):                      # label maps are input data here, as in bench.py
        maps = bench.synthetic_label_maps(8, 224, 16, seed=100)
        model.segmentation.set_label_maps(torch.from_numpy(np.stack([maps[i % 8] for i in range(B)])).to(dev))
        model.assume_num_tokens = 16
    model.eval()
    loader = [(images, labels)] * args.batches
    metrics = {m: H.EvalMetrics(c["classes"], topk=(1, 5)) for m in ("eager", "graphed")}
    graphed = H.GraphedEval(model, images, labels, metrics["graphed"])

    def issue(mode):
        """The launches of one pass, without its read-out."""
        if mode == "today":
            return H.evaluate(model, loader)
        with torch.no_grad():
            for x, y in loader:
                if mode == "eager":
                    metrics[mode].update(model(x), y)
                else:
                    graphed(x, y)

    def whole(mode):
        if mode == "today":
            return H.evaluate(model, loader)
        metrics[mode].reset()
        return H._evaluate_metrics(model, loader, None, metrics[mode], graphed if mode == "graphed" else False, None)[0]

    modes = ["today", "eager", "graphed"]
    res = {m: {"enqueue_ms": [], "device_ms": [], "wall_ms": []} for m in modes}
    accs = {}
    for m in modes:
        for _ in range(args.warmup):
            accs[m] = whole(m)["test_acc"]
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for m in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            issue(m)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            res[m]["enqueue_ms"].append(1e3 * (t1 - t0) / args.batches)
            res[m]["device_ms"].append(e0.elapsed_time(e1) / args.batches)
            t0 = time.perf_counter()
            whole(m)
            torch.cuda.synchronize()
            res[m]["wall_ms"].append(1e3 * (time.perf_counter() - t0) / args.batches)
    out = {"tool": "eval_bench", "config": cfg, "batch": B, "batches": args.batches, "rounds": args.rounds,
           "host_syncs_per_pass": {"today": args.batches, "eager": 1, "graphed": 1}, "test_acc": accs,
           "knobs": bench.active_knobs()}
    for m in modes:
        out[m] = {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                  for k, v in res[m].items()}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2", "cfg3"], choices=["cfg1", "cfg2", "cfg3", "cfg4"])
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pkg = importlib.import_module("focused-attention-vit_amd")
    pkg._abi.lib()
    pkg.set_compute_dtype("bf16")
    for cfg in args.configs:
        run_config(pkg, cfg, args, dev)
        pkg.functional.clear_lp_mirrors()


if __name__ == "__main__":
    main()
