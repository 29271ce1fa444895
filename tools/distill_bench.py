#!/usr/bin/env python3
"""What knowledge distillation costs.  Two parts, one JSON line.

Kernels, at (B, C) = (256, 10), (256, 1000), (1024, 1000), label smoothing 0.1, mixed targets, with dlogits:
  mix          favit_cross_entropy_mix: the loss launch of before, which reads one row per sample
  soft, hard   favit_cross_entropy_distill (alpha 0.5, tau 3): the same plus the teacher's row
  soft_stream, hard_stream, soft_regs, hard_regs   the same entry point of the PROBE build (make -C .../csrc probe) with
               FAVIT_DISTILL_DBG=stream, which walks every row in memory, and =regs, which holds every row of C <= 1024 in
               registers (the library chooses by C).  Only when tools/probe_build/libfavit_probe.so exists.
  torch        the same loss and gradient composed from torch ops (log_softmax, one_hot, kl_div, autograd)
Every arm is captured as --launches back-to-back calls in one HIP graph and timed with HIP events around a replay, so the
figure is device time per call including the gap between two dependent kernels, without the host's launch path; the
arms alternate over --repeats.  `eager_us` is the host-inclusive time of one call from Python, for the new wrapper and
for the torch composition.

Steps, cfg2 (ViT-MHLA-Small, bf16, 256 images, the pruned CLS-only step): without a teacher, eager and graphed; with a
dense VisionTransformer teacher of the student's size (Distill(0.5, 3.0)), eager and graphed.  As tools/drop_path_bench.py:
one process, the arms alternate, HIP events around --steps consecutive steps.

    python tools/distill_bench.py [--steps 50] [--repeats 3] [--launches 200] [--shapes 256x10,...] [--skip_steps]"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import torch


def summarise(vals):
    return {"runs": [round(v, 3) for v in vals], "median": round(statistics.median(vals), 3),
            "spread": round(max(vals) - min(vals), 3)}


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters, out


def graph_of(fn, launches):
    """`launches` calls of fn captured in one graph (after a warm-up on a side stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def kernel_part(pkg, a, dev, probe):
    K, abi = pkg.kernels, pkg._abi
    lib = abi.lib()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    eps, alpha, tau = 0.1, 0.5, 3.0
    out = {}
    for B, Cn in a.shapes:
        g = torch.Generator(device=dev).manual_seed(B + Cn)
        x = torch.randn(B, Cn, device=dev, generator=g) * 3
        z = torch.randn(B, Cn, device=dev, generator=g) * 3
        y = torch.randint(0, Cn, (B,), device=dev, generator=g)
        lam = torch.rand(B, device=dev, generator=g)
        rows, kd, dlog = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, Cn, device=dev)

        def mix():
            abi.check(lib.favit_cross_entropy_mix(P(x), P(y), P(lam), P(rows), P(dlog), B, Cn, 1.0 / B, eps, st()), "mix")

        def distill(l, hard, env=None):
            def run():
                if env is None:
                    os.environ.pop("FAVIT_DISTILL_DBG", None)
                else:
                    os.environ["FAVIT_DISTILL_DBG"] = env
                abi.check(l.favit_cross_entropy_distill(P(x), P(z), P(y), P(lam), P(rows), P(kd), P(dlog), B, Cn, 1.0 / B,
                                                        eps, alpha, tau, hard, st()), "distill")
            return run

        xg = x.clone().requires_grad_(True)

        def torch_comp():
            F_ = torch.nn.functional
            hot = F_.one_hot(y, Cn).float()
            t = (1.0 - eps) * (lam[:, None] * hot + (1.0 - lam)[:, None] * hot.flip(0)) + eps / Cn
            base = -(t * torch.log_softmax(xg, 1)).sum(1)
            kl = F_.kl_div(torch.log_softmax(xg / tau, 1), torch.log_softmax(z / tau, 1), reduction="none",
                           log_target=True).sum(1) * (tau * tau)
            loss = ((1.0 - alpha) * base + alpha * kl).mean()
            return loss, torch.autograd.grad(loss, xg)[0]

        arms = {"mix": mix, "soft": distill(lib, 0), "hard": distill(lib, 1), "torch": torch_comp}
        if probe is not None:
            arms.update({"soft_regs": distill(probe, 0, "regs"), "soft_stream": distill(probe, 0, "stream"),
                         "hard_regs": distill(probe, 1, "regs"), "hard_stream": distill(probe, 1, "stream")})
        graphs = {k: graph_of(f, a.launches) for k, f in arms.items()}
        os.environ.pop("FAVIT_DISTILL_DBG", None)
        us = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, gr in graphs.items():
                gr.replay()
                ms, _ = timed_ms(gr.replay, 5)
                us[k].append(ms * 1e3 / a.launches)
        # the fused launch and the composition agree (the figures compare like with like)
        arms["soft"]()
        ref_loss, ref_grad = torch_comp()
        err = ((dlog - ref_grad).norm() / ref_grad.norm()).item()
        res = {"us_per_call_graph_replayed": {k: summarise(v) for k, v in us.items()},
               "fused_vs_torch": {"loss": [rows.mean().item(), ref_loss.item()], "dlogits_rel_l2": err},
               "bytes_moved": {"mix": 2 * 4 * B * Cn, "distill": 3 * 4 * B * Cn}}
        eager = {"distill_wrapper": lambda: K.cross_entropy_distill(x, z, y, 1.0 / B, eps, lam, alpha, tau),
                 "mix_wrapper": lambda: K.cross_entropy(x, y, 1.0 / B, eps, lam), "torch": torch_comp}
        res["eager_us"] = {}
        for k, f in eager.items():
            timed_ms(f, 20)
            res["eager_us"][k] = summarise([timed_ms(f, 200)[0] * 1e3 for _ in range(a.repeats)])
        out[f"B{B}_C{Cn}"] = res
    return out


def step_part(pkg, a, dev):
    import bench
    T = pkg.train
    pkg.set_compute_dtype("bf16")
    c = bench.CONFIGS["cfg2"]
    B = a.batch or c["batch"]
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(B, 3, c["img"], c["img"], device=dev, generator=g)
    labels = torch.randint(0, c["classes"], (B,), device=dev, generator=g)
    d = T.Distill(0.5, 3.0)

    def arm(with_teacher, graphed):
        torch.manual_seed(1234)
        model = bench.build_model(pkg, "cfg2", dev, 0.0).train()
        teacher = None
        if with_teacher:
            torch.manual_seed(4321)
            teacher = pkg.models.vit.VisionTransformer(img_size=c["img"], patch_size=16, num_classes=c["classes"],
                                                       embed_dim=384, depth=12, num_heads=6).to(dev).eval()
            for p in teacher.parameters():
                p.requires_grad = False
        opt = T.FusedAdamW(T.param_groups(model, lr=1e-4), lr=1e-4, weight_decay=0.05)
        kw = dict(teacher=teacher, distill=d) if with_teacher else {}
        if graphed:
            gs = T.GraphedStep(model, opt, images, labels, static_inputs=True, **kw)
            step = lambda: gs(images, labels)
        else:
            gs = None
            step = lambda: T.train_step(model, images, labels, opt, **kw)
        return {"step": step, "keep": (model, teacher, opt, gs), "ms": [], "loss": None}

    arms = {}
    for graphed in (False, True):
        for with_teacher in (False, True):
            arms[("graph" if graphed else "eager") + ("_teacher" if with_teacher else "_plain")] = arm(with_teacher, graphed)
    for _ in range(a.repeats):
        for r in arms.values():
            timed_ms(r["step"], a.warmup)
            ms, loss = timed_ms(r["step"], a.steps)
            r["ms"].append(ms)
            r["loss"] = float(loss.detach())
    res = {"config": "cfg2", "dtype": "bf16", "batch": B, "steps": a.steps, "warmup": a.warmup, "arms": {}}
    for name, r in arms.items():
        res["arms"][name] = dict(summarise(r["ms"]), last_loss=r["loss"])
    for kind in ("eager", "graph"):
        res[kind + "_teacher_minus_plain_ms"] = round(res["arms"][kind + "_teacher"]["median"] -
                                                      res["arms"][kind + "_plain"]["median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200, help="calls per captured graph in the kernel part")
    ap.add_argument("--shapes", default="256x10,256x1000,1024x1000", help="kernel part: BxC,BxC,...")
    ap.add_argument("--batch", type=int, default=0, help="images per step (default: cfg2's 256)")
    ap.add_argument("--skip_steps", action="store_true", help="the kernel part only")
    ap.add_argument("--skip_kernels", action="store_true", help="the step part only")
    a = ap.parse_args()
    a.shapes = [tuple(int(v) for v in s_.split("x")) for s_ in a.shapes.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench needs the GPU: nothing here can be measured on the host")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    pkg = importlib.import_module("focused-attention-vit_amd")
    dev = torch.device("cuda", 0)
    probe = None
    probe_path = os.path.join(root, "tools", "probe_build", "libfavit_probe.so")
    if os.path.exists(probe_path):
        probe = ctypes.CDLL(probe_path)
        probe.favit_cross_entropy_distill.argtypes = pkg._abi._SIGS["favit_cross_entropy_distill"][0]
        probe.favit_cross_entropy_distill.restype = ctypes.c_int
    res = {"tool": "distill_bench", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "launches": a.launches,
           "probe_build": probe is not None}
    if not a.skip_kernels:
        res["kernels"] = kernel_part(pkg, a, dev, probe)
    if not a.skip_steps:
        res["steps"] = step_part(pkg, a, dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
