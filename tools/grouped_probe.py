#!/usr/bin/env python3
"""Grouped weight-gradient launch (dW = dY^T X of the four Linear layers of a block, for NB blocks in one launch) at
the benchmark shapes.  One process per setting (the library reads its knobs once):
    FAVIT_GROUPED_S=n   force n K-splits          NB=4      blocks per launch (default 1)
    CFG=cfg2|cfg4|cfg3|cfg1                        FAVIT_LIB=path   another build of the library (A/B against HEAD)
    FAVIT_GEMM_DBG=1    probe build: main loop only (no epilogue; timing only)
    ROWS=5,11,17;41,47  ragged groups (round 8): one launch per ';'-separated group, a block of BATCH (default 256) x rows
                        tokens per entry, through favit_gemm_grouped_tn_ragged; D from CFG (first name).  Prints every
                        group's launch time, its plan (favit_gemm_grouped_plan) and the same blocks launched one by one.
Prints the launch time, the time per block and the K-splits the library chose."""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
pkg = importlib.import_module("focused-attention-vit_amd")
if os.environ.get("FAVIT_LIB"):
    pkg._abi.LIB_PATH = os.path.abspath(os.environ["FAVIT_LIB"])
    import ctypes
    _probe = ctypes.CDLL(pkg._abi.LIB_PATH)
    for _n in list(pkg._abi._SIGS):                  # an older build: bind only what it exports
        if not hasattr(_probe, _n):
            del pkg._abi._SIGS[_n]
elif os.environ.get("FAVIT_GEMM_DBG"):
    pkg._abi.LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe_build", "libfavit_probe.so")
K = pkg.kernels
dev = "cuda"
CFGS = {"cfg2": (256 * 197, 384), "cfg4": (64 * 577, 768), "cfg3": (128 * 17, 384), "cfg1": (64 * 65, 192)}
NB = int(os.environ.get("NB", "1"))


def _time(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


if os.environ.get("ROWS"):
    import ctypes
    D = CFGS[os.environ.get("CFG", "cfg2").split(",")[0]][1]
    B = int(os.environ.get("BATCH", "256"))
    shapes = [(D, 4 * D), (4 * D, D), (D, D), (3 * D, D)]
    for grp in os.environ["ROWS"].split(";"):
        rows = [int(r) for r in grp.split(",")]
        blocks = [[(torch.randn(B * r, N, device=dev).bfloat16(), torch.randn(B * r, Kd, device=dev).bfloat16(),
                    torch.zeros(N, Kd, device=dev), torch.zeros(N, device=dev), True) for N, Kd in shapes] for r in rows]
        probs = [p for b in blocks for p in b]
        assert K.gemm_grouped_tn_ragged(probs)
        us = _time(lambda: K.gemm_grouped_tn_ragged(probs))
        each = [_time(lambda b=b: K.gemm_grouped_tn(b)) for b in blocks]
        ksteps = sum(B * r // 32 for r in rows)
        print(f"rows {rows} x {B}, D={D}: one ragged launch {us:.1f} us ({us / ksteps * 8:.3f} us per k-step of a 512-slot round); "
              f"block by block {sum(each):.1f} us ({', '.join(f'{e:.0f}' for e in each)})", flush=True)
    sys.exit(0)

for name in os.environ.get("CFG", "cfg2,cfg4").split(","):
    T, D = CFGS[name]
    shapes = [(D, 4 * D), (4 * D, D), (D, D), (3 * D, D)]
    probs = []
    for _ in range(NB):
        for N, Kd in shapes:
            probs.append((torch.randn(T, N, device=dev).bfloat16(), torch.randn(T, Kd, device=dev).bfloat16(),
                          torch.zeros(N, Kd, device=dev), torch.zeros(N, device=dev), True))
    old = "favit_gemm_grouped_last_splits" not in pkg._abi._SIGS
    chunks = [probs[i:i + 4] for i in range(0, len(probs), 4)] if (old or os.environ.get("PER_BLOCK")) else [probs]
    for _ in range(3):
        for c in chunks:
            assert K.gemm_grouped_tn(c)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    e0.record()
    for _ in range(reps):
        for c in chunks:
            K.gemm_grouped_tn(c)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    fl = NB * sum(2.0 * T * n * k for n, k in shapes)
    sp = "?" if old else int(pkg._abi.lib().favit_gemm_grouped_last_splits())
    print(f"{name}: T={T} D={D} blocks/launch={NB if len(chunks) == 1 else 1} (x{len(chunks)} launches) splits={sp}: "
          f"{us:.1f} us = {us / NB:.1f} us per block, {fl / us / 1e6:.0f} TF", flush=True)
