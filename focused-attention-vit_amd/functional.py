"""Forward/backward chains of the encoder hot path, built on the HIP kernels.

Each ``*Op`` below restates one reference forward (cited per class) as a sequence of
libfavit kernel launches and supplies the hand-written backward sequence.  ``OpFn`` is
the single ``torch.autograd.Function`` that plugs an Op into autograd so that the
``nn.Module`` mirrors in ``models/`` stay drop-in (``loss.backward()`` works unchanged).

Data layout in HBM: the residual stream is fp32 ``[B*L, D]``; every GEMM
operand is a contiguous row-major ``[rows, features]`` matrix in the compute dtype (bf16
or fp32); q, k~, v~ live interleaved in one ``[B*L, 3D]`` buffer exactly as the fused qkv
projection writes them; gradients of the residual stream are kept in fp32 plus a
compute-dtype copy that feeds the backward GEMMs.
"""
from __future__ import annotations

import contextlib
import math
import os
import weakref
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import torch

from . import kernels as K
from ._abi import ACT_DGELU, ACT_GELU, ACT_GELU_SAVEGRAD, ACT_MULAUX, ACT_NONE

# ------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------
_STATE = {"cdt": torch.float32, "epoch": 0, "direct_grads": True, "grad_ready": None}


def set_direct_grads(on: bool) -> None:
    """When on (default), parameter gradients are accumulated by the kernels straight into an
    existing fp32 ``param.grad`` buffer (split-K atomics / fused reductions write there anyway),
    and autograd gets ``None`` for those parameters: no temporary gradient tensors, no zero-fill,
    no ``grad += g`` pass.  Parameters without a ``.grad`` buffer get ordinary returned grads."""
    _STATE["direct_grads"] = bool(on)


def set_grad_ready_hook(fn) -> None:
    """fn(param) is called after a parameter's gradient was accumulated directly (dp.GradSync)."""
    _STATE["grad_ready"] = fn


def _gt(p):
    """The gradient buffer of parameter p that kernels may accumulate into, or None."""
    if p is None or not _STATE["direct_grads"] or not getattr(p, "requires_grad", False):
        return None
    g = p.grad
    if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or not g.is_cuda:
        return None
    return g


def _ready(*params):
    fn = _STATE["grad_ready"]
    if fn is not None:
        for p in params:
            if p is not None:
                if _SIDE["active"]:
                    _SIDE["pending"].append(p)       # gradient lives on the side stream: notify after the join
                else:
                    fn(p)


# ------------------------------------------------------------------------------------
# Optional side stream for weight-gradient GEMMs (dW = dY^T.X does not feed the backward chain).
# Measured on MI355X it bought nothing for this workload (21.42 vs 21.35 ms/step: every GEMM already
# fills the chip), so it is OFF by default; kept because it is the natural hook for overlapping the
# DP all-reduce of early buckets with compute on multi-GPU runs.  Also measured: the small latency-bound
# latent_proj fold kernels (36 per step, 15-40 us) moved to this stream (forward folds launched up
# front, backward folds under the LayerNorm backward) -- no gain either (18.7 vs 18.3 ms/step): every
# cross-stream dependency costs a barrier packet of several microseconds, about what the overlap saves.
# ------------------------------------------------------------------------------------
_SIDE = {"enabled": False, "stream": None, "active": False, "pending": [], "used": False}


def set_side_stream(on: bool) -> None:
    _SIDE["enabled"] = bool(on)


class _side_stream:
    """with _side_stream(t1, t2, ...): launches inside run on the side stream after everything
    already queued on the current stream; the tensors are marked as used by it."""

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if t is not None]

    def __enter__(self):
        if not _SIDE["enabled"]:
            self.ctx = None
            return self
        if _SIDE["stream"] is None:
            _SIDE["stream"] = torch.cuda.Stream()
        s = _SIDE["stream"]
        s.wait_stream(torch.cuda.current_stream())
        for t in self.tensors:
            t.record_stream(s)
        self.ctx = torch.cuda.stream(s)
        self.ctx.__enter__()
        _SIDE["active"] = True
        _SIDE["used"] = True
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            _SIDE["active"] = False
            self.ctx.__exit__(*exc)
        return False


def join_side_stream() -> None:
    """Current stream waits for the side stream; deferred gradient-ready notifications fire."""
    if _SIDE["used"]:
        torch.cuda.current_stream().wait_stream(_SIDE["stream"])
        _SIDE["used"] = False
    if _SIDE["pending"]:
        fn = _STATE["grad_ready"]
        pend, _SIDE["pending"] = _SIDE["pending"], []
        if fn is not None:
            for p in pend:
                fn(p)


def set_compute_dtype(d) -> None:
    """'fp32' (exact f32 MFMA path, the parity mode), 'fp32x3' (fp32 storage and fp32 everywhere except the inner
    product of the large GEMMs, which is the three-pass split-bf16 product FAVIT_F32X3 of include/favit.h: about
    4e-6 per GEMM against 4e-7, inside every fp32-mode tolerance), 'bf16' (bf16 MFMA, fp32 accumulate) or 'fp8'
    (BASELINE.json configs[3]: the nn.Linear GEMMs of the encoder blocks run on fp8 MFMA -- e4m3
    activations / weights, e5m2 gradients, per-tensor scales taken on the device -- everything else as
    in 'bf16'; patch embedding and classifier head stay bf16).
    With FAVIT_FP32_GEMM=x3 in the environment (read at each call) 'fp32' selects 'fp32x3': unlike the
    kernel-selection switches this one changes results."""
    fp8 = x3 = False
    if isinstance(d, str):
        fp8 = d == "fp8"
        x3 = d == "fp32x3"
        d = {"fp32": torch.float32, "float32": torch.float32, "fp32x3": torch.float32, "bf16": torch.bfloat16,
             "bfloat16": torch.bfloat16, "fp8": torch.bfloat16}[d]
    if d not in (torch.float32, torch.bfloat16):
        raise ValueError("compute dtype must be fp32, fp32x3, bf16 or fp8")
    if d == torch.float32 and os.environ.get("FAVIT_FP32_GEMM") == "x3":
        x3 = True
    _STATE["cdt"] = d
    _STATE["fp8"] = fp8
    _STATE["x3"] = x3
    K.set_f32_gemm_split(x3)


def get_compute_mode() -> str:
    if _STATE.get("fp8"):
        return "fp8"
    if _STATE["cdt"] == torch.bfloat16:
        return "bf16"
    return "fp32x3" if _STATE.get("x3") else "fp32"


def get_compute_dtype() -> torch.dtype:
    return _STATE["cdt"]


def bump_weight_epoch(synced_mirrors=()) -> None:
    """Called by optimizers that update parameters through raw pointers.  synced_mirrors: the bf16
    mirrors the caller has just rewritten itself (they stay valid across the bump)."""
    _STATE["epoch"] += 1
    for m in synced_mirrors:
        m.epoch = _STATE["epoch"]


# parameter storage -> (fp32 flat buffer, bf16 mirror) kept fresh by the fused optimizer (train.FusedAdamW)
class _LPMirror:
    """bf16 mirror ``lp`` of the flat fp32 parameter buffer ``flat_p`` of one optimizer group.

    The owner (train.FusedAdamW) rewrites it inside the AdamW kernel and tells the mirror so
    (``mark_synced``).  Every other way of editing a parameter is detected when the parameter is next
    used: ``load_state_dict`` / ``nn.init.*`` / ``p.copy_`` bump the tensor's version counter (compared
    per parameter), ``invalidate_weight_cache()`` bumps the weight epoch (compared per mirror; needed
    for ``p.data.copy_``, which no counter sees).  A stale slice / mirror is re-cast before it is returned."""
    __slots__ = ("flat_ref", "lp", "epoch", "versions", "params")

    def __init__(self, flat_p, lp, params=()):
        self.flat_ref, self.lp, self.params = weakref.ref(flat_p), lp, [weakref.ref(p) for p in params]
        self.mark_synced()

    def mark_synced(self):
        """The owner has just rewritten the whole mirror from flat_p (AdamW kernel or a cast): every
        parameter's current version counter is the one the mirror reflects."""
        self.epoch = _STATE["epoch"]
        self.versions = {id(p): p._version for p in (r() for r in self.params) if p is not None}

    def refresh_if_stale(self) -> bool:
        """Host-side check for callers that cannot check at use time (a replayed HIP graph reads the mirror without
        going through lookup): re-cast the whole mirror if any parameter was edited since it was last written."""
        fp = self.flat_ref()
        if fp is None:
            return False
        stale = self.epoch != _STATE["epoch"]
        if not stale:
            for r in self.params:
                p = r()
                if p is not None and self.versions.get(id(p), p._version) != p._version:
                    stale = True
                    break
        if stale:
            K.cast(fp, torch.bfloat16, out=self.lp)
            self.mark_synced()
        return stale

    def lookup(self, src, w):
        fp = self.flat_ref()
        if fp is None:
            return None
        base, ptr = fp.data_ptr(), w.data_ptr()
        if not (base <= ptr < base + 4 * fp.numel()):
            return False
        if self.epoch != _STATE["epoch"]:                 # explicit invalidation: refresh the whole mirror once
            K.cast(fp, torch.bfloat16, out=self.lp)
            self.epoch = _STATE["epoch"]
        off = (ptr - base) // 4
        view = self.lp[off:off + w.numel()].view(w.shape)
        key = id(src)
        ver = src._version
        if self.versions.get(key, ver) != ver:            # edited in place since the last use: re-cast this slice
            K.cast(w, torch.bfloat16, out=view)
        self.versions[key] = ver
        return view


_LP_MIRRORS: List[_LPMirror] = []


def register_lp_mirror(flat_p: torch.Tensor, flat_lp: torch.Tensor, params=()) -> _LPMirror:
    """flat_lp is a bf16 mirror of the fp32 parameter buffer flat_p, just cast from it; params are the
    nn.Parameters living in flat_p (see _LPMirror)."""
    m = _LPMirror(flat_p, flat_lp, params)
    _LP_MIRRORS.append(m)
    return m


def clear_lp_mirrors() -> None:
    _LP_MIRRORS.clear()


def invalidate_weight_cache() -> None:
    """Drop every cached compute-dtype copy of a parameter (per-tensor caches and the fused optimizer's
    bf16 mirrors alike).  Needed only after editing parameters through ``.data`` (``p.data.copy_(...)``),
    which autograd's version counter cannot see; ``load_state_dict``, ``nn.init.*``, ``p.copy_`` and
    optimizer steps are detected automatically."""
    _STATE["epoch"] += 1


def wcast(w: torch.Tensor) -> torch.Tensor:
    """Parameter in the compute dtype.  The copy is cached ON the tensor object that was passed in
    (so it dies with the parameter: another model whose weights later reuse the same address can
    never see it) and is tagged with (address, version counter, weight epoch, dtype)."""
    cdt = _STATE["cdt"]
    src = w
    w = w.detach()
    if w.dtype == cdt and w.is_contiguous():
        return w
    if cdt == torch.bfloat16 and w.dtype == torch.float32 and w.is_contiguous():
        for m in list(_LP_MIRRORS):
            hit = m.lookup(src, w)
            if hit is None:                   # the optimizer that owned this mirror is gone
                _LP_MIRRORS.remove(m)
            elif hit is not False:
                return hit
    tag = (w.data_ptr(), tuple(w.shape), w._version, _STATE["epoch"], cdt)
    hit = getattr(src, "_favit_cast", None)
    if hit is not None and hit[0] == tag:
        return hit[1]
    c = K.cast(w, cdt)
    try:
        src._favit_cast = (tag, c)
    except AttributeError:                    # pragma: no cover  (objects without a __dict__)
        pass
    return c


def set_dropout_epoch(word: Optional[torch.Tensor]) -> None:
    """Register (or, with None, clear) the device word every dropout-drawing kernel mixes into its seed at execution
    time (favit_set_dropout_epoch): a one-element int64 tensor on the current device that the caller increments once per
    step.  With it, dropout seeds frozen into a captured HIP graph still give fresh masks at every replay."""
    if word is not None:
        K.require_gpu(word)
        if word.dtype != torch.int64 or word.numel() != 1:
            raise TypeError("the dropout epoch is a one-element int64 device tensor")
    _STATE["drop_epoch"] = word
    from . import _abi
    _abi.check(_abi.lib().favit_set_dropout_epoch(None if word is None else word.data_ptr()), "favit_set_dropout_epoch")


def get_dropout_epoch() -> Optional[torch.Tensor]:
    return _STATE.get("drop_epoch")


def _seed() -> int:
    # drawn from torch's CPU generator: reproducible under torch.manual_seed, no device sync
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing() and _STATE.get("drop_epoch") is None:
        raise RuntimeError("dropout inside a captured HIP graph: the seed is a kernel argument and would be frozen "
                           "into the graph; register a dropout epoch word first (functional.set_dropout_epoch; "
                           "train.GraphedStep does it for models with dropout)")
    return int(torch.empty((), dtype=torch.int64).random_().item())


# Backward in segments (train.GraphedStep): models/vit.py::run_encoder splits the block stack into this many autograd
# nodes and reports the tensors between them.
_SEG = {"n": 1, "boundaries": []}


class encoder_segments:
    """with encoder_segments(n): forward passes split every encoder into n autograd nodes that are CUT APART: node k + 1
    reads a detached leaf copy of node k's output.  .boundaries collects the (output of node k, leaf input of node
    k + 1) pairs in forward order; backward then runs back to front, one autograd call per piece:
    backward(loss); backward(out_k, grad_tensors=in_{k+1}.grad) ... (train.GraphedStep)."""

    def __init__(self, n: int):
        self.n = max(1, int(n))

    def __enter__(self):
        self.prev = (_SEG["n"], _SEG["boundaries"])
        _SEG["n"], _SEG["boundaries"] = self.n, []
        self.boundaries = _SEG["boundaries"]
        return self

    def __exit__(self, *exc):
        _SEG["n"], _SEG["boundaries"] = self.prev
        return False


def get_encoder_segments() -> int:
    return _SEG["n"]


def note_segment_boundary(x: torch.Tensor) -> torch.Tensor:
    leaf = x.detach().requires_grad_(True)
    _SEG["boundaries"].append((x, leaf))
    return leaf


def _as_cdt(x: torch.Tensor) -> torch.Tensor:
    cdt = _STATE["cdt"]
    x = x.contiguous()
    return x if x.dtype == cdt else K.cast(x, cdt)


def _as_f32(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    return x if x.dtype == torch.float32 else K.cast(x, torch.float32)


def _mask_u8(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    return (mask != 0).to(torch.uint8).contiguous()


def _check_mask_shape(who: str, mask: Optional[torch.Tensor], form: str, shape) -> None:
    """An attention chain's mask must have the module's documented form: the kernels index it with those extents, so
    another rank or extent (a [B, L] key-keep mask handed to an MHLA module, say) would be read past its end."""
    if mask is None:
        return
    if not torch.is_tensor(mask) or tuple(mask.shape) != tuple(shape):
        got = tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__
        raise ValueError(f"{who}: the attention mask must be {form} = {tuple(shape)}, got {got}")


# ------------------------------------------------------------------------------------
# GEMM helpers (nn.Linear forward / backward)
# ------------------------------------------------------------------------------------
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


# Delayed scaling (fp8 mode): one amax history per quantisation site = (weight nn.Parameter of the Linear, operand
# role).  Callers that pass no site measure the amax of every tensor in a separate pass (as before).
_FP8_HIST = {}


def _fp8_hist(site, role: str):
    """site: a long-lived object that identifies the Linear (its weight nn.Parameter); None = no history."""
    if site is None or torch.cuda.is_current_stream_capturing():      # the slot rotation is host state
        return None
    key = (id(site), role)
    ent = _FP8_HIST.get(key)
    if ent is None or ent[0]() is not site:           # (weakref guards against a recycled id)
        ent = (weakref.ref(site), K.Fp8History(site.device))
        _FP8_HIST[key] = ent
        if len(_FP8_HIST) > 4096:                     # models come and go in a test process
            for k in [k for k, v in _FP8_HIST.items() if v[0]() is None]:
                del _FP8_HIST[k]
    return ent[1]


def _q8(t: torch.Tensor, fmt: torch.dtype, want_t: bool = False, hist=None):
    """(q, q_t or None, scale_inv) of a 2-D bf16 matrix, cached on the tensor object.  Activations and gradients are
    only needed row-major (forward and input-gradient GEMMs); the transposed copy is for weights (W^T of the
    input-gradient GEMM).  Weight-gradient GEMMs stay on the bf16 grouped launch: measured at ViT-Base, the fp8
    weight-gradient GEMMs (split-K with fp32 atomics, both operands quantised AND transposed first) cost 9.6 ms per
    step against 7.5 ms for the bf16 grouped launch + its reduction, before counting the transposing passes."""
    hit = getattr(t, "_favit_q8", None)
    if hit is not None and hit[0] == (fmt, t._version) and (hit[1][1] is not None or not want_t):
        return hit[1]
    q, qt, sinv = K.fp8_quantize(t, fmt, want=True, want_t=want_t, hist=hist)
    out = (q, qt, sinv)
    try:
        t._favit_q8 = ((fmt, t._version), out)
    except AttributeError:                    # pragma: no cover
        pass
    return out


def _q8_request(chain, prm, which: str, D: int):
    """fp8 mode: (fp8 dtype, amax history) of the GEMM operand that the tensor a LayerNorm pass is about to write will
    become -- `which` = "fwd": the chain's input (qkv / fc1 activations, e4m3), "bwd": the gradient of its output (the
    proj / fc2 input-gradient GEMM's dY, e5m2).  K.layernorm_fwd / _bwd then write the quantised copy in the same pass
    and park it where _q8 finds it (favit_layernorm_*_q8).  None: not fp8 mode, an unknown chain, a contraction the
    fp8 GEMM does not take, or no history (graph capture)."""
    if not _STATE.get("fp8") or get_compute_dtype() != torch.bfloat16 or D % 64 != 0 or os.environ.get("FAVIT_FP8_NO_LNQ8"):
        return None
    idx = getattr(chain, "q8_" + which, None)
    if idx is None or prm is None or idx >= len(prm) or prm[idx] is None:
        return None
    hist = _fp8_hist(prm[idx], "a" if which == "fwd" else "dy")
    return None if hist is None else ((E4M3 if which == "fwd" else E5M2), hist)


def _use_fp8(allow, *mats, k_dims=()):
    """fp8 GEMM applies: fp8 mode, bf16 row-major operands, contraction lengths multiples of 64."""
    if not (allow and _STATE.get("fp8")):
        return False
    return all(m.dtype == torch.bfloat16 and m.dim() == 2 and m.is_contiguous() for m in mats) and \
        all(k % 64 == 0 for k in k_dims)


def lin_fwd(a, w_c, bias, M, N, Kd, out_dtype, *, act=ACT_NONE, residual=None, want_pre=False, drop=(0.0, 0),
            allow_fp8=True, site=None):
    out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    pre = torch.empty((M, N), dtype=out_dtype, device=a.device) if want_pre else None
    if _use_fp8(allow_fp8, a, w_c, k_dims=(Kd,)):
        aq, _, sa = _q8(a, E4M3, hist=_fp8_hist(site, "a"))
        wq, _, sw = _q8(w_c, E4M3, want_t=True, hist=_fp8_hist(site, "w"))      # the backward wants W^T from the same pass
        K.gemm(aq, wq, out, M, N, Kd, Kd, Kd, N, bias=bias, act=act, aux_out=pre, ld_aux_out=N, residual=residual,
               ld_res=N, dropout_p=drop[0], dropout_seed=drop[1], scale_a=sa, scale_b=sw)
        return (out, pre) if want_pre else out
    K.gemm(a, w_c, out, M, N, Kd, Kd, Kd, N, bias=bias, act=act, aux_out=pre, ld_aux_out=N, residual=residual,
           ld_res=N, dropout_p=drop[0], dropout_seed=drop[1])
    return (out, pre) if want_pre else out


def lin_bwd_x(dy, w_c, M, N, Kd, out_dtype, *, dgelu_pre=None, pre_is_grad=False, drop=(0.0, 0), allow_fp8=True,
              site=None):
    """dx[M,K] = dy[M,N] @ w[N,K]  (optionally * gelu'(pre) * dropout-mask; pre_is_grad: `dgelu_pre` already holds
    gelu'(pre), saved by the forward's ACT_GELU_SAVEGRAD epilogue)."""
    dx = torch.empty((M, Kd), dtype=out_dtype, device=dy.device)
    act = (ACT_MULAUX if pre_is_grad else ACT_DGELU) if dgelu_pre is not None else ACT_NONE
    if _use_fp8(allow_fp8, dy, w_c, k_dims=(N,)) and (dgelu_pre is None or dgelu_pre.dtype == torch.bfloat16):
        dyq, _, sdy = _q8(dy, E5M2, hist=_fp8_hist(site, "dy"))
        _, wqt, sw = _q8(w_c, E4M3, want_t=True, hist=_fp8_hist(site, "w"))      # (cached from the forward)
        K.gemm(dyq, wqt, dx, M, Kd, N, N, wqt.stride(0), Kd, act=act, aux_in=dgelu_pre, ld_aux_in=Kd,
               dropout_p=drop[0], dropout_seed=drop[1], scale_a=sdy, scale_b=sw)
        return dx
    K.gemm(dy, w_c, dx, M, Kd, N, N, Kd, Kd, b_kmajor=False, act=act,
           aux_in=dgelu_pre, ld_aux_in=Kd, dropout_p=drop[0], dropout_seed=drop[1])
    return dx


# Weight-gradient GEMMs are collected -- over SEVERAL blocks at short token counts -- and issued as one grouped launch
# (favit_gemm_grouped_tn): nothing downstream in the backward chain reads a weight gradient, so the launch can wait,
# and the more tiles it holds, the fewer K-splits it needs to fill the chip (round 4; csrc/gemm.hip grouped_plan: the
# twelve blocks of cfg3 in ONE launch without any split, slab or reduction kernel: 19 us per block against 40).
# How long it waits is bounded by the bytes the waiting operands keep alive (FAVIT_WGRAD_HOLD_MB, default 384: about
# the Infinity Cache + L2): at 50,432 tokens one block already holds 620 MB, so the dense cfg2 / cfg4 step launches per
# block as before -- measured, four cfg2 blocks per launch make the launch itself 2.5 % faster and the STEP 1 % slower
# (14.49 vs 14.35 ms; cfg4 28.99 vs 28.82): the held dY buffers are no longer recycled block after block, every
# input-gradient GEMM writes into memory that is cold in the Infinity Cache and the TLB (those GEMMs: 3.74 -> 3.84 ms).
# At most four blocks per launch when somebody listens for finished gradients (data parallelism: the buckets of those
# blocks go out while the rest of backward runs; the graph segments of train.GraphedStep end a launch as well).
# A pruned (CLS-only) encoder has a different token count in every block.  Until round 8 a grouped launch shared one
# token count and such an encoder launched per block; favit_gemm_grouped_tn_ragged plans K-splits per block, so its
# blocks join one list under the same limits ("ragged").  The blocks grow as backward walks down (5 .. 71 rows at cfg2),
# so the list is launched BEFORE the next block would pass a limit: EncoderOp.bwd tells end_block how many rows the
# next block has.  "ends" are the list lengths at the block boundaries: if the library declines a ragged list, it is
# launched block by block as before (then GEMM by GEMM), never half of it.
_WG_HOLD_BYTES = int(float(os.environ.get("FAVIT_WGRAD_HOLD_MB", "384")) * (1 << 20))
# (ragged lists wait longer by default: the pruned cfg2 encoder holds 1.4 GB in all and its step is fastest with ONE
# launch for the twelve blocks -- DESIGN.md section 11 has the A/B; FAVIT_WGRAD_HOLD_MB sets both limits)
_WG_HOLD_RAGGED_BYTES = int(float(os.environ.get("FAVIT_WGRAD_HOLD_MB", "2048")) * (1 << 20))


# Small latency-bound launches that only produce PARAMETER gradients (nothing downstream in the backward chain reads
# them) are collected per encoder backward and issued batched: the latent_proj fold backward (one ~100-workgroup launch
# per layer: 22.9 us x 12 per cfg2 step) and the fold of the LayerNorm dgamma / dbeta partial sums (one per LayerNorm
# backward: 4.7 us x 24).  Single process: one batch at the end of the encoder backward; under data parallelism whenever
# the grouped weight-gradient launch has gone out (every 4 blocks), so that the buckets holding these gradients start
# their all-reduce while the rest of backward still runs.  The fold consumes dWeff: never before that launch.
#
# Zero-initialised fp32 vectors for fused column sums that have no gradient buffer to accumulate into (the bias
# gradient of the folded qkv weights, one per block): carved out of ONE zero-filled pool per encoder backward instead
# of one 5-us fill launch each (12 per cfg2 step).

# What waits in a _BackwardQueue, as named records:
# a weight-gradient GEMM, dw (+)= dy^T a with db += column sums of dy; ready: the parameters to announce afterwards
_WGrad = namedtuple("_WGrad", "dy a dw db accumulate ready")
# a latent_proj fold backward (K.mhla_fold_bwd_multi); out: the four gradient buffers, None where a half is switched off
_Fold = namedtuple("_Fold", "dweff dbeff wqkv bqkv wl out H ready")
# a fold of LayerNorm partial sums into the dgamma / dbeta buffers (K.reduce_rows_multi)
_LNFold = namedtuple("_LNFold", "part dg db ready")


def _launch_wgrads(probs) -> None:
    if not K.gemm_grouped_tn(probs):           # (one problem too: fine-tuning with frozen layers leaves only dWeff)
        for dy, a, dw, db, acc in probs:
            K.gemm(dy, a, dw, dy.shape[1], a.shape[1], dy.shape[0], dy.stride(0), a.stride(0), dw.stride(0),
                   a_kmajor=False, b_kmajor=False, a_rowsum=db, accumulate=acc)


class _BackwardQueue:
    """What one encoder backward holds back: ``with _BackwardQueue(...) as q`` makes q the current queue (_QUEUE), and
    lin_bwd_w, MHLAChain.qkv_grads and _zero_vec then queue into it / carve from it instead of launching.  Leaving
    the ``with`` launches what still waits (weight gradients, then the deferred folds) and joins the side stream; an
    exception drops everything unlaunched.  Outside a ``with`` _QUEUE is None and everything launches at once.
    per_block: the token count differs from block to block (CLS-only encoders).  The blocks are grouped through the
    ragged launch; in side-stream mode and with FAVIT_WGRAD_PER_BLOCK set every block launches on its own (and in
    side-stream mode nothing is deferred).  zero_floats: size of the zero pool on `device`."""

    def __init__(self, per_block: bool = False, zero_floats: int = 0, device=None):
        self.every = 4 if _STATE["grad_ready"] is not None else K.GROUP_MAX // 4
        self.ragged = per_block
        if _SIDE["enabled"] or os.environ.get("FAVIT_WGRAD_PER_BLOCK"):
            self.every = 1                    # (side-stream mode and the A/B switch: one launch per block, as in round 3)
            self.ragged = False
        self.wgrads: List[_WGrad] = []
        self.blocks, self.bytes, self.ends, self.blk_bytes = 0, 0, [], 0
        self.defer = not _SIDE["enabled"]
        self.folds: List[_Fold] = []
        self.ln_folds: List[_LNFold] = []
        self.zeros = torch.zeros(zero_floats, dtype=torch.float32, device=device) if zero_floats > 0 else None
        self.zero_off = 0

    def __enter__(self):
        global _QUEUE
        _QUEUE = self
        return self

    def __exit__(self, exc_type, exc, tb):
        global _QUEUE
        try:
            if exc_type is None:
                self.flush_wgrads()
                self.flush_deferred()
        finally:
            _QUEUE = None
        if exc_type is None:
            join_side_stream()
        else:
            _SIDE["pending"].clear()          # (the half-collected gradients of the failed backward are dropped)
        return False

    def add_wgrad(self, dy, a, dw, db, accumulate, ready) -> None:
        self.wgrads.append(_WGrad(dy, a, dw, db, accumulate, ready))
        self.bytes += dy.numel() * dy.element_size() + a.numel() * a.element_size()

    def end_block(self, next_rows=None) -> bool:
        """The end of a block: launches the weight gradients only every `every` blocks or once the waiting operands
        exceed the hold limit.  next_rows = (rows of the block that just ended, rows of the next one) where the blocks
        differ (ragged lists).  Returns True if no weight gradient waits afterwards."""
        lst = self.wgrads
        self.blocks += 1
        nb = self.blocks
        if self.ragged:
            n_blk = len(lst) - (self.ends[-1] if self.ends else 0)
            b_blk = self.bytes - self.blk_bytes
            self.ends.append(len(lst))
            self.blk_bytes = self.bytes
            # (would the NEXT block still fit the hold limit and the launch?  its operands scale with its rows)
            scale = next_rows[1] / max(next_rows[0], 1) if next_rows else 1.0
            if nb < self.every and self.bytes + b_blk * scale <= _WG_HOLD_RAGGED_BYTES and len(lst) + n_blk <= K.GROUP_MAX:
                return not lst
        # (would one more block of the same size still fit the hold limit and the launch?)
        elif nb < self.every and self.bytes * (nb + 1) <= _WG_HOLD_BYTES * nb and len(lst) * (nb + 1) <= K.GROUP_MAX * nb:
            return not lst
        self.flush_wgrads()
        return True

    def flush_wgrads(self) -> None:
        """Launch the collected weight-gradient GEMMs (grouped if the library can, else one by one)."""
        lst, ends = self.wgrads, self.ends
        self.wgrads, self.blocks, self.bytes, self.ends, self.blk_bytes = [], 0, 0, [], 0
        if not lst:
            return
        probs = [(e.dy, e.a, e.dw, e.db, e.accumulate) for e in lst]
        with _side_stream(*[t for e in lst for t in (e.dy, e.a, e.dw, e.db)]):
            if not self.ragged:
                _launch_wgrads(probs)
            elif not K.gemm_grouped_tn_ragged(probs):
                # declined as a whole (a token count that is no multiple of 32): block by block, as before round 8
                bounds = [0] + [e for e in ends if 0 < e < len(probs)] + [len(probs)]
                for lo, hi in zip(bounds[:-1], bounds[1:]):
                    if hi > lo:
                        _launch_wgrads(probs[lo:hi])
            for e in lst:
                _ready(*e.ready)

    def flush_deferred(self) -> None:
        if not self.defer:
            return
        assert not self.wgrads, "the latent_proj fold reads weight gradients that have not been launched"
        folds, ln = self.folds, self.ln_folds
        self.folds, self.ln_folds = [], []
        if ln:
            by_cols = {}                      # (one launch per width: the row counts of a pruned encoder's blocks differ,
            for e in ln:                      #  and favit_reduce_rows_multi_ragged takes them together)
                by_cols.setdefault(e.part.shape[-1], []).append(e)
            for es in by_cols.values():
                K.reduce_rows_multi([(e.part, e.dg, e.db) for e in es])
            for e in ln:
                _ready(*e.ready)
        by_h = {}
        for e in folds:
            by_h.setdefault((e.H, tuple(e.wqkv.shape), e.out[0] is None), []).append(e)
        for (H, _, _), es in by_h.items():
            K.mhla_fold_bwd_multi([(e.dweff, e.dbeff, e.wqkv, e.bqkv, e.wl, e.out) for e in es], H)
            for e in es:
                _ready(*e.ready)

    def zero_vec(self, n: int, device) -> torch.Tensor:
        """n zeros carved from the pool; fresh ones where it is exhausted or lives on another device."""
        buf = self.zeros
        n4 = (n + 3) // 4 * 4                 # keep every slice 16-byte aligned (slab reduction)
        if buf is not None and buf.device == device and self.zero_off + n4 <= buf.numel():
            o = self.zero_off
            self.zero_off = o + n4
            return buf[o:o + n]
        return torch.zeros(n, dtype=torch.float32, device=device)


_QUEUE: Optional[_BackwardQueue] = None       # the encoder backward that is running, if any


def _zero_vec(n: int, device) -> torch.Tensor:
    return _QUEUE.zero_vec(n, device) if _QUEUE is not None else torch.zeros(n, dtype=torch.float32, device=device)


def lin_bwd_w(dy, a, M, N, Kd, want_bias=True, wp=None, bp=None, allow_fp8=True):
    """dw[N,K] = dy[M,N]^T @ a[M,K] (fp32, split-K over the tokens), db[N] = column sums of dy (fused).
    If the parameters wp / bp own usable .grad buffers the results are accumulated there and None
    is returned in their place."""
    frozen_w = wp is not None and not wp.requires_grad
    frozen_b = (not want_bias) or (bp is not None and not bp.requires_grad)
    if frozen_w and frozen_b:          # frozen layer (experiments/mhla_pretrained.py:237-247): no weight-gradient GEMM
        return None, None
    tw = _gt(wp)
    tb = _gt(bp) if want_bias else None
    dw = tw if tw is not None else torch.empty((N, Kd), dtype=torch.float32, device=dy.device)
    db = None
    if want_bias:
        db = tb if tb is not None else _zero_vec(N, dy.device)
    if _QUEUE is not None and dy.dtype == torch.bfloat16:
        # deferred: joins the block's grouped weight-gradient launch
        _QUEUE.add_wgrad(dy, a, dw, db, tw is not None, [p for p, t in ((wp, tw), (bp, tb)) if t is not None])
        return (None if tw is not None else dw), (None if tb is not None else db)
    with _side_stream(dy, a, dw, db):
        # a long-token weight gradient outside a block (patch embedding: 50,176 tokens at cfg2): the grouped launch
        # with ONE problem -- K-splits into slabs + fixed-order reduction -- instead of split-K with fp32 atomics
        # (73 -> ~45 us, and bitwise reproducible); it declines what it cannot take (short or ragged token counts)
        if not (dy.dtype == torch.bfloat16 and M >= 8192 and (db is not None or not want_bias) and
                K.gemm_grouped_tn([(dy, a, dw, db, tw is not None)])):
            K.gemm(dy, a, dw, N, Kd, M, N, Kd, Kd, a_kmajor=False, b_kmajor=False, a_rowsum=db,
                   accumulate=tw is not None)
    if tw is not None:
        _ready(wp)
    if tb is not None:
        _ready(bp)
    return (None if tw is not None else dw), (None if tb is not None else db)


# ------------------------------------------------------------------------------------
# scaled-dot-product attention on the MFMA GEMM (dense variants)
# ------------------------------------------------------------------------------------
class _View:
    """[rows, ld] matrix holding per-(batch, head) [L, hd] blocks: element (b,h,l,d) at
    off + b*sb + h*sh + l*ld + d."""
    __slots__ = ("t", "off", "ld", "sb", "sh")

    def __init__(self, t, off, ld, sb, sh):
        self.t, self.off, self.ld, self.sb, self.sh = t, off, ld, sb, sh


def sdpa_fwd(q: _View, k: _View, v: _View, o: _View, B, H, Lq, Lk, hd, scale, mask, m_sb, m_sq, p, seed):
    """softmax(scale * q k^T, masked) (dropout) v on the fused kernel (csrc/sdpa.hip): no [B*H, Lq, Lk] tensor
    in HBM.  Returns what backward needs: (lse,) -- or, for a head dim the fused kernel does not take (not a
    multiple of 16), the unfused MFMA-GEMM + softmax chain's (P, Pd)."""
    if hd % 16 == 0:
        return (K.sdpa_fwd(q, k, v, o, B, H, Lq, Lk, hd, scale, mask, m_sb, m_sq, p, seed),)
    cdt = q.t.dtype
    Z = B * H
    S = torch.empty((Z, Lq, Lk), dtype=torch.float32, device=q.t.device)
    K.gemm(q.t, k.t, S, Lq, Lk, hd, q.ld, k.ld, Lk, alpha=scale, batch=Z, batch_inner=H, sA=(q.sb, q.sh),
           sB=(k.sb, k.sh), sC=(H * Lq * Lk, Lq * Lk), a_off=q.off, b_off=k.off)
    P, Pd = K.softmax_fwd(S, cdt, H, Z, Lq, Lk, mask, m_sb, m_sq, p, seed)
    K.gemm(Pd, v.t, o.t, Lq, hd, Lk, Lk, v.ld, o.ld, b_kmajor=False, batch=Z, batch_inner=H,
           sA=(H * Lq * Lk, Lq * Lk), sB=(v.sb, v.sh), sC=(o.sb, o.sh), b_off=v.off, c_off=o.off)
    return P, Pd


def sdpa_bwd(q: _View, k: _View, v: _View, o: _View, do: _View, dq: _View, dk: _View, dv: _View, saved, B, H, Lq, Lk,
             hd, scale, mask, m_sb, m_sq, p, seed):
    if len(saved) == 1:
        K.sdpa_bwd(q, k, v, o, do, dq, dk, dv, saved[0], B, H, Lq, Lk, hd, scale, mask, m_sb, m_sq, p, seed)
        return
    P, Pd = saved
    Z = B * H
    sP = (H * Lq * Lk, Lq * Lk)
    dPd = torch.empty((Z, Lq, Lk), dtype=torch.float32, device=q.t.device)
    K.gemm(do.t, v.t, dPd, Lq, Lk, hd, do.ld, v.ld, Lk, batch=Z, batch_inner=H, sA=(do.sb, do.sh), sB=(v.sb, v.sh),
           sC=sP, a_off=do.off, b_off=v.off)
    dS = K.softmax_bwd(P, dPd, Z, Lq, Lk, p, seed)
    # dQ = scale * dS . K
    K.gemm(dS, k.t, dq.t, Lq, hd, Lk, Lk, k.ld, dq.ld, b_kmajor=False, alpha=scale, batch=Z, batch_inner=H, sA=sP,
           sB=(k.sb, k.sh), sC=(dq.sb, dq.sh), b_off=k.off, c_off=dq.off)
    # dK = scale * dS^T . Q
    K.gemm(dS, q.t, dk.t, Lk, hd, Lq, Lk, q.ld, dk.ld, a_kmajor=False, b_kmajor=False, alpha=scale, batch=Z,
           batch_inner=H, sA=sP, sB=(q.sb, q.sh), sC=(dk.sb, dk.sh), b_off=q.off, c_off=dk.off)
    # dV = Pd^T . dO
    K.gemm(Pd, do.t, dv.t, Lk, hd, Lq, Lk, do.ld, dv.ld, a_kmajor=False, b_kmajor=False, batch=Z, batch_inner=H,
           sA=sP, sB=(do.sb, do.sh), sC=(dv.sb, dv.sh), b_off=do.off, c_off=dv.off)


# ------------------------------------------------------------------------------------
# attention chains: input = LayerNorm output xn [M, D] (compute dtype), output fp32 [M, D]
# (+ residual fused into the projection epilogue).  bwd takes the compute-dtype copy of the
# output gradient and returns (dxn [M,D] compute dtype, [param grads in `names` order]).
# What a chain's fwd saves for its bwd is a record, read by field name everywhere.  Dropout: p_* is the rate in force
# (0.0 in eval mode), seed_* its seed (0 where the rate is 0).  prm: the chain's parameters in `names` order.
# ------------------------------------------------------------------------------------
# xn: the chain's input [M, D]; weff: the qkv weight with latent_proj folded in; qkv [M, 3D]; o: the attention output
# [M, D]; wp_c: the proj weight in the compute dtype; lse: the row statistics of the saved-statistics backward, or None
MHLASaved = namedtuple("MHLASaved", "xn weff qkv o wp_c mask B L p_attn seed_attn p_proj seed_proj prm lse")
# att: what sdpa_fwd saved
DenseSaved = namedtuple("DenseSaved", "xn wqkv_c qkv o wp_c att mask B L p_attn seed_attn p_proj seed_proj prm")
# qn / kn: the normalised query / key-value inputs; q, k, v: their projections; w_c: the (q, k, v, out) projection
# weights in the compute dtype
CrossSaved = namedtuple("CrossSaved", "qn kn q k v o w_c att mask B Lq Lk p_attn seed_attn scale prm")
# pre: the fc1 pre-activation, or GELU'(pre) where pre_is_grad; h: fc1's output behind GELU and dropout [M, hidden];
# p: the one rate of both dropouts (behind fc1 and behind fc2)
MLPSaved = namedtuple("MLPSaved", "xn pre pre_is_grad h w1_c w2_c p seed_fc1 seed_fc2 prm")


# ------------------------------------------------------------------------------------------------------------------
# Attention maps.  kind: "mhla" (probs [B, L, W], or [B, H, L, W] per head, slot layout of
# window_indices) or "dense" (probs [B, L, L] / [B, H, L, L], W = 0); fp32, in original token coordinates.
AttentionRecord = namedtuple("AttentionRecord", "kind probs W B L H")
_CAPTURE = {"active": None}


class AttentionCapture:
    """What capture_attention yields.  layers: one AttentionRecord per attention chain that ran, in execution order."""

    def __init__(self, per_head: bool):
        self.per_head = bool(per_head)
        self.layers: List[AttentionRecord] = []

    @staticmethod
    def admit(who: str, training: bool) -> None:
        """Raises where a chain's forward cannot be captured: the maps describe the eval forward as stored."""
        if training:
            raise RuntimeError(f"capture_attention: {who}.fwd ran in training mode; attention maps are taken from an "
                               "eval-mode forward (model.eval(), no dropout draws)")
        if _STATE.get("fp8"):
            raise RuntimeError("capture_attention: the fp8 compute mode is active; capture in bf16, fp32 or fp32x3")


@contextlib.contextmanager
def capture_attention(per_head: bool = False):
    """While active, every MHLAChain.fwd / DenseChain.fwd also runs the probability kernel (K.mhla_attn_probs /
    K.sdpa_probs) on the qkv its projection just wrote -- the values the fused attention kernel reads -- and appends an
    AttentionRecord to the yielded object's .layers (head-mean maps, or per-head ones with per_head=True).  The
    unpruned Python chains run: cls_only_cuts returns None and the native block path is not taken, so the maps are in
    original token coordinates (pruned capture, the compact head + tail layout mapped back, is not implemented).
    Raises: ValueError for a nested capture; RuntimeError in fp8 mode, for a forward in training mode and for a
    CrossChain.  With no capture active the chains do one dictionary lookup more and nothing else."""
    if _CAPTURE["active"] is not None:
        raise ValueError("capture_attention: a capture is already active; captures do not nest")
    AttentionCapture.admit("capture_attention", False)
    cap = AttentionCapture(per_head)
    _CAPTURE["active"] = cap
    try:
        yield cap
    finally:
        _CAPTURE["active"] = None


def window_indices(L: int, W: int) -> torch.Tensor:
    """int64 [L, W] on the CPU: the key in slot w of row i of an MHLA window (the closed form of the reference's
    MultiHeadLatentAttention._get_window_indices, win_idx in csrc/common.h).  A window cut at 0 repeats key L - 1 in
    its last slots, a window cut at L only repeats key 0 in its first slots."""
    if W < 1 or W % 2 == 0 or L < 1:
        raise ValueError(f"window_indices: L >= 1 and an odd W >= 1, got L = {L}, W = {W}")
    h = W // 2
    i = torch.arange(L, dtype=torch.int64).unsqueeze(1)
    w = torch.arange(W, dtype=torch.int64).unsqueeze(0)
    lo = (i - h).clamp(min=0)
    n = (i + h + 1).clamp(max=L) - lo
    pad = W - n
    at_start = torch.where(w < n, w.expand(L, W), torch.full((L, W), L - 1, dtype=torch.int64))
    at_end = torch.where(w < pad, torch.zeros((L, W), dtype=torch.int64), lo + w - pad)
    return torch.where(n == W, lo + w, torch.where(lo == 0, at_start, at_end))


class MHLAChain:
    q8_fwd, q8_bwd = 0, 4        # prm index of the weight whose GEMM consumes the chain's input (qkv) / output gradient (proj)
    """MultiHeadLatentAttention.forward (models/mhla.py:85-161)."""
    names = ("qkv.weight", "qkv.bias", "latent_proj.weight", "latent_proj.bias", "proj.weight", "proj.bias")

    def __init__(self, H, W, p_attn=0.0, p_proj=0.0):
        if W % 2 == 0:
            raise ValueError("window_size must be odd: the reference crashes on even sizes (models/mhla.py:83)")
        self.H, self.W, self.p_attn, self.p_proj = H, W, p_attn, p_proj

    def fwd(self, xn, prm, B, L, residual, mask, training, pre=None):
        """mask: [B, L, L] (0 = masked) or None.  pre: (weff, beff) where the caller has folded latent_proj already."""
        _check_mask_shape("MHLAChain", mask, "[B, L, L]", (B, L, L))
        cap = _CAPTURE["active"]
        if cap is not None:
            cap.admit("MHLAChain", training)
        wqkv, bqkv, wl, bl, wp, bp = prm
        M, D = xn.shape
        H, hd = self.H, D // self.H
        pa = self.p_attn if training else 0.0
        pp = self.p_proj if training else 0.0
        sa = _seed() if pa > 0 else 0
        sp = _seed() if pp > 0 else 0
        weff, beff = pre if pre is not None else K.mhla_fold_fwd(wqkv, bqkv, wl, bl, H, xn.dtype)
        qkv = lin_fwd(xn, weff, beff, M, 3 * D, D, xn.dtype, site=wqkv)
        if cap is not None:
            cap.layers.append(AttentionRecord("mhla", K.mhla_attn_probs(qkv, B, L, H, hd, self.W, mask,
                                                                        head_mean=not cap.per_head), self.W, B, L, H))
        # training: the forward also leaves lse per row, and backward runs the saved-statistics kernel (None where
        # that kernel does not apply: other head sizes, fp32)
        o, lse = K.mhla_attn_fwd(qkv, B, L, H, hd, self.W, mask, pa, sa, want_lse=True) if training else \
            (K.mhla_attn_fwd(qkv, B, L, H, hd, self.W, mask, pa, sa), None)
        wp_c = wcast(wp)
        y = lin_fwd(o, wp_c, bp.detach(), M, D, D, torch.float32, residual=residual, drop=(pp, sp), site=wp)
        return y, MHLASaved(xn=xn, weff=weff, qkv=qkv, o=o, wp_c=wp_c, mask=mask, B=B, L=L, p_attn=pa, seed_attn=sa,
                            p_proj=pp, seed_proj=sp, prm=prm, lse=lse)

    @staticmethod
    def out_dropout(saved):
        """(p, seed) of the dropout on this branch's output (the mask its incoming gradient must carry)."""
        return saved.p_proj, saved.seed_proj

    def bwd(self, saved, dy_lp, premasked=False):
        s = saved
        xn, prm = s.xn, s.prm
        wqkv, _, _, _, wp, _ = prm
        M, D = xn.shape
        H, hd = self.H, D // self.H
        dym = K.dropout(dy_lp, s.p_proj, s.seed_proj) if (s.p_proj > 0 and not premasked) else dy_lp
        do = lin_bwd_x(dym, s.wp_c, M, D, D, xn.dtype, site=wp)
        dwp, dbp = self.proj_grads(dym, s.o, prm)
        dqkv = K.mhla_attn_bwd(s.qkv, do, s.B, s.L, H, hd, self.W, s.mask, s.p_attn, s.seed_attn,
                               o=s.o if s.lse is not None else None, lse=s.lse)
        dxn = lin_bwd_x(dqkv, s.weff, M, 3 * D, D, xn.dtype, site=wqkv)
        return dxn, self.qkv_grads(dqkv, xn, prm) + [dwp, dbp]

    @staticmethod
    def proj_grads(dym, o, prm):
        M, D = o.shape
        return lin_bwd_w(dym, o, M, D, D, wp=prm[4], bp=prm[5])

    def qkv_grads(self, dqkv, xn, prm):
        """[dwqkv, dbqkv, dwl, dbl] (None where a gradient buffer took the result) from the gradient of the folded
        projection's output: the dWeff GEMM and the latent_proj fold backward, launched or queued.  Shared by bwd and
        the native block backward (EncoderOp), which differ only in who launched the input-gradient chain."""
        wqkv, bqkv, wl, bl = prm[:4]
        M, D = xn.shape
        H = self.H
        dweff, dbeff = lin_bwd_w(dqkv, xn, M, 3 * D, D)
        # (dW2, dW1, dWproj, dWeff join the grouped weight-gradient launch, which may wait for further blocks; the
        # batched fold below consumes dWeff only after that launch -- EncoderOp.bwd flushes in that order)
        tg = [_gt(p) for p in (wqkv, bqkv, wl, bl)]
        q = _QUEUE
        defer = q is not None and q.defer
        if all(t is not None for t in tg) and defer:
            q.folds.append(_Fold(dweff, dbeff, wqkv.detach(), bqkv.detach(), wl.detach(), tg, H, (wqkv, bqkv, wl, bl)))
            return [None, None, None, None]
        if (defer and not wqkv.requires_grad and not bqkv.requires_grad and tg[2] is not None and tg[3] is not None):
            # frozen qkv projection, trainable latent_proj (experiments/sppp_mhla_pretrained.py:236-247): the batched
            # launch with its qkv half switched off, straight into the latent_proj gradient buffers
            q.folds.append(_Fold(dweff, dbeff, wqkv.detach(), bqkv.detach(), wl.detach(), [None, None, tg[2], tg[3]], H,
                                 (wl, bl)))
            return [None, None, None, None]
        if q is not None:
            q.flush_wgrads()                # the fold runs now: dWeff must have been launched
        if all(t is not None for t in tg):
            with _side_stream(dweff, dbeff):
                K.mhla_fold_bwd(dweff, dbeff, wqkv, bqkv, wl, H, out=tg)
                _ready(wqkv, bqkv, wl, bl)
            return [None, None, None, None]
        join_side_stream()
        return list(K.mhla_fold_bwd(dweff, dbeff, wqkv, bqkv, wl, H))


class DenseChain:
    q8_fwd, q8_bwd = 0, 2
    """vit.MultiHeadAttention.forward (models/vit.py:77-104) and, with the
    nn.MultiheadAttention parameter names, the use_mhla=False branch
    (models/vit_mhla.py:57-62,96-101).  mask: key-keep [B,L] (torch MHA) or None."""

    def __init__(self, H, p_attn=0.0, p_proj=0.0, torch_mha=False):
        self.H, self.p_attn, self.p_proj, self.torch_mha = H, p_attn, p_proj, torch_mha
        self.names = (("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias") if torch_mha
                      else ("qkv.weight", "qkv.bias", "proj.weight", "proj.bias"))

    def _views(self, t, B, L, D, hd):
        ld = 3 * D
        return (_View(t, 0, ld, L * ld, hd), _View(t, D, ld, L * ld, hd), _View(t, 2 * D, ld, L * ld, hd))

    def fwd(self, xn, prm, B, L, residual, mask, training):
        _check_mask_shape("DenseChain", mask, "key-keep [B, L]", (B, L))
        cap = _CAPTURE["active"]
        if cap is not None:
            cap.admit("DenseChain", training)
        wqkv, bqkv, wp, bp = prm
        M, D = xn.shape
        H, hd = self.H, D // self.H
        pa = self.p_attn if training else 0.0
        pp = self.p_proj if (training and not self.torch_mha) else 0.0   # nn.MultiheadAttention has no proj dropout
        sa = _seed() if pa > 0 else 0
        sp = _seed() if pp > 0 else 0
        wqkv_c, wp_c = wcast(wqkv), wcast(wp)
        qkv = lin_fwd(xn, wqkv_c, bqkv.detach(), M, 3 * D, D, xn.dtype, site=wqkv)
        if cap is not None:
            cap.layers.append(AttentionRecord("dense", K.sdpa_probs(qkv, B, L, H, hd, mask, hd ** -0.5,
                                                                    head_mean=not cap.per_head), 0, B, L, H))
        o = torch.empty((M, D), dtype=xn.dtype, device=xn.device)
        q, k, v = self._views(qkv, B, L, D, hd)
        ov = _View(o, 0, D, L * D, hd)
        att = sdpa_fwd(q, k, v, ov, B, H, L, L, hd, hd ** -0.5, mask, L if mask is not None else 0, 0, pa, sa)
        y = lin_fwd(o, wp_c, bp.detach(), M, D, D, torch.float32, residual=residual, drop=(pp, sp), site=wp)
        return y, DenseSaved(xn=xn, wqkv_c=wqkv_c, qkv=qkv, o=o, wp_c=wp_c, att=att, mask=mask, B=B, L=L, p_attn=pa,
                             seed_attn=sa, p_proj=pp, seed_proj=sp, prm=prm)

    @staticmethod
    def out_dropout(saved):
        return saved.p_proj, saved.seed_proj

    def bwd(self, saved, dy_lp, premasked=False):
        s = saved
        xn, qkv, o, mask, B, L = s.xn, s.qkv, s.o, s.mask, s.B, s.L
        wqkv, bqkv, wp, bp = s.prm
        M, D = xn.shape
        H, hd = self.H, D // self.H
        dym = K.dropout(dy_lp, s.p_proj, s.seed_proj) if (s.p_proj > 0 and not premasked) else dy_lp
        do = lin_bwd_x(dym, s.wp_c, M, D, D, xn.dtype, site=wp)
        dwp, dbp = lin_bwd_w(dym, o, M, D, D, wp=wp, bp=bp)
        dqkv = torch.empty_like(qkv)
        q, k, v = self._views(qkv, B, L, D, hd)
        dq, dk, dv = self._views(dqkv, B, L, D, hd)
        sdpa_bwd(q, k, v, _View(o, 0, D, L * D, hd), _View(do, 0, D, L * D, hd), dq, dk, dv, s.att, B, H, L, L, hd,
                 hd ** -0.5, mask, L if mask is not None else 0, 0, s.p_attn, s.seed_attn)
        dxn = lin_bwd_x(dqkv, s.wqkv_c, M, 3 * D, D, xn.dtype, site=wqkv)
        dwqkv, dbqkv = lin_bwd_w(dqkv, xn, M, 3 * D, D, wp=wqkv, bp=bqkv)
        return dxn, [dwqkv, dbqkv, dwp, dbp]


class CrossChain:
    """CrossAttention.forward (models/attention.py:37-78; ONE head, scores / embed_dim**0.5,
    no dropout after out_proj) and MultiHeadCrossAttention.forward (attention.py:105-148)."""
    names = ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "v_proj.weight", "v_proj.bias",
             "out_proj.weight", "out_proj.bias")

    def __init__(self, H, p_attn=0.0):
        self.H, self.p_attn = H, p_attn

    def fwd(self, qn, kn, prm, B, Lq, Lk, residual, mask, training):
        _check_mask_shape("CrossChain", mask, "[B, Lq, Lk]", (B, Lq, Lk))
        if _CAPTURE["active"] is not None:
            raise RuntimeError("capture_attention: a CrossChain ran under the capture; cross-attention maps (Lq x Lk, "
                               "two sequences) are not implemented")
        wq, bq, wk, bk, wv, bv, wo, bo = prm
        D = qn.shape[1]
        H, hd = self.H, D // self.H
        pa = self.p_attn if training else 0.0
        sa = _seed() if pa > 0 else 0
        cdt = qn.dtype
        wq_c, wk_c, wv_c, wo_c = wcast(wq), wcast(wk), wcast(wv), wcast(wo)
        q = lin_fwd(qn, wq_c, bq.detach(), B * Lq, D, D, cdt)
        k = lin_fwd(kn, wk_c, bk.detach(), B * Lk, D, D, cdt)
        v = lin_fwd(kn, wv_c, bv.detach(), B * Lk, D, D, cdt)
        o = torch.empty((B * Lq, D), dtype=cdt, device=qn.device)
        scale = 1.0 / (hd ** 0.5)
        att = sdpa_fwd(_View(q, 0, D, Lq * D, hd), _View(k, 0, D, Lk * D, hd), _View(v, 0, D, Lk * D, hd),
                       _View(o, 0, D, Lq * D, hd), B, H, Lq, Lk, hd, scale, mask,
                       Lq * Lk if mask is not None else 0, Lk if mask is not None else 0, pa, sa)
        y = lin_fwd(o, wo_c, bo.detach(), B * Lq, D, D, torch.float32, residual=residual)
        return y, CrossSaved(qn=qn, kn=kn, q=q, k=k, v=v, o=o, w_c=(wq_c, wk_c, wv_c, wo_c), att=att, mask=mask, B=B,
                             Lq=Lq, Lk=Lk, p_attn=pa, seed_attn=sa, scale=scale, prm=prm)

    def bwd(self, saved, dy_lp):
        s = saved
        qn, kn, q, k, v, o, att, mask, B, Lq, Lk = s.qn, s.kn, s.q, s.k, s.v, s.o, s.att, s.mask, s.B, s.Lq, s.Lk
        (wq_c, wk_c, wv_c, wo_c), pa, sa, scale = s.w_c, s.p_attn, s.seed_attn, s.scale
        wq, bq, wk, bk, wv, bv, wo, bo = s.prm
        D = qn.shape[1]
        H, hd = self.H, D // self.H
        cdt = qn.dtype
        Mq, Mk = B * Lq, B * Lk
        do = lin_bwd_x(dy_lp, wo_c, Mq, D, D, cdt)
        dwo, dbo = lin_bwd_w(dy_lp, o, Mq, D, D, wp=wo, bp=bo)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        sdpa_bwd(_View(q, 0, D, Lq * D, hd), _View(k, 0, D, Lk * D, hd), _View(v, 0, D, Lk * D, hd),
                 _View(o, 0, D, Lq * D, hd), _View(do, 0, D, Lq * D, hd), _View(dq, 0, D, Lq * D, hd),
                 _View(dk, 0, D, Lk * D, hd), _View(dv, 0, D, Lk * D, hd), att, B, H, Lq, Lk, hd, scale, mask,
                 Lq * Lk if mask is not None else 0, Lk if mask is not None else 0, pa, sa)
        dqn = lin_bwd_x(dq, wq_c, Mq, D, D, cdt)
        dwq, dbq = lin_bwd_w(dq, qn, Mq, D, D, wp=wq, bp=bq)
        dkn = torch.empty((Mk, D), dtype=torch.float32, device=qn.device)
        K.gemm(dk, wk_c, dkn, Mk, D, D, D, D, D, b_kmajor=False)
        K.gemm(dv, wv_c, dkn, Mk, D, D, D, D, D, b_kmajor=False, accumulate=True)
        # (the key bias adds q.bk to every score of a query row, which softmax removes: every row of dS sums to 0 under
        # any mask and dropout, so dbk is exactly 0.  The column sum of the stored dk would leave its rounding there --
        # ~1e-3 in bf16 -- which an optimizer that normalises gradients turns into a random walk of the bias.)
        dwk, _ = lin_bwd_w(dk, kn, Mk, D, D, want_bias=False, wp=wk)
        dbk = None
        if bk.requires_grad:
            if _gt(bk) is not None:
                _ready(bk)                   # nothing to add to the gradient buffer
            else:
                dbk = _zero_vec(D, dk.device)
        dwv, dbv = lin_bwd_w(dv, kn, Mk, D, D, wp=wv, bp=bv)
        return dqn, dkn, [dwq, dbq, dwk, dbk, dwv, dbv, dwo, dbo]


class MLPChain:
    q8_fwd, q8_bwd = 0, 2
    """MLP.forward fc1 -> GELU -> drop -> fc2 -> drop (models/vit.py:124-139)."""

    def __init__(self, p=0.0, fc1="fc1", fc2="fc2"):
        self.p = p
        self.names = (f"{fc1}.weight", f"{fc1}.bias", f"{fc2}.weight", f"{fc2}.bias")

    def fwd(self, xn, prm, residual, training):
        w1, b1, w2, b2 = prm
        M, D = xn.shape
        Hd = w1.shape[0]
        Do = w2.shape[0]
        p = self.p if training else 0.0
        s1 = _seed() if p > 0 else 0
        s2 = _seed() if p > 0 else 0
        w1_c, w2_c = wcast(w1), wcast(w2)
        # Low-precision path: the fc1 epilogue saves GELU'(u) (Phi and phi share one exponential) instead of u, so the
        # backward epilogue is a multiply: the GELU arithmetic (~20 VALU slots per element) runs once instead of twice
        # (measured: -0.09 ms per cfg2 step; both epilogues stay bound by their 310 MB of HBM traffic).  The fp32 parity mode keeps the pre-activation and the exact erf.
        sg = self.saves_gelu_grad(xn.dtype)
        h, pre = lin_fwd(xn, w1_c, b1.detach(), M, Hd, D, xn.dtype, act=ACT_GELU_SAVEGRAD if sg else ACT_GELU,
                         want_pre=True, drop=(p, s1), site=w1)
        y = lin_fwd(h, w2_c, b2.detach(), M, Do, Hd, torch.float32, residual=residual, drop=(p, s2), site=w2)
        return y, MLPSaved(xn=xn, pre=pre, pre_is_grad=sg, h=h, w1_c=w1_c, w2_c=w2_c, p=p, seed_fc1=s1, seed_fc2=s2, prm=prm)

    @staticmethod
    def saves_gelu_grad(cdt) -> bool:
        """Does fc1 run ACT_GELU_SAVEGRAD in this compute dtype (then backward multiplies by the saved GELU', ACT_MULAUX)?
        The native block chain (csrc/block.hip) is the bf16 case of this rule."""
        return cdt != torch.float32

    @staticmethod
    def out_dropout(saved):
        return saved.p, saved.seed_fc2

    def bwd(self, saved, dy_lp, premasked=False):
        s = saved
        xn, prm, p = s.xn, s.prm, s.p
        w1, _, w2, _ = prm
        M, D = xn.shape
        Hd, Do = s.w1_c.shape[0], s.w2_c.shape[0]
        dym = K.dropout(dy_lp, p, s.seed_fc2) if (p > 0 and not premasked) else dy_lp
        dpre = lin_bwd_x(dym, s.w2_c, M, Do, Hd, xn.dtype, dgelu_pre=s.pre, pre_is_grad=s.pre_is_grad, drop=(p, s.seed_fc1),
                         site=w2)
        dw2, db2 = self.fc2_grads(dym, s.h, prm)
        dxn = lin_bwd_x(dpre, s.w1_c, M, Hd, D, xn.dtype, site=w1)
        dw1, db1 = self.fc1_grads(dpre, xn, prm)
        return dxn, [dw1, db1, dw2, db2]

    # the two weight-gradient problems, as bwd and the native block backward (EncoderOp) both queue them
    @staticmethod
    def fc2_grads(dym, h, prm):
        return lin_bwd_w(dym, h, dym.shape[0], dym.shape[1], h.shape[1], wp=prm[2], bp=prm[3])

    @staticmethod
    def fc1_grads(dpre, xn, prm):
        return lin_bwd_w(dpre, xn, dpre.shape[0], dpre.shape[1], xn.shape[1], wp=prm[0], bp=prm[1])


# ------------------------------------------------------------------------------------
# Ops (autograd granularity)
# ------------------------------------------------------------------------------------
class OpFn(torch.autograd.Function):
    """forward(op, n_in, *inputs, *params); the Op owns the kernel sequences."""

    @staticmethod
    def forward(ctx, op, n_in, *tensors):
        K.require_gpu(*[t for t in tensors if t is not None])
        ins, prm = tensors[:n_in], tensors[n_in:]
        out, saved = op.fwd(ins, prm)
        ctx.op, ctx.saved, ctx.n_in, ctx.n_prm = op, saved, n_in, len(prm)
        return out

    @staticmethod
    def backward(ctx, dout):
        din, dprm = ctx.op.bwd(ctx.saved, _as_f32(dout), ctx.needs_input_grad[2:2 + ctx.n_in])
        join_side_stream()
        ctx.saved = None
        return (None, None, *din, *dprm)


def run(op, inputs: Sequence[torch.Tensor], params: Sequence[torch.Tensor]) -> torch.Tensor:
    return OpFn.apply(op, len(inputs), *inputs, *params)


class LinearOp:
    """nn.Linear on fp32 activations (head, standalone projections)."""

    def __init__(self, act=ACT_NONE):
        self.act = act

    def fwd(self, ins, prm):
        (x,), (w, b) = ins, prm
        shp = x.shape
        N = w.shape[0]
        if (self.act == ACT_NONE and N <= K.SMALL_LINEAR_MAX_N and x.dtype == torch.float32 and w.dtype == torch.float32
                and (b is None or b.dtype == torch.float32)):
            # a few classes on a batch of CLS rows: exact-fp32 dot products in one launch instead of one 128x128 GEMM tile
            # behind two casts (favit_small_linear_*: 13-21 us per GEMM launch -> 3-4 us), in every compute mode
            x2 = x.reshape(-1, shp[-1])
            if x2.stride(-1) != 1:
                x2 = x2.contiguous()
            y = K.small_linear_fwd(x2, w.detach(), None if b is None else b.detach())
            return y.reshape(*shp[:-1], N), ("small", x2, shp, b is not None, (w, b))
        a = _as_cdt(x.reshape(-1, shp[-1]))
        w_c = wcast(w)
        M, Kd, N = a.shape[0], a.shape[1], w.shape[0]
        y = lin_fwd(a, w_c, None if b is None else b.detach(), M, N, Kd, torch.float32, allow_fp8=False)
        return y.reshape(*shp[:-1], N), (a, w_c, shp, b is not None, (w, b))

    def bwd(self, saved, dy, needs):
        if isinstance(saved[0], str):
            _, x2, shp, has_b, (w, b) = saved
            M, N = x2.shape[0], w.shape[0]
            dy2 = _as_f32(dy.reshape(M, N))
            if not dy2.is_contiguous():
                dy2 = dy2.contiguous()
            tw, tb = _gt(w), (_gt(b) if has_b else None)
            direct = tw is not None and (tb is not None or not has_b)
            dx, dw, db = K.small_linear_bwd(dy2, x2, w.detach(), want_dx=bool(needs[0]), want_db=has_b,
                                            dw_out=tw if direct else None, db_out=tb if direct else None)
            if direct:
                _ready(w, *( [b] if has_b else [] ))
            dx = dx.reshape(shp) if dx is not None else None
            return [dx], [dw, db] if has_b else [dw]
        a, w_c, shp, has_b, (w, b) = saved
        M, Kd, N = a.shape[0], a.shape[1], w_c.shape[0]
        dy_c = _as_cdt(dy.reshape(M, N))
        dx = lin_bwd_x(dy_c, w_c, M, N, Kd, torch.float32, allow_fp8=False).reshape(shp) if needs[0] else None
        dw, db = lin_bwd_w(dy_c, a, M, N, Kd, want_bias=has_b, wp=w, bp=b, allow_fp8=False)
        return [dx], [dw, db] if has_b else [dw]


class PatchEmbedOp:
    """PatchEmbedding.forward (models/vit.py:43-53): rearrange + Linear(P*P*C -> D)."""

    def __init__(self, P):
        self.P = P

    def fwd(self, ins, prm):
        (img,), (w, b) = ins, prm
        B, Cc, HW, _ = img.shape
        patches = K.patchify_fwd(_as_f32(img), self.P, get_compute_dtype())
        M, Kd = patches.shape
        D = w.shape[0]
        w_c = wcast(w)
        tok = lin_fwd(patches, w_c, b.detach(), M, D, Kd, torch.float32, allow_fp8=False)
        return tok.reshape(B, M // B, D), (patches, w_c, (B, Cc, HW), (w, b))

    def bwd(self, saved, dy, needs):
        patches, w_c, (B, Cc, HW), (w, b) = saved
        M, Kd = patches.shape
        D = w_c.shape[0]
        dy_c = _as_cdt(dy.reshape(M, D))
        dw, db = lin_bwd_w(dy_c, patches, M, D, Kd, wp=w if w.is_leaf else None, bp=b, allow_fp8=False)
        dimg = None
        if needs[0]:
            dpatch = lin_bwd_x(dy_c, w_c, M, D, Kd, torch.float32, allow_fp8=False)
            dimg = K.patchify_bwd(dpatch, B, Cc, HW, self.P)
        return [dimg], [dw, db]


pos_resample_matrix = K.pos_resample_matrix


def _grid_side(n: int) -> Optional[int]:
    """g with g * g == n, or None."""
    g = math.isqrt(n) if n >= 1 else 0
    return g if g >= 1 and g * g == n else None


class _PosResampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, g_in, g_out, antialias, n_prefix):
        K.require_gpu(pos)
        ctx.cfg = (g_in, g_out, antialias, n_prefix, pos.shape)
        x = _as_f32(pos.detach()).reshape(-1, pos.shape[-1]).contiguous()
        y = K.pos_resample(x, g_in, g_out, antialias, n_prefix)
        return y.reshape(*pos.shape[:-2], y.shape[0], y.shape[1])

    @staticmethod
    def backward(ctx, dy):
        g_in, g_out, antialias, n_prefix, shape = ctx.cfg
        d = _as_f32(dy).reshape(-1, shape[-1]).contiguous()
        return K.pos_resample(d, g_in, g_out, antialias, n_prefix, adjoint=True).reshape(shape), None, None, None, None


def pos_resample(pos: torch.Tensor, g_out: int, antialias: bool = True, n_prefix: int = 1) -> torch.Tensor:
    """A learned position embedding on a square grid, resampled to a g_out x g_out grid on the device (bicubic,
    align_corners=False; antialias as in pos_resample_matrix, True being timm's default).  pos: fp32
    [n_prefix + g_in^2, D] or [1, n_prefix + g_in^2, D] on the GPU; the n_prefix (0 or 1) leading rows -- the CLS row
    -- are copied.  Forward and backward are one favit_pos_resample launch each (the backward with the transposed
    table: the exact adjoint, no atomics, bitwise reproducible); the gradient has pos's shape.  D % 4 == 0."""
    if pos.dim() not in (2, 3) or (pos.dim() == 3 and pos.shape[0] != 1):
        raise ValueError(f"pos_resample: pos must be [n, D] or [1, n, D], got {tuple(pos.shape)}")
    g_in = _grid_side(pos.shape[-2] - n_prefix)
    if g_in is None:
        raise ValueError(f"pos_resample: {pos.shape[-2] - n_prefix} grid rows (of {pos.shape[-2]} with {n_prefix} prefix "
                         "rows) are not a square grid")
    return _PosResampleFn.apply(pos, g_in, int(g_out), bool(antialias), int(n_prefix))


class PrologueOp:
    """cat(cls, tokens) (+ pos_embed) (models/vit.py:292-296, models/sppp_mhla.py:303-304).  A pos_embed whose grid is
    not the tokens' (an input of another resolution than the parameter was made for) is resampled to the tokens' grid in
    front of the kernel and its gradient goes back through the adjoint, so the parameter keeps its shape
    (K.pos_resample, antialias as given).  With equal grids nothing of that runs."""

    def __init__(self, has_pos, antialias=True):
        self.has_pos, self.antialias = has_pos, bool(antialias)

    def fwd(self, ins, prm):
        (tok,) = ins
        cls = prm[0]
        pos = prm[1] if self.has_pos else None
        B, N, D = tok.shape
        grids = None
        if pos is not None:
            pos = pos.detach().contiguous()
            if pos.shape[1] != N + 1:
                grids = (_grid_side(pos.shape[1] - 1), _grid_side(N))
                if None in grids:
                    raise ValueError(f"the input gives {N} patch tokens and pos_embed holds {pos.shape[1] - 1} grid rows: "
                                     "resampling needs both to be perfect squares (a square image, a square pos_embed)")
                pos = K.pos_resample(_as_f32(pos).reshape(-1, D), grids[0], grids[1], self.antialias)
        x = K.embed_prologue_fwd(_as_f32(tok), cls.detach().contiguous(), pos, B, N, D)
        return x, (B, N, D, grids)

    def bwd(self, saved, dy, needs):
        B, N, D, grids = saved
        dtok, dcls, dpos = K.embed_prologue_bwd(dy, B, N, D, torch.float32, want_pos=self.has_pos)
        out = [dcls.reshape(1, 1, D)]
        if self.has_pos:
            if grids is not None:
                dpos = K.pos_resample(dpos, grids[0], grids[1], self.antialias, adjoint=True)
            out.append(dpos.reshape(1, -1, D))
        return [dtok.reshape(B, N, D)], out


class BlockSpec:
    """Static description of one pre-LN transformer block (models/vit.py:165-179,
    models/vit_mhla.py:77-109, models/mhla.py:205-222).  drop_path: stochastic depth rate of both residual branches
    (as timm's two DropPath modules of a block; not in the reference), active in training mode only -- see EncoderOp."""

    def __init__(self, attn, mlp, drop_path=0.0):
        if not 0.0 <= float(drop_path) < 1.0:
            raise ValueError("drop_path must lie in [0, 1)")
        self.attn, self.mlp, self.drop_path = attn, mlp, float(drop_path)
        self.names = (("norm1.weight", "norm1.bias") + tuple("attn." + n for n in attn.names) +
                      ("norm2.weight", "norm2.bias") + tuple("mlp." + n for n in mlp.names))
        self.n = len(self.names)

    def split(self, p):
        """(g1, b1, pa, g2, b2, pm) of the block's parameters p, which come in the order of `names`."""
        na = len(self.attn.names)
        return p[0], p[1], p[2:2 + na], p[2 + na], p[3 + na], p[4 + na:]


def cls_plan(L: int, W: int, depth: int) -> List[Optional[Tuple[int, int]]]:
    """Token rows each block of an all-MHLA encoder has to compute when only row 0 (CLS) of the last block is read
    (FinalNormOp).  Row i of a window-W block reads keys [i - h, i + h] (h = W // 2) plus pad copies of key L - 1 (rows
    whose window is cut at 0) or key 0 (rows whose window is cut at L), so the field grows by h rows at each end per
    block going down: block k (1-based) of `depth`, j = depth - k, needs its input rows [0, 1 + h (j + 1)) and
    [L - (1 + h j), L).  Entry k - 1 is that (head, tail) pair, or None where the two ranges cover the sequence.
    Stored head rows first, tail rows after them, a block computes the needed rows correctly with the unchanged window
    rule at L' = head + tail (tests/test_cls_only_plan.py checks both against the oracle)."""
    h = W // 2
    plan: List[Optional[Tuple[int, int]]] = []
    for k in range(1, depth + 1):
        j = depth - k
        a, b = 1 + h * (j + 1), 1 + h * j
        plan.append(None if a + b >= L else (a, b))
    return plan


def cls_only_cuts(specs: Sequence["BlockSpec"], L: int, mask, training: bool):
    """The cls_plan of an encoder whose only consumer is the CLS row, or None where the full path has to run: a block
    that is not MHLA + MLP, differing windows, an attention mask, a dropout that is active in this mode (the masks are
    indexed by element position: a compact layout would draw other masks), fp8 mode (its quantisation sites hand
    tensors of the full shape from kernel to kernel), FAVIT_NO_PRUNE=1 (A/B switch, read at each call), or a sequence
    so short that every block needs all rows, or an active capture_attention (its maps are in original token
    coordinates)."""
    if os.environ.get("FAVIT_NO_PRUNE") or mask is not None or not specs or _STATE.get("fp8"):
        return None
    if _CAPTURE["active"] is not None:
        return None
    if not all(isinstance(s.attn, MHLAChain) and isinstance(s.mlp, MLPChain) for s in specs):
        return None
    if len({s.attn.W for s in specs}) != 1:
        return None
    if training and any(s.attn.p_attn > 0 or s.attn.p_proj > 0 or s.mlp.p > 0 for s in specs):
        return None
    plan = cls_plan(L, specs[0].attn.W, len(specs))
    return plan if any(c is not None for c in plan) else None


def mlp_narrow_plan(cuts: Sequence[Optional[Tuple[int, int]]], after: Optional[Tuple[int, int]] = None):
    """Rows of every block's MLP half.  Only attention mixes rows: proj, LayerNorm 2, fc1, fc2
    and the residual adds are row-wise, and the block after block k reads just its own (head, tail) rows of block k's
    output, so the cut between the two blocks can sit between block k's attention half and its MLP half.
    cuts: the cls_plan entries of the blocks of ONE encoder node; after: the rows the stream must have behind the node
    (the first block of the next graph segment), None where nobody said -- the node's last block then keeps its rows
    (the last block of the encoder always does: the caller reads its rows).  Entry k is the (head, tail) pair block
    k's MLP half runs on, or None for "the rows of its attention half".  A block on all rows (cuts[k] is None) that is
    followed by a narrower one narrows too."""
    cuts = list(cuts)
    out: List[Optional[Tuple[int, int]]] = []
    for k, c in enumerate(cuts):
        nxt = cuts[k + 1] if k + 1 < len(cuts) else after
        out.append(tuple(nxt) if nxt is not None and (c is None or sum(nxt) < sum(c)) else None)
    return out


def mlp_narrow_on() -> bool:
    """A/B switch of the narrowed MLP halves (default on): FAVIT_NO_MLP_NARROW=1, read at each call like
    FAVIT_NO_NATIVE_BLOCKS, restores a cut in front of every block.  K.GEMM_TRACE holds every block on one row count as
    well: its readers (tests/test_gpu_native_blocks.py) look every GEMM of a block up under the block's own rows."""
    return not os.environ.get("FAVIT_NO_MLP_NARROW") and K.GEMM_TRACE is None


# Native block chains: where a block is MHLA + MLP in bf16 without mask or dropout, the seven
# launches of its forward and the seven of its input-gradient chain are issued by ONE library call each
# (favit_mhla_block_fwd / _bwd) instead of one Python wrapper call each, with its allocations and its descriptor.  The
# launches and their arguments are the same, so results are bit-identical; the switches below select the path.
_NATIVE = {"on": True}


def set_native_blocks(on: bool) -> None:
    """A/B switch of the native block chains (default on).  FAVIT_NO_NATIVE_BLOCKS=1 in the environment (read at each
    call, so it shows among a benchmark's knobs) switches them off as well."""
    _NATIVE["on"] = bool(on)


def _native_blocks_on() -> bool:
    """The conditions that do not depend on the block.  K.GEMM_TRACE has to see every GEMM; the side stream is a
    launch pattern of the Python chains only; capture_attention hooks the Python chains' qkv."""
    return (_NATIVE["on"] and K.GEMM_TRACE is None and not _SIDE["enabled"] and _CAPTURE["active"] is None
            and get_compute_mode() == "bf16" and not os.environ.get("FAVIT_NO_NATIVE_BLOCKS"))


def _carve(flat, off, shape):
    """A contiguous view of `shape` at element offset `off` of the flat tensor (one op; it shares the storage, so it
    keeps the whole allocation alive for as long as it lives)."""
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= d
    return torch.as_strided(flat, shape, tuple(reversed(st)), off)


class _Tape:
    """What the Python chains of one block's forward left for backward.  x / x1: input of the attention / MLP half
    (behind cut / mcut); ln1 / ln2: (gamma, beta); sa / sm: what the two chains saved; pa / pm: their parameters.
    cut = (n_in, head, tail): the stream was cut from n_in rows to head + tail in front of the block, mcut: the same
    between its halves, None: no cut there.  rows: token rows (batch x rows per image) the tape holds operands for,
    both halves together (the ratio of two blocks scales the bytes their weight-gradient operands keep alive).
    dpa / dpm: (rate, seed) of the drop-path draw of the attention / MLP half, None where the half was not dropped."""
    __slots__ = ("x", "mu1", "rs1", "ln1", "sa", "x1", "mu2", "rs2", "ln2", "sm", "pa", "pm", "cut", "mcut", "rows",
                 "dpa", "dpm")
    native = False

    def __init__(self, *fields):
        for k, v in zip(self.__slots__, fields):
            setattr(self, k, v)
        self.rows = self.x.shape[0] + self.x1.shape[0]
        self.dpa = self.dpm = None


class _NativeTape:
    """What a native block forward left for backward: ONE device allocation (buf, carved by plan.off) plus the
    references a _Tape holds, under the same names.  Tensor views of the allocation are made only when somebody asks:
    the native backward needs four of them (the weight-gradient operands, through bf); the Python backward reads the
    fields of _Tape, and the first one it reads of a half makes that half's views (__getattr__).
    mcut: the MLP half ran on x1, the cut copy of the tape's x1 (held here for backward).  mlp_in_tape = False: the
    library declined that half's call, and mu2 / rs2 / sm are what the Python chain left."""
    __slots__ = ("plan", "buf", "x", "ln1", "ln2", "pa", "pm", "weff", "wc", "cut", "mcut", "rows", "mlp_in_tape",
                 "mu1", "rs1", "sa", "x1", "mu2", "rs2", "sm", "_bf", "_f32")
    native = True
    dpa = dpm = None              # (a block with an active drop-path rate never runs the native chain)

    def __init__(self, plan, buf, x, ln1, ln2, pa, pm, weff, wc, cut):
        self.plan, self.buf, self.x, self.ln1, self.ln2, self.pa, self.pm = plan, buf, x, ln1, ln2, pa, pm
        self.weff, self.wc, self.cut, self.mcut, self.mlp_in_tape = weff, wc, cut, None, True
        self.rows = plan.M + plan.Mm
        self._bf = self._f32 = None

    def bf(self, name, *shape):
        if self._bf is None:
            self._bf = self.buf.view(torch.bfloat16)
        return _carve(self._bf, self.plan.off[name][0] // 2, shape)

    def f32(self, name, *shape):
        if self._f32 is None:
            self._f32 = self.buf.view(torch.float32)
        return _carve(self._f32, self.plan.off[name][0] // 4, shape)

    def __getattr__(self, name):
        """Reached for a slot that is still empty: the Python backward reads one half of this tape.  Fills that half's
        slots with what EncoderOp.fwd's Python path would have saved there, once."""
        if name in ("mu1", "rs1", "sa"):
            pl = self.plan
            M, D = pl.M, pl.D
            lse = self.f32("lse", pl.B, pl.H, pl.n) if pl.off["lse"][1] else None
            self.sa = MHLASaved(xn=self.bf("xn1", M, D), weff=self.weff, qkv=self.bf("qkv", M, 3 * D), o=self.bf("o", M, D),
                                wp_c=self.wc[0], mask=None, B=pl.B, L=pl.n, p_attn=0.0, seed_attn=0, p_proj=0.0,
                                seed_proj=0, prm=self.pa, lse=lse)
            self.mu1, self.rs1 = self.f32("mu1", M), self.f32("rs1", M)
        elif name in ("x1", "mu2", "rs2", "sm"):
            pl = self.plan
            Mm, D, Hd = pl.Mm, pl.D, pl.hidden
            self.sm = MLPSaved(xn=self.bf("xn2", Mm, D), pre=self.bf("pre", Mm, Hd),
                               pre_is_grad=MLPChain.saves_gelu_grad(torch.bfloat16), h=self.bf("h", Mm, Hd),
                               w1_c=self.wc[1], w2_c=self.wc[2], p=0.0, seed_fc1=0, seed_fc2=0, prm=self.pm)
            self.mu2, self.rs2 = self.f32("mu2", Mm), self.f32("rs2", Mm)
            if self.mcut is None:
                self.x1 = self.f32("x1", pl.M, D)
        else:
            raise AttributeError(name)
        return getattr(self, name)


class EncoderOp:
    """A stack of pre-LN blocks on the fp32 residual stream [B, L, D]:
    x += attn(LN1(x)); x += mlp(LN2(x)).
    cuts (CLS-only mode, see cls_plan): per block the (head, tail) rows it runs on, or None for all rows.  The stream
    is cut to a block's rows in front of it (favit_rows_cut_fwd), the block runs on the compact [B, n, D] tensor with
    L = n throughout, and the output keeps the last block's rows; backward expands at the same points
    (favit_rows_cut_bwd).
    mlp_cuts (mlp_narrow_plan): per block the (head, tail) rows its MLP half runs on, or None.  The stream is then cut
    inside the block, after proj + residual, and the next block finds its rows in place: the cut in front of it moves
    up into this block.

    Stochastic depth.  A half is "dropped" iff `training` and its block's BlockSpec.drop_path
    is > 0: x += keep(b) / (1 - p) * branch(LN(x)) per sample b.  Its chain runs with residual=None (the proj / fc2
    GEMM writes the fp32 branch, output dropout still in its epilogue) and K.drop_path_add makes the sum on the half's
    own row count; backward scales and masks the branch gradient in K.drop_path_bwd (which also carries the branch's
    output-dropout mask, so the chain runs premasked) while the LayerNorm backward keeps adding the unscaled stream
    gradient.  The draw is indexed by the sample alone: pruning (cuts / mlp_cuts) does not change it.
    SEED ORDER (part of the interface; tests rebuild the masks from it): one _seed() per dropped half, drawn right
    AFTER the dropout seeds of that half's own chain (attention: p_attn, then p_proj; MLP: fc1, then fc2, each only
    where its rate is > 0); within a block the attention half first, then the MLP half; blocks in order.  A half
    with rate 0, and every half in eval mode, draws nothing and runs exactly the code it ran before.
    fp8 compute mode with an active rate raises NotImplementedError (the q8 hand-offs between the LayerNorm backward
    and the GEMMs are not covered)."""

    def __init__(self, blocks: List[BlockSpec], mask=None, training=False, cuts=None, mlp_cuts=None):
        self.blocks, self.mask, self.training = blocks, mask, training
        self.cuts = list(cuts) if cuts is not None else None
        if self.cuts is not None and (len(self.cuts) != len(blocks) or mask is not None):
            raise ValueError("cuts: one entry per block, and no attention mask")
        self.mlp_cuts = list(mlp_cuts) if mlp_cuts is not None else None
        if self.mlp_cuts is not None and (self.cuts is None or len(self.mlp_cuts) != len(blocks)):
            raise ValueError("mlp_cuts: one entry per block of an encoder with cuts")

    def fwd(self, ins, prm):
        (x,) = ins
        B, L, D = x.shape
        M = B * L
        L_in = L
        cdt = get_compute_dtype()
        x = _as_f32(x).reshape(M, D)
        tapes = []
        # the latent_proj folds only depend on parameters: all MHLA blocks of equal geometry in ONE launch
        pre = [None] * len(self.blocks)
        idx, fp, off = [], [], 0
        for bi, bs in enumerate(self.blocks):
            if isinstance(bs.attn, MHLAChain):
                idx.append(bi)
                fp.append(tuple(prm[off + 2:off + 6]))
            off += bs.n
        if 2 <= len(idx) <= 32 and len({(self.blocks[i].attn.H, tuple(q[0].shape)) for i, q in zip(idx, fp)}) == 1:
            for bi, we in zip(idx, K.mhla_fold_fwd_multi(fp, self.blocks[idx[0]].attn.H, cdt)):
                pre[bi] = we
        native = self.mask is None and x.is_cuda and _native_blocks_on()
        off = 0
        for bi, bs in enumerate(self.blocks):
            g1, b1, pa, g2, b2, pm = p = bs.split(list(prm[off:off + bs.n]))
            off += bs.n
            # 1. the cut in front of the block
            cut = None
            if self.cuts is not None and self.cuts[bi] is not None and sum(self.cuts[bi]) < L:
                ca, cb = self.cuts[bi]
                x = K.rows_cut_fwd(x, B, L, ca, cb, D).reshape(B * (ca + cb), D)
                cut = (L, ca, cb)
                L = ca + cb
                M = B * L
            mc = self.mlp_cuts[bi] if self.mlp_cuts is not None else None
            if mc is not None and sum(mc) >= L:
                mc = None
            dp = self.drop_path_of(bs)
            if dp > 0 and _STATE.get("fp8"):
                raise NotImplementedError("stochastic depth (drop_path > 0) in training is not implemented in the fp8 "
                                          "compute mode; use bf16 or fp32")
            # 2. the attention half, x1 = x + attn(LN1(x)) (the library runs a block without an inner cut whole)
            nt = self._fwd_native(bs, p, x, B, L, D, pre[bi], cut, mc) if native and pre[bi] is not None else None
            dpa = dpm = None
            if nt is None:
                x1, mu1, rs1, sa = self._attn_half_fwd(bs, pa, x, g1, b1, B, L, D, cdt, pre[bi], branch=dp > 0)
                if dp > 0:                    # x1 holds the branch: the sum goes back into it
                    dpa = (dp, _seed())
                    x1 = K.drop_path_add(x, x1, B, L, D, dp, dpa[1], out=x1)
            elif mc is not None:
                x1 = nt.f32("x1", M, D)
            # 3. the cut between the halves, to the rows the next block reads: everything from here on is row-wise
            mcut = None
            if mc is not None:
                x1 = K.rows_cut_fwd(x1, B, L, mc[0], mc[1], D).reshape(B * sum(mc), D)
                mcut = (L, mc[0], mc[1])
                L = sum(mc)
                M = B * L
            # 4. the MLP half, x2 = x1 + mlp(LN2(x1)), and the block's tape
            if nt is None:
                xn2, mu2, rs2, sm, x2 = self._mlp_half_fwd(bs, pm, x1, g2, b2, M, D, cdt, branch=dp > 0)
                if dp > 0:                    # (L: the rows of this half, behind mcut)
                    dpm = (dp, _seed())
                    x2 = K.drop_path_add(x1, x2, B, L, D, dp, dpm[1], out=x2)
                tapes.append(_Tape(x, mu1, rs1, (g1, b1), sa, x1, mu2, rs2, (g2, b2), sm, pa, pm, cut, mcut))
                tapes[-1].dpa, tapes[-1].dpm = dpa, dpm
                x = x2
                continue
            if mcut is not None:
                # the second call on the descriptor the attention half filled; where the library declines it, the
                # Python chain runs the half and the tape holds its tensors
                nt.mcut, nt.x1 = mcut, x1
                if K.mhla_block_mlp_fwd(nt.plan, x1) != 0:
                    nt.mlp_in_tape = False
                    _, nt.mu2, nt.rs2, nt.sm, x2 = self._mlp_half_fwd(bs, pm, x1, g2, b2, M, D, cdt)
            tapes.append(nt)
            x = nt.f32("x2", M, D) if nt.mlp_in_tape else x2
        return x.reshape(B, L, D), (tapes, B, L_in, D)

    def drop_path_of(self, bs) -> float:
        """The stochastic depth rate in force for both halves of block bs: its rate in training mode, else 0."""
        return bs.drop_path if self.training else 0.0

    def _attn_half_fwd(self, bs, pa, x, g1, b1, B, L, D, cdt, pre, branch=False):
        """LayerNorm 1 and the attention chain on the B * L rows of x (the Python chains).  branch: the chain runs
        without its residual and the first result is attn(LN1(x)) alone (a dropped half)."""
        M = B * L
        kw = {"pre": pre} if pre is not None else {}
        xn1, mu1, rs1 = K.layernorm_fwd(x, D, g1, b1, M, D, cdt, q8=_q8_request(bs.attn, pa, "fwd", D))
        x1, sa = bs.attn.fwd(xn1, pa, B, L, None if branch else x, self.mask, self.training, **kw)
        return x1, mu1, rs1, sa

    def _mlp_half_fwd(self, bs, pm, x1, g2, b2, M, D, cdt, branch=False):
        """LayerNorm 2 and the MLP chain on the M rows of x1 (the Python chains).  branch: as in _attn_half_fwd."""
        xn2, mu2, rs2 = K.layernorm_fwd(x1, D, g2, b2, M, D, cdt, q8=_q8_request(bs.mlp, pm, "fwd", D))
        x2, sm = bs.mlp.fwd(xn2, pm, None if branch else x1, self.training)
        return xn2, mu2, rs2, sm, x2

    def _fwd_native(self, bs, p, x, B, L, D, pre, cut, mc):
        """One block's forward as one library call, or None where this block runs the Python chains: not MHLA + MLP, a
        dropout that is active in this mode, parameters of another dtype or shape than the chain assumes, a geometry
        the library declines (favit_mhla_block_tape_layout), or a declined call (nothing was launched then).
        p: BlockSpec.split of the block's parameters.  mc = (head, tail): the MLP half will run on those rows -- this
        call is the attention half then (x1 is in the tape), and EncoderOp.fwd follows with the Python-visible row cut
        of x1 and the MLP half as a second call on the same descriptor."""
        at, ml = bs.attn, bs.mlp
        g1, b1, pa, g2, b2, pm = p
        if not (isinstance(at, MHLAChain) and isinstance(ml, MLPChain)) or (len(pa), len(pm)) != (len(at.names), len(ml.names)):
            return None
        if self.training and (at.p_attn > 0 or at.p_proj > 0 or ml.p > 0) or self.drop_path_of(bs) > 0:
            return None
        (wqkv, bqkv, wl, bl, wp, bp), (w1, c1, w2, c2) = pa, pm
        Hd = w1.shape[0]
        if tuple(w2.shape) != (D, Hd) or tuple(w1.shape) != (Hd, D) or tuple(wp.shape) != (D, D):
            return None
        if any(t.dtype != torch.float32 or not t.is_contiguous() for t in (g1, b1, g2, b2, bp, c1, c2)):
            return None
        weff, beff = pre
        wc = (wcast(wp), wcast(w1), wcast(w2))
        if weff.dtype != torch.bfloat16 or any(w.dtype != torch.bfloat16 or not w.is_contiguous() for w in wc):
            return None
        # the plan (descriptor geometry + layouts) is kept on the block's first parameter, per shape: it lives and
        # dies with the block
        plans = getattr(g1, "_favit_blocks", None)
        if plans is None:
            plans = g1._favit_blocks = {}
        key = (B, L, D, at.H, at.W, Hd, bool(self.training))
        if mc is not None:
            key += (sum(mc),)
        if key not in plans:
            plans[key] = K.mhla_block_plan(*key[:7], n_mlp=sum(mc)) if mc is not None else K.mhla_block_plan(*key)
        plan = plans[key]
        if plan is None:
            return None
        buf = torch.empty(plan.tape_bytes, dtype=torch.uint8, device=x.device)
        if K.mhla_block_fwd(plan, x, buf, g1, b1, g2, b2, weff, beff, wc[0], bp, wc[1], c1, wc[2], c2) != 0:
            return None
        return _NativeTape(plan, buf, x, (g1, b1), (g2, b2), pa, pm, weff, wc, cut)

    def _bwd_native(self, bs, tp, g, g_lp, handed=None):
        """The input-gradient chain of a block with a native tape as one library call -- of a narrowed block
        (tp.mcut) its attention half, g / g_lp being the expanded gradient of x1 -- then what MLPChain.bwd,
        MHLAChain.bwd and _ln_bwd do besides launching it: the weight-gradient problems and the deferred folds, in
        their order.  Returns (g, g_lp or None, attention grads, mlp grads or None for a half), or None where the
        Python chains have to run (a LayerNorm parameter without a gradient buffer, a gradient of another layout, a
        declined call).
        handed = (arena, its bf16 view, its fp32 view) from _bwd_native_mlp: that call was taken on tp.plan in this
        iteration of EncoderOp.bwd and only the row cut came since, so the descriptor holds this block's pointers and
        the stream (ptrs_set), LayerNorm 2 has its gradient buffers, and g / g_lp come from the row cut.  Plans are
        shared by every tape of one shape: in any other case the pointers have to be written again.
        Lifetime: every buffer the queued launches read or write is a VIEW of the arena or of the tape, held by
        the backward queue (_QUEUE) until those launches have been issued; nothing is freed or reused before."""
        plan = tp.plan
        g1, g2 = tp.ln1[0], tp.ln2[0]
        tg = [_gt(q) for q in (tp.ln1 if handed is not None else tp.ln1 + tp.ln2)]
        if any(t is None for t in tg):
            return None
        M, D, Hd = plan.M, plan.D, plan.hidden
        want_lp = tp.cut is None
        if handed is None and (g.dtype != torch.float32 or g_lp.dtype != torch.bfloat16 or tuple(g.shape) != (M, D)
                               or not g.is_contiguous() or tuple(g_lp.shape) != (M, D) or not g_lp.is_contiguous()):
            return None
        arena, abf, af = handed or (torch.empty(plan.bwd_bytes[want_lp], dtype=torch.uint8, device=g.device), None, None)
        if K.mhla_block_bwd(plan, tp.x, tp.buf, g1, g2, tp.weff, *tp.wc, g, g_lp, arena, want_lp,
                            ptrs_set=handed is not None) != 0:
            return None
        bo = plan.boff[want_lp]
        if handed is None:
            abf, af = arena.view(torch.bfloat16), arena.view(torch.float32)
        part = lambda k: _carve(af, bo[k][0] // 4, (2, plan.nparts, D))
        gm = None
        if tp.mcut is None:                   # the whole block: its MLP half's problems and fold come first
            dw2, db2 = bs.mlp.fc2_grads(g_lp, tp.bf("h", M, Hd), tp.pm)
            dw1, db1 = bs.mlp.fc1_grads(_carve(abf, bo["dpre"][0] // 2, (M, Hd)), tp.bf("xn2", M, D), tp.pm)
            _QUEUE.ln_folds.append(_LNFold(part("part2"), tg[2], tg[3], tp.ln2))
            gm = [dw1, db1, dw2, db2]
            g_lp = _carve(abf, bo["g1_lp"][0] // 2, (M, D))         # the gradient of x1 the call left
        dqkv = _carve(abf, bo["dqkv"][0] // 2, (M, 3 * D))
        dwp, dbp = bs.attn.proj_grads(g_lp, tp.bf("o", M, D), tp.pa)
        ga = bs.attn.qkv_grads(dqkv, tp.bf("xn1", M, D), tp.pa) + [dwp, dbp]
        _QUEUE.ln_folds.append(_LNFold(part("part1"), tg[0], tg[1], tp.ln1))
        g_out = _carve(af, bo["g_out_f32"][0] // 4, (M, D))
        return g_out, (_carve(abf, bo["g_out_lp"][0] // 2, (M, D)) if want_lp else None), ga, gm

    def _bwd_native_mlp(self, bs, tp, g, g_lp):
        """The MLP half of a narrowed block's input-gradient chain as one library call (dpre, dxn2, LayerNorm 2
        backward on the half's rows), with the weight-gradient problems and the deferred fold MLPChain.bwd and _ln_bwd
        queue.  Returns what _mlp_half_bwd returns, or None (then the Python chain runs the half).  handed: the block's
        arena with its two views, for _bwd_native to issue the attention half into after the row cut."""
        plan = tp.plan
        g1, g2 = tp.ln1[0], tp.ln2[0]
        tg2, tb2 = _gt(g2), _gt(tp.ln2[1])
        if tg2 is None or tb2 is None or not tp.mlp_in_tape:
            return None
        Mm, D, Hd = plan.Mm, plan.D, plan.hidden
        if (g.dtype != torch.float32 or g_lp.dtype != torch.bfloat16 or tuple(g.shape) != (Mm, D) or not g.is_contiguous()
                or tuple(g_lp.shape) != (Mm, D) or not g_lp.is_contiguous()):
            return None
        want_lp = tp.cut is None
        arena = torch.empty(plan.bwd_bytes[want_lp], dtype=torch.uint8, device=g.device)
        if K.mhla_block_mlp_bwd(plan, tp.x, tp.buf, g1, g2, tp.weff, *tp.wc, tp.x1, g, g_lp, arena, want_lp) != 0:
            return None
        bo = plan.boff[want_lp]
        abf, af = arena.view(torch.bfloat16), arena.view(torch.float32)
        dw2, db2 = bs.mlp.fc2_grads(g_lp, tp.bf("h", Mm, Hd), tp.pm)
        dw1, db1 = bs.mlp.fc1_grads(_carve(abf, bo["dpre"][0] // 2, (Mm, Hd)), tp.bf("xn2", Mm, D), tp.pm)
        _QUEUE.ln_folds.append(_LNFold(_carve(af, bo["part2"][0] // 4, (2, plan.nparts2, D)), tg2, tb2, tp.ln2))
        g1_f32 = _carve(af, bo["g1_f32"][0] // 4, (Mm, D))
        return g1_f32, None, [None, None], [dw1, db1, dw2, db2], torch.bfloat16, (arena, abf, af)

    @staticmethod
    def _ln_bwd(dxn, xin, ln, mu, rs, dres, pd, q8=None, want_lp=True):
        """LayerNorm backward of the stream; the dgamma / dbeta fold joins the deferred batch when the parameters own
        gradient buffers (the fused-optimizer flow).  q8: the low-precision copy also leaves quantised (fp8 mode).
        want_lp=False: a row cut follows, and favit_rows_cut_bwd writes the copy of the expanded gradient."""
        gam, bet = ln
        M, D = xin.shape
        if not gam.requires_grad and not bet.requires_grad:      # frozen layer: no dgamma / dbeta fold at all
            return K.layernorm_bwd(dxn, xin, D, gam, mu, rs, M, D, dres=dres, want_lp=want_lp, lp_drop=pd, frozen=True, q8=q8)
        tg_, tb_ = _gt(gam), _gt(bet)
        q = _QUEUE
        lst = [] if (q is not None and q.defer and tg_ is not None and tb_ is not None) else None
        out = K.layernorm_bwd(dxn, xin, D, gam, mu, rs, M, D, dres=dres, want_lp=want_lp, dg_out=tg_, db_out=tb_,
                              lp_drop=pd, defer=lst, q8=q8)
        if lst is not None:
            q.ln_folds.extend(_LNFold(*e, ready=(gam, bet)) for e in lst)
        elif out[2] is None:
            _ready(gam, bet)
        return out

    def _mlp_half_bwd(self, bs, tp, g, g_lp, premasked, nat_ok):
        """Backward of x2 = x1 + mlp(LN2(x1)) on the half's rows, from the library (a narrowed native tape that holds
        the half) or from the Python chain.  Returns (gradient of x1, its low-precision copy or None where the row cut
        that follows writes it, [dgamma2, dbeta2], the chain's parameter gradients, the dtype of that copy, and the
        arena for _bwd_native where the library took the call, else None)."""
        done = self._bwd_native_mlp(bs, tp, g, g_lp) if nat_ok and tp.mcut is not None else None
        if done is not None:
            return done
        dxn2, gm = bs.mlp.bwd(tp.sm, g_lp, premasked=premasked)
        # the mask of the attention branch's output dropout (a native forward had none: its attention views stay
        # unmade); fp8 mode: the copy feeds this block's proj input-gradient GEMM as its dY -- consumed as it is
        # written, since a branch with output dropout gets it pre-masked
        # (a dropped attention half makes its own copy from the stream gradient, K.drop_path_bwd: none is written here)
        pd = (0.0, 0) if tp.native or tp.dpa is not None else bs.attn.out_dropout(tp.sa)
        g, g_lp, dg2, db2 = self._ln_bwd(dxn2, tp.x1, tp.ln2, tp.mu2, tp.rs2, g, pd,
                                         want_lp=tp.mcut is None and tp.dpa is None,
                                         q8=_q8_request(bs.attn, tp.pa, "bwd", g.shape[1]))
        return g, g_lp, [dg2, db2], gm, dxn2.dtype, None

    def _attn_half_bwd(self, bs, tp, g, g_lp, pd_n, q8n, nat_ok, handed, want_lp=True):
        """Backward of x1 = x + attn(LN1(x)) on the block's rows, likewise.  pd_n / q8n: what the low-precision copy
        of the result has to carry for the block below.  Returns (gradient of x, its low-precision copy or None where
        a row cut follows, [dgamma1, dbeta1], the chain's parameter gradients, the dtype of that copy)."""
        done = self._bwd_native(bs, tp, g, g_lp, handed) if nat_ok and tp.mcut is not None else None
        if done is not None:
            g, g_lp, ga, _ = done
            return g, g_lp, [None, None], ga, torch.bfloat16
        sa = tp.sa
        dxn1, ga = bs.attn.bwd(sa, g_lp, premasked=bs.attn.out_dropout(sa)[0] > 0)
        g, g_lp, dg1, db1 = self._ln_bwd(dxn1, tp.x, tp.ln1, tp.mu1, tp.rs1, g, pd_n, q8=q8n,
                                         want_lp=want_lp and tp.cut is None)
        return g, g_lp, [dg1, db1], ga, dxn1.dtype

    def bwd(self, saved, dy, needs):
        tapes, B, L, D = saved
        g = dy.reshape(-1, D)
        cdt = get_compute_dtype()
        g_lp = g if tapes and tapes[-1].dpm is not None else _as_cdt(g)      # (a dropped half makes its own copy)
        grads = []

        def expand(g, cut, lp_dtype):
            # back over a row cut: zeros in the rows it dropped, and the compute-dtype copy the next backward GEMMs read
            # written in the same pass (lp_dtype; None: no copy)
            n_in, ca, cb = cut
            g, g_lp = K.rows_cut_bwd(g, B, n_in, ca, cb, D, lp_dtype=lp_dtype)
            g = g.reshape(B * n_in, D)
            return g, (g_lp.reshape(B * n_in, D) if g_lp is not None else g)
        with _BackwardQueue(per_block=any(tp.cut is not None or tp.mcut is not None for tp in tapes),
                            zero_floats=sum(3 * D + 4 for bs in self.blocks if isinstance(bs.attn, MHLAChain)),
                            device=dy.device) as queue:
            # The low-precision copy of the stream gradient only feeds the next branch's backward GEMMs; when that
            # branch's output was dropped in forward, the LayerNorm backward that produces the copy applies the mask
            # (no separate masking pass: 24 launches of 28 us per cfg2 step at dropout 0.1).
            order = list(zip(reversed(self.blocks), reversed(tapes)))
            premasked = False
            for bi, (bs, tp) in enumerate(order):
                nbs, ntp = order[bi + 1] if bi + 1 < len(order) else (None, None)
                # what the low-precision copy of this block's input gradient has to carry for the block below
                # (a native tape there: no dropout was active and the mode is bf16, so nothing)
                pd_n, q8n = (0.0, 0), None
                if ntp is not None and not ntp.native and ntp.dpm is None:
                    pd_n = nbs.mlp.out_dropout(ntp.sm)
                    q8n = _q8_request(nbs.mlp, ntp.pm, "bwd", D)       # the next block's fc2 input-gradient GEMM
                # the block below starts with a dropped half: it makes its copy itself, none is written for it
                lp_below = ntp is not None and ntp.dpm is None
                nat_ok = (tp.native and not premasked and pd_n[0] == 0 and q8n is None and queue.defer
                          and _native_blocks_on())
                whole = self._bwd_native(bs, tp, g, g_lp) if nat_ok and tp.mcut is None else None
                if whole is not None:         # the block without an inner cut: ONE library call
                    (g, g_lp, ga, gm), ln1_g, ln2_g, lp_dt = whole, [None, None], [None, None], torch.bfloat16
                else:
                    if tp.dpm is not None:
                        # a dropped MLP half: its branch gradient is the stream gradient scaled per sample, under the
                        # mask of the branch's output dropout; the stream gradient itself goes on unscaled (dres)
                        g_lp = K.drop_path_bwd(g, cdt, B, g.shape[0] // B, D, *tp.dpm, lp_drop=bs.mlp.out_dropout(tp.sm))
                        premasked = True
                    g, g_lp, ln2_g, gm, lp_dt, handed = self._mlp_half_bwd(bs, tp, g, g_lp, premasked, nat_ok)
                    if tp.mcut is not None:
                        # the MLP half ran on the rows the block above reads: back to this block's rows
                        g, g_lp = expand(g, tp.mcut, lp_dt if g.dtype != lp_dt and tp.dpa is None else None)
                    if tp.dpa is not None:
                        g_lp = K.drop_path_bwd(g, cdt, B, g.shape[0] // B, D, *tp.dpa, lp_drop=bs.attn.out_dropout(tp.sa))
                    g, g_lp, ln1_g, ga, lp_dt = self._attn_half_bwd(bs, tp, g, g_lp, pd_n, q8n, nat_ok, handed,
                                                                    want_lp=lp_below or ntp is None)
                premasked = pd_n[0] > 0
                if tp.cut is not None:
                    # this block ran on its (head, tail) rows: back to the rows of the block below
                    g, g_lp = expand(g, tp.cut, lp_dt if lp_below and g.dtype != lp_dt else None)
                if queue.end_block((tp.rows, ntp.rows) if ntp is not None else None) and _STATE["grad_ready"] is not None:
                    queue.flush_deferred()
                if not _SIDE["enabled"]:
                    join_side_stream()
                grads = ln1_g + ga + ln2_g + gm + grads
        return [g.reshape(B, L, D)], grads


class FinalNormOp:
    """norm(x)[:, 0] (models/vit.py:303-307): only the CLS row of the last LayerNorm is computed."""

    def fwd(self, ins, prm):
        (x,), (g, b) = ins, prm
        B, L, D = x.shape
        x = _as_f32(x)
        y, mu, rs = K.layernorm_fwd(x, L * D, g, b, B, D, torch.float32)
        return y, (x, mu, rs, (g, b), (B, L, D))

    def bwd(self, saved, dy, needs):
        x, mu, rs, (g, b), (B, L, D) = saved
        dx = torch.zeros((B, L, D), dtype=torch.float32, device=x.device)
        _, _, dg, db = K.layernorm_bwd(dy, x, L * D, g, mu, rs, B, D, dx=dx, lddx=L * D, dg_out=_gt(g), db_out=_gt(b))
        if dg is None:
            _ready(g, b)
        return [dx], [dg, db]


class HeadPoolOp:
    """The mean-pooled head (timm's global_pool='avg'): the mean over the token rows [first, L) in place of the CLS row.
    norm_first: norm(x)[:, first:].mean(1), one fused launch pair per direction (kernels.ln_meanpool_fwd / _bwd);
    otherwise norm(x[:, first:].mean(1)), timm's fc_norm order (kernels.meanpool_fwd / _bwd around the LayerNorm of
    the B pooled rows).  Reads every row of x, so the encoder in front of it runs all rows (no cls_only cuts)."""

    def __init__(self, norm_first: bool, first: int = 1, eps: float = 1e-5):
        self.norm_first, self.first, self.eps = bool(norm_first), int(first), float(eps)

    def fwd(self, ins, prm):
        (x,), (g, b) = ins, prm
        B, L, D = x.shape
        x = _as_f32(x).contiguous()
        if self.norm_first:
            y, s, mu, rs = K.ln_meanpool_fwd(x, g, b, self.first, self.eps)
            return y, (x, s, mu, rs, (g, b), L)
        p = K.meanpool_fwd(x, self.first)
        y, mu, rs = K.layernorm_fwd(p, D, g, b, B, D, torch.float32, self.eps)
        return y, (None, p, mu, rs, (g, b), L)

    def bwd(self, saved, dy, needs):
        x, s, mu, rs, (g, b), L = saved
        dy = dy.contiguous()
        if self.norm_first:
            dx, dg, db = K.ln_meanpool_bwd(dy, x, g, s, mu, rs, self.first, dg_out=_gt(g), db_out=_gt(b))
        else:
            B, D = s.shape
            dp, _, dg, db = K.layernorm_bwd(dy, s, D, g, mu, rs, B, D, dg_out=_gt(g), db_out=_gt(b))
            dx = K.meanpool_bwd(dp, L, self.first)
        if dg is None:
            _ready(g, b)
        return [dx], [dg, db]


class AttnOp:
    """Stand-alone attention module on fp32 [B, L, D] (no LayerNorm, no residual)."""

    def __init__(self, chain, mask=None, training=False):
        self.chain, self.mask, self.training = chain, mask, training

    def fwd(self, ins, prm):
        (x,) = ins
        B, L, D = x.shape
        xn = _as_cdt(x.reshape(B * L, D))
        y, saved = self.chain.fwd(xn, list(prm), B, L, None, self.mask, self.training)
        return y.reshape(B, L, D), (saved, (B, L, D))

    def bwd(self, saved, dy, needs):
        s, (B, L, D) = saved
        dxn, grads = self.chain.bwd(s, _as_cdt(dy.reshape(B * L, D)))
        return [_as_f32(dxn).reshape(B, L, D)], grads


class MLPOp:
    def __init__(self, chain, training=False):
        self.chain, self.training = chain, training

    def fwd(self, ins, prm):
        (x,) = ins
        shp = x.shape
        xn = _as_cdt(x.reshape(-1, shp[-1]))
        y, saved = self.chain.fwd(xn, list(prm), None, self.training)
        return y.reshape(*shp[:-1], y.shape[-1]), (saved, shp)

    def bwd(self, saved, dy, needs):
        s, shp = saved
        dxn, grads = self.chain.bwd(s, _as_cdt(dy.reshape(-1, dy.shape[-1])))
        return [_as_f32(dxn).reshape(shp)], grads


class CrossAttnOp:
    """Stand-alone (MultiHead)CrossAttention on fp32 query [B,Lq,D], key_value [B,Lk,D]."""

    def __init__(self, chain, mask=None, training=False):
        self.chain, self.mask, self.training = chain, mask, training

    def fwd(self, ins, prm):
        q, kv = ins
        B, Lq, D = q.shape
        Lk = kv.shape[1]
        qn, kn = _as_cdt(q.reshape(B * Lq, D)), _as_cdt(kv.reshape(B * Lk, D))
        y, saved = self.chain.fwd(qn, kn, list(prm), B, Lq, Lk, None, self.mask, self.training)
        return y.reshape(B, Lq, D), (saved, (B, Lq, Lk, D))

    def bwd(self, saved, dy, needs):
        s, (B, Lq, Lk, D) = saved
        dqn, dkn, grads = self.chain.bwd(s, _as_cdt(dy.reshape(B * Lq, D)))
        return [_as_f32(dqn).reshape(B, Lq, D), dkn.reshape(B, Lk, D)], grads


class CrossBlockOp:
    """CrossAttentionTransformerBlock.forward (models/attention.py:194-219)."""

    def __init__(self, chain, mlp, mask=None, training=False):
        self.chain, self.mlp, self.mask, self.training = chain, mlp, mask, training
        self.names = (("norm1_query.weight", "norm1_query.bias", "norm1_kv.weight", "norm1_kv.bias") +
                      tuple("attn." + n for n in chain.names) + ("norm2.weight", "norm2.bias") +
                      tuple("mlp." + n for n in mlp.names))

    def fwd(self, ins, prm):
        q, kv = ins
        B, Lq, D = q.shape
        Lk = kv.shape[1]
        Mq, Mk = B * Lq, B * Lk
        cdt = get_compute_dtype()
        p = list(prm)
        q2, kv2 = _as_f32(q).reshape(Mq, D), _as_f32(kv).reshape(Mk, D)
        qn, muq, rsq = K.layernorm_fwd(q2, D, p[0], p[1], Mq, D, cdt)
        kn, muk, rsk = K.layernorm_fwd(kv2, D, p[2], p[3], Mk, D, cdt)
        x1, sa = self.chain.fwd(qn, kn, p[4:12], B, Lq, Lk, q2, self.mask, self.training)
        xn2, mu2, rs2 = K.layernorm_fwd(x1, D, p[12], p[13], Mq, D, cdt)
        x2, sm = self.mlp.fwd(xn2, p[14:], x1, self.training)
        return x2.reshape(B, Lq, D), (q2, kv2, muq, rsq, muk, rsk, sa, x1, mu2, rs2, sm, p, (B, Lq, Lk, D))

    def bwd(self, saved, dy, needs):
        q2, kv2, muq, rsq, muk, rsk, sa, x1, mu2, rs2, sm, p, (B, Lq, Lk, D) = saved
        Mq, Mk = B * Lq, B * Lk
        g = dy.reshape(Mq, D)
        dxn2, gm = self.mlp.bwd(sm, _as_cdt(g))
        g, g_lp, dg2, db2 = K.layernorm_bwd(dxn2, x1, D, p[12], mu2, rs2, Mq, D, dres=g, want_lp=True)
        dqn, dkn, ga = self.chain.bwd(sa, g_lp)
        dq, _, dgq, dbq = K.layernorm_bwd(dqn, q2, D, p[0], muq, rsq, Mq, D, dres=g)
        dkv, _, dgk, dbk = K.layernorm_bwd(dkn, kv2, D, p[2], muk, rsk, Mk, D)
        return [dq.reshape(B, Lq, D), dkv.reshape(B, Lk, D)], [dgq, dbq, dgk, dbk] + ga + [dg2, db2] + gm


class PoolOp:
    """SuperpixelPooling.pool over a batch (models/sppp.py:192-223, models/sppp_mhla.py:286-300)."""

    def __init__(self, kind, perm, offs, R):
        self.kind, self.perm, self.offs, self.R = kind, perm, offs, R

    def fwd(self, ins, prm):
        (emb,) = ins
        emb = _as_f32(emb)
        out, argmax = K.sppp_pool_fwd(emb, self.perm, self.offs, self.kind, self.R)
        return out, (emb, argmax)

    def bwd(self, saved, dy, needs):
        emb, argmax = saved
        return [K.sppp_pool_bwd(dy, emb, self.perm, self.offs, argmax, self.kind, self.R)], []


class PosEncOp:
    """DynamicPositionalEncoding.forward, centroid branch (models/sppp.py:267-300)."""

    def __init__(self, cent):
        self.cent = cent

    def fwd(self, ins, prm):
        (x,) = ins
        return K.sppp_posenc_fwd(_as_f32(x), self.cent), None

    def bwd(self, saved, dy, needs):
        return [dy], []


class DropoutOp:
    """nn.Dropout on an fp32 activation (embedding dropout, models/vit.py:297)."""

    def __init__(self, p):
        self.p = p

    def fwd(self, ins, prm):
        s = _seed()
        return K.dropout(_as_f32(ins[0]), self.p, s), s

    def bwd(self, saved, dy, needs):
        return [K.dropout(dy, self.p, saved)], []
