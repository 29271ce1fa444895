"""Training-step harness: the counterpart of the reference's hot loop
(experiments/mhla_pretrained.py:350-372: zero_grad -> model(images) -> CrossEntropyLoss ->
backward -> AdamW.step) with the name-based parameter groups of
experiments/mhla_pretrained.py:308-327.  Loss and optimizer run in libfavit kernels
(favit_cross_entropy, favit_adamw); nothing in the step synchronises with the host.
"""
from __future__ import annotations

import contextlib
import os
import warnings
from typing import Dict, List, Optional

import torch

from . import functional as F
from . import kernels as K
from .dp import FlatBuffers, GradSync


class _CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean reduction) forward + gradient in one kernel."""

    @staticmethod
    def forward(ctx, logits, labels, label_smoothing=0.0, mix_lam=None):
        B = logits.shape[0]
        rows, dlog = K.cross_entropy(logits.contiguous(), labels.contiguous(), grad_scale=1.0 / B,
                                     label_smoothing=label_smoothing, mix_lam=mix_lam)
        ctx.save_for_backward(dlog)
        return K.reduce_rows(rows.view(B, 1))[0] / B

    @staticmethod
    def backward(ctx, g):
        (dlog,) = ctx.saved_tensors
        return dlog * g, None, None, None


class Distill:
    """How a frozen teacher enters the loss: loss = (1 - alpha) * base + alpha * kd, with base the cross-entropy of the
    labels (smoothed, mixed) and kd the distance to the teacher's logits.  kind "soft": tau^2 * KL(softmax(z / tau) ||
    softmax(x / tau)) per row (Hinton's loss; DeiT's code divides by the class count on top, a factor a caller folds
    into alpha); kind "hard": the cross-entropy against the teacher's argmax (tau unused).  Validates on construction."""
    __slots__ = ("alpha", "tau", "kind")

    def __init__(self, alpha: float, tau: float = 1.0, kind: str = "soft"):
        if kind not in ("soft", "hard"):
            raise ValueError(f"Distill: kind must be 'soft' or 'hard', got {kind!r}")
        alpha, tau = float(alpha), float(tau)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Distill: alpha must be in [0, 1], got {alpha}")
        if not (tau == tau and tau not in (float("inf"), float("-inf")) and tau > 0.0):
            raise ValueError(f"Distill: tau must be a finite number > 0, got {tau}")
        self.alpha, self.tau, self.kind = alpha, tau, kind

    @property
    def hard(self) -> bool:
        return self.kind == "hard"

    def __repr__(self):
        return f"Distill(alpha={self.alpha}, tau={self.tau}, kind={self.kind!r})"


class _DistillFn(torch.autograd.Function):
    """The distilled loss (mean reduction) forward + gradient in one kernel; the second output is the mean of kd_rows
    (for logging, no gradient).  The teacher's logits get no gradient."""

    @staticmethod
    def forward(ctx, logits, labels, label_smoothing, mix_lam, teacher_logits, alpha, tau, hard):
        B = logits.shape[0]
        rows, dlog, kd = K.cross_entropy_distill(logits.contiguous(), teacher_logits, labels.contiguous(),
                                                 grad_scale=1.0 / B, label_smoothing=label_smoothing, mix_lam=mix_lam,
                                                 alpha=alpha, tau=tau, hard=hard)
        ctx.save_for_backward(dlog)
        sums = K.reduce_rows(torch.stack((rows, kd), 1))
        kd_mean = sums[1] / B
        ctx.mark_non_differentiable(kd_mean)
        return sums[0] / B, kd_mean

    @staticmethod
    def backward(ctx, g, _g_kd):
        (dlog,) = ctx.saved_tensors
        return dlog * g, None, None, None, None, None, None, None


def cross_entropy_distill(logits: torch.Tensor, labels: torch.Tensor, teacher_logits: torch.Tensor, distill: Distill,
                          label_smoothing: float = 0.0, mix_lam: Optional[torch.Tensor] = None):
    """(loss, kd): the distilled loss of `cross_entropy` and the mean of the rows' teacher term (a device scalar without
    a gradient, for logging)."""
    if not isinstance(distill, Distill):
        raise TypeError(f"cross_entropy: distill must be a train.Distill, got {type(distill).__name__}")
    if teacher_logits is None:
        raise ValueError("cross_entropy: distill= needs teacher_logits")
    t = teacher_logits.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return _DistillFn.apply(logits, labels, float(label_smoothing), mix_lam, t, distill.alpha, distill.tau, distill.hard)


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, label_smoothing: float = 0.0,
                  mix_lam: Optional[torch.Tensor] = None, teacher_logits: Optional[torch.Tensor] = None,
                  distill: Optional[Distill] = None) -> torch.Tensor:
    """nn.CrossEntropyLoss(label_smoothing=label_smoothing)(logits, labels), mean reduction.
    mix_lam (fp32 [B] on the device, no gradient): the loss against the Mixup / CutMix target of data.BatchMix,
    lam[b] * onehot(labels[b]) + (1 - lam[b]) * onehot(labels[B-1-b]), smoothed on top; None: the plain loss.
    distill (a Distill) with teacher_logits ([B, C], detached here: the gradient goes to `logits` only): the mean of
    (1 - alpha) * that loss's row + alpha * the row's distance to the teacher (favit_cross_entropy_distill).
    distill=None is the call of before, whatever teacher_logits holds."""
    if distill is None:
        return _CrossEntropyFn.apply(logits, labels, float(label_smoothing), mix_lam)
    return cross_entropy_distill(logits, labels, teacher_logits, distill, label_smoothing, mix_lam)[0]


def _check_teacher_frozen(teacher: torch.nn.Module, opt) -> None:
    """Raise if a teacher parameter with requires_grad=True sits in `opt` (a FusedAdamW or a torch optimizer)."""
    if any(p.requires_grad for p in teacher.parameters()):
        owned = set()
        for g in getattr(opt, "groups", None) or getattr(opt, "param_groups", ()):
            flat = g.get("flat") if isinstance(g, dict) else None
            for p in (flat.params if flat is not None else g.get("params", ())):
                owned.add(id(p))
        for n, p in teacher.named_parameters():
            if p.requires_grad and id(p) in owned:
                raise ValueError(f"teacher_logits: teacher parameter {n!r} requires grad and is in the optimizer; "
                                 "the teacher must be frozen and kept out of it")


def teacher_logits(teacher: torch.nn.Module, images: torch.Tensor, opt=None) -> torch.Tensor:
    """The frozen teacher's fp32 logits for `images`: run in eval() (no dropout, no drop path) under torch.no_grad()
    (no tape); the teacher's `training` flag is restored.  opt (a FusedAdamW or a torch optimizer): raises if a
    teacher parameter with requires_grad=True sits in it -- such a teacher would be trained, not distilled from."""
    if opt is not None:
        _check_teacher_frozen(teacher, opt)
    was_training = teacher.training
    teacher.eval()
    try:
        with torch.no_grad():
            out = teacher(images)
    finally:
        teacher.train(was_training)
    return out.float()


def param_groups(model: torch.nn.Module, lr: float, head_lr: Optional[float] = None,
                 latent_lr_mult: float = 5.0, layer_decay: Optional[float] = None, no_weight_decay=None) -> List[Dict]:
    """The reference's name-based groups (experiments/mhla_pretrained.py:320-327): every
    trainable parameter whose name contains 'latent_proj' trains at 5x lr, 'head' at head_lr.

    The two fine-tuning refinements (both off by default; with both off the list is the three groups above):
    no_weight_decay="auto": parameters with ndim <= 1 (biases, LayerNorm weights) and those whose last name component
        is cls_token or pos_embed go into groups carrying "weight_decay": 0.0; the other groups carry no such key (the
        optimizer's default applies).  An iterable of name substrings exempts by name instead.
    layer_decay=d, 0 < d <= 1: with depth = 1 + the largest i of the names blocks.i.*, a parameter of layer id k trains
        at its category rate (head_lr / lr * latent_lr_mult / lr, as above) times d ** (depth + 1 - k), where
        blocks.i.* has id i + 1, names containing 'head' and the final norm.* have id depth + 1 and everything in
        front of the blocks (cls_token, pos_embed, patch_embed.*, the SPPP front end) id 0.
    With either, parameters of equal (rate, weight decay) share a group, no two groups have the same pair, and the
    groups come in descending layer id -- the order in which backward completes their gradients, so that
    FusedAdamW(fuse_groups=True) fills its arena (and its all-reduce buckets) in that order."""
    if layer_decay is not None or no_weight_decay is not None:
        return _recipe_groups(model, lr, head_lr, latent_lr_mult, layer_decay, no_weight_decay)
    base, lat, head = [], [], []
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if "head" in n:
            head.append(p)
        elif "latent_proj" in n:
            lat.append(p)
        else:
            base.append(p)
    out = [{"params": base, "lr": lr}]
    if lat:
        out.append({"params": lat, "lr": lr * latent_lr_mult})
    if head:
        out.append({"params": head, "lr": head_lr if head_lr is not None else lr})
    return [g for g in out if g["params"]]


def _recipe_groups(model, lr, head_lr, latent_lr_mult, layer_decay, no_weight_decay) -> List[Dict]:
    """param_groups with layer_decay and / or no_weight_decay (see there)."""
    import re
    if layer_decay is not None and not 0.0 < float(layer_decay) <= 1.0:
        raise ValueError(f"param_groups: layer_decay must be in (0, 1], got {layer_decay}")
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    block_of = {n: int(mt.group(1)) for n, _ in model.named_parameters()
                for mt in [re.match(r"^blocks\.(\d+)\.", n)] if mt}
    if layer_decay is not None and not block_of:
        raise ValueError("param_groups: layer_decay needs parameters named blocks.<i>.*, the model has none")
    depth = 1 + max(block_of.values()) if block_of else 0
    if no_weight_decay is None:
        exempt = lambda n, p: False
    elif isinstance(no_weight_decay, str):
        if no_weight_decay != "auto":
            raise ValueError(f"param_groups: no_weight_decay is 'auto' or an iterable of name substrings, got "
                             f"{no_weight_decay!r}")
        exempt = lambda n, p: p.ndim <= 1 or n.rsplit(".", 1)[-1] in ("cls_token", "pos_embed")
    else:
        subs = tuple(no_weight_decay)
        exempt = lambda n, p: any(s in n for s in subs)
    groups: Dict = {}
    for n, p in named:
        if n in block_of:
            k = block_of[n] + 1
        elif "head" in n or n.startswith("norm."):
            k = depth + 1
        else:
            k = 0
        if "head" in n:
            rate = head_lr if head_lr is not None else lr
        elif "latent_proj" in n:
            rate = lr * latent_lr_mult
        else:
            rate = lr
        if layer_decay is not None:
            rate = rate * layer_decay ** (depth + 1 - k)
        key = (rate, 0.0 if exempt(n, p) else None)
        g = groups.setdefault(key, {"params": [], "layer": k})
        g["params"].append(p)
        g["layer"] = max(g["layer"], k)
    out = []
    for (rate, wd), g in sorted(groups.items(), key=lambda kv: -kv[1]["layer"]):      # (stable: ties keep name order)
        out.append({"params": g["params"], "lr": rate})
        if wd is not None:
            out[-1]["weight_decay"] = wd
    return out


def ema_decay_at(decay: float, n: int, warmup: bool = False) -> float:
    """The decay of the EMA update that follows n earlier ones: `decay`, or with warm-up min(decay, (1 + n) / (10 + n))
    -- the average forgets its initial value (the untrained weights) quickly and reaches `decay` from below."""
    return min(decay, (1 + n) / (10 + n)) if warmup else decay


def _named_slots(opt: "FusedAdamW", model: torch.nn.Module):
    """{state_dict key: (group index, offset, parameter)} of every parameter the optimizer holds in a flat buffer.
    Raises ValueError for an optimizer parameter the model does not have (state is keyed by the model's names)."""
    names = {id(t): k for k, t in model.state_dict(keep_vars=True).items()}
    out = {}
    for gi, g in enumerate(opt.groups):
        for p_, o in zip(g["flat"].params, g["flat"].offsets):
            k = names.get(id(p_))
            if k is None:
                raise ValueError(f"FusedAdamW: a parameter of shape {tuple(p_.shape)} in group {gi} does not belong to "
                                 f"the model whose names key the optimizer state")
            out[k] = (gi, o, p_)
    return out


class FusedAdamW:
    """torch.optim.AdamW semantics; one favit_adamw launch per parameter group over flat
    parameter / gradient / moment buffers (and the DP all-reduce runs on the same flat
    gradient buffers, see dp.py).

    max_grad_norm: torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) in front of every update, on the device:
    step() computes the global norm of all groups' (all-reduced) gradients once (favit_grad_norm, scale = 1 / world)
    and every group's AdamW launch multiplies its gradients by the coefficient it reads from device memory
    (favit_adamw_clip) -- no host sync, no extra pass over the gradients.
    skip_nonfinite: an update whose gradient norm is inf / NaN is not applied: p, m, v and the bf16 mirror keep their
    values and `skipped_steps` counts it.  Works without max_grad_norm (the coefficient is then 1 or "skip").  The
    host-side step count behind the bias correction still advances on a skipped step (the host never learns of the
    skip): the next applied update uses bias-correction factors one step further on, which after the first few
    steps is a difference far below the update's own rounding.
    Read-outs (None when both options are off): `grad_norm`, a 0-dim fp32 device view of the last step's pre-clip
    norm, and `skipped_steps`, a 0-dim int32 device view.  Both options need at most 16 parameter groups (per-group
    layout; fuse_groups=True has no such limit).

    ema_decay (in [0, 1), None = off): every group keeps `g["ema"]`, an fp32 flat buffer laid out like flat_p and
    initialised as a copy of it, and the group's AdamW launch itself moves it towards the parameters it has just
    computed, ema = d * ema + (1 - d) * p (favit_adamw_ema / favit_adamw_clip_ema): no extra launch, no second pass
    over the parameters.  d = ema_decay_at(ema_decay, ema_updates, ema_warmup), a by-value argument of the launch;
    `ema_updates` counts the EMA updates issued so far.  On a device-side skipped step `ema_updates` still advances,
    like the step count (the launch leaves the average itself untouched).  Frozen parameters are in no flat buffer and
    are their own average.  `ema_weights()` evaluates with the average, `ema_state_dict(model)` exports it.  Under data
    parallelism every rank's average is bitwise the same (same p, same decay).

    state_dict(model) / load_state_dict(state, model): m, v and the average per parameter, keyed by the model's
    state_dict names (independent of the flat layout), the hyper-parameters per group and the counters.

    fuse_groups=True (off by default; off is the layout and the launches above): all groups live in ONE arena, each in
    a range that starts and ends on a 256-element boundary, in the order given; inside a range the tensors keep the
    4-element alignment and the reverse registration order.  step() is then one favit_adamw_multi launch per 64 groups
    with a learning rate and weight decay per range (per element the bits of the per-group launch), with the guard one
    norm over the arena in front (any number of groups); zero_grad() is one memset, ema_weights() one exchange, and one
    bf16 mirror and ONE GradSync (groups[0]["sync"] / ["mirror"], None in the others; buckets may cross groups)
    cover the arena.  `groups` keeps its keys, every buffer a view of the group's range, so schedules, checkpoints
    (interchangeable with a per-group optimizer of the same grouping), Health.report and GraphedStep work unchanged.
    betas and eps are shared by the launch: groups that differ in them raise ValueError."""

    def __init__(self, groups, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, bucket_mb=None,
                 distributed=None, wire_dtype=None, max_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                 ema_warmup=False, fuse_groups=False):
        if isinstance(groups, torch.nn.Module):
            groups = [{"params": list(groups.parameters())}]
        elif groups and not isinstance(groups[0], dict):
            groups = [{"params": list(groups)}]
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"FusedAdamW: max_grad_norm must be > 0 (or None for no clipping), got {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guard = self.max_grad_norm is not None or self.skip_nonfinite
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"FusedAdamW: ema_decay must be in [0, 1) (or None for no average), got {ema_decay}")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema_updates = 0
        self._ema_swapped = False
        self.fuse_groups = bool(fuse_groups)
        if self._guard and not self.fuse_groups and len(groups) > K.GRAD_NORM_MAX_BUFS:
            raise ValueError(f"FusedAdamW: max_grad_norm / skip_nonfinite take at most {K.GRAD_NORM_MAX_BUFS} parameter "
                             f"groups, got {len(groups)}")
        self.groups = []
        dist_on = torch.distributed.is_initialized() if distributed is None else distributed
        if self.fuse_groups:
            self._init_fused(groups, lr, betas, eps, weight_decay, bucket_mb, wire_dtype, dist_on)
            groups = []                                # (built above; the per-group loop has nothing left to do)
        for g in groups:
            flat = FlatBuffers(g["params"])
            self.groups.append({
                "flat": flat, "lr": g.get("lr", lr), "betas": g.get("betas", betas), "eps": g.get("eps", eps),
                "weight_decay": g.get("weight_decay", weight_decay),
                "m": torch.zeros_like(flat.flat_p), "v": torch.zeros_like(flat.flat_p),
                "lp": torch.empty(flat.numel, dtype=torch.bfloat16, device=flat.flat_p.device) if flat.flat_p.is_cuda else None,
                "sync": GradSync(flat, bucket_mb, wire_dtype=wire_dtype) if dist_on else None,
            })
            self.groups[-1]["mirror"] = None
            if self.groups[-1]["lp"] is not None:
                K.cast(flat.flat_p, torch.bfloat16, out=self.groups[-1]["lp"])
                self.groups[-1]["mirror"] = F.register_lp_mirror(flat.flat_p, self.groups[-1]["lp"], flat.params)
            if self.ema_decay is not None:
                if not flat.flat_p.is_cuda:
                    raise RuntimeError("FusedAdamW: ema_decay runs in HIP kernels; the parameters are on the CPU (there "
                                       "is no CPU fallback)")
                self.groups[-1]["ema"] = flat.flat_p.clone()         # allocated here: step() allocates nothing
        self.steps = 0
        self.world = torch.distributed.get_world_size() if dist_on else 1
        # norm / coefficient, skip counter and the norm kernel's workspace live as long as the optimizer: step()
        # allocates nothing (and a GraphedStep built on it keeps replaying against the same addresses)
        self.grad_norm = self.skipped_steps = None
        if self._guard:
            dev = self.groups[0]["flat"].flat_p.device if self.groups else torch.device("cuda", torch.cuda.current_device())
            if dev.type != "cuda":
                raise RuntimeError("FusedAdamW: max_grad_norm / skip_nonfinite run in HIP kernels; the parameters are "
                                   "on the CPU (there is no CPU fallback)")
            self._norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
            self._skipped = torch.zeros(1, dtype=torch.int32, device=dev)
            self._norm_ws = K.grad_norm_workspace(dev)
            self.grad_norm, self.skipped_steps = self._norm_out[0], self._skipped[0]
        syncs = [g["sync"] for g in self.groups if g["sync"] is not None]
        if syncs:
            F.set_grad_ready_hook(lambda p: [s.grad_ready(p) for s in syncs])

    def _init_fused(self, groups, lr, betas, eps, weight_decay, bucket_mb, wire_dtype, dist_on):
        """fuse_groups=True: every group is a range of ONE arena (parameters, gradients, m, v, bf16 mirror, average),
        starting and ending on a K.ADAMW_SEG_ALIGN boundary; the padding is zero and stays zero.  self.groups keeps
        its shape -- every buffer of a group is a view of its range -- so schedules, checkpoints and reports do not
        know the difference; the arena-wide objects (one GradSync, one mirror) sit in groups[0]."""
        align = K.ADAMW_SEG_ALIGN
        if not groups:
            raise ValueError("FusedAdamW: fuse_groups needs at least one parameter group")
        hyper = [(tuple(g.get("betas", betas)), g.get("eps", eps)) for g in groups]
        if any(h != hyper[0] for h in hyper):
            raise ValueError("FusedAdamW: fuse_groups shares betas and eps among all groups (one launch), got "
                             f"{sorted(set(hyper))}")
        starts, n = [], 0
        for g in groups:
            size = FlatBuffers.size_of(g["params"])
            if not size:
                raise ValueError("no trainable parameters")
            starts.append(n)
            n += (size + align - 1) // align * align
        ends = starts[1:] + [n]
        dev = next(p for p in groups[0]["params"] if p.requires_grad).device
        if self.ema_decay is not None and dev.type != "cuda":
            raise RuntimeError("FusedAdamW: ema_decay runs in HIP kernels; the parameters are on the CPU (there "
                               "is no CPU fallback)")
        new = lambda: torch.zeros(n, dtype=torch.float32, device=dev)
        a = {"p": new(), "g": new(), "m": new(), "v": new(), "lp": None, "ema": None}
        if dev.type == "cuda":
            a["lp"] = torch.empty(n, dtype=torch.bfloat16, device=dev)
        for g, s, e in zip(groups, starts, ends):
            flat = FlatBuffers(g["params"], a["p"][s:e], a["g"][s:e])
            self.groups.append({
                "flat": flat, "lr": g.get("lr", lr), "betas": g.get("betas", betas), "eps": g.get("eps", eps),
                "weight_decay": g.get("weight_decay", weight_decay), "m": a["m"][s:e], "v": a["v"][s:e],
                "lp": None if a["lp"] is None else a["lp"][s:e], "sync": None, "mirror": None,
            })
        whole = FlatBuffers.joined([g["flat"] for g in self.groups], starts, a["p"], a["g"])
        if dist_on:
            self.groups[0]["sync"] = GradSync(whole, bucket_mb, wire_dtype=wire_dtype)   # buckets may cross groups
        if a["lp"] is not None:
            K.cast(a["p"], torch.bfloat16, out=a["lp"])
            self.groups[0]["mirror"] = F.register_lp_mirror(a["p"], a["lp"], whole.params)
        if self.ema_decay is not None:
            a["ema"] = a["p"].clone()
            for g, s, e in zip(self.groups, starts, ends):
                g["ema"] = a["ema"][s:e]
        self._arena, self._arena_flat, self._starts, self._ends = a, whole, starts, ends
        # one launch per K.ADAMW_MAX_SEGMENTS groups: the views every launch takes, made once (step() allocates nothing)
        self._launches = []
        for i in range(0, len(groups), K.ADAMW_MAX_SEGMENTS):
            j = min(len(groups), i + K.ADAMW_MAX_SEGMENTS)
            lo, hi = starts[i], ends[j - 1]
            self._launches.append((i, j, [e - lo for e in ends[i:j]],
                                   {k: (None if t is None else t[lo:hi]) for k, t in a.items()}))

    def no_sync(self):
        """Gradient accumulation under data parallelism: ``with opt.no_sync(): loss.backward()`` for every
        micro-batch but the last (dp.GradSync.no_sync)."""
        import contextlib
        stack = contextlib.ExitStack()
        for g in self.groups:
            if g["sync"] is not None:
                stack.enter_context(g["sync"].no_sync())
        return stack

    def zero_grad(self):
        if self.fuse_groups:
            sync = self.groups[0]["sync"]
            if sync is not None and (sync._handles or any(sync._launched)):
                sync.abort()                           # (as below)
            self._arena_flat.zero_grad()               # one memset for every group
            return
        for g in self.groups:
            if g["sync"] is not None and (g["sync"]._handles or any(g["sync"]._launched)):
                # the previous backward did not reach step() (it raised, or the caller skipped the step): its
                # all-reduces may still be reading the gradient buffer this call is about to zero
                g["sync"].abort()
            g["flat"].zero_grad()
            # The bf16 mirror is rewritten by the AdamW kernel and validated per parameter at every use
            # (functional._LPMirror), so eager steps need no refresh here.  A captured step cannot run that host-side
            # check at replay time: GraphedStep.__call__ runs it before every replay (refresh_mirrors) -- round 3
            # recorded a full re-cast of every group in the graph instead (52 us of a 2.5-ms cfg3 step).

    def refresh_mirrors(self) -> None:
        """Re-cast the bf16 mirror of any group whose parameters were edited outside the optimizer since the mirror
        was last written (load_state_dict, nn.init, p.copy_, invalidate_weight_cache)."""
        for g in self.groups:
            if g["mirror"] is not None:
                g["mirror"].refresh_if_stale()

    def step(self):
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.step() inside ema_weights(): the parameters hold the average")
        self.steps += 1
        ema_kw = [{} for _ in self.groups]                 # (no average: exactly the launches without one)
        if self.ema_decay is not None:
            d = ema_decay_at(self.ema_decay, self.ema_updates, self.ema_warmup)
            self.ema_updates += 1
            ema_kw = [{"ema": g["ema"], "ema_decay": d} for g in self.groups]
        if self.fuse_groups:
            return self._step_fused(ema_kw[0].get("ema_decay", 0.0))
        if self._guard:
            for g in self.groups:                      # the norm is that of the COMPLETE all-reduced gradient
                if g["sync"] is not None:
                    g["sync"].finish(average=False)
            K.grad_norm([g["flat"].flat_g for g in self.groups], scale=1.0 / self.world,
                        max_norm=self.max_grad_norm or 0.0, out=self._norm_out, skipped=self._skipped, ws=self._norm_ws)
            coef = self._norm_out[1:2]
            for g, kw in zip(self.groups, ema_kw):
                f = g["flat"]
                K.adamw(f.flat_p, f.flat_g, g["m"], g["v"], g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                        g["weight_decay"], self.steps, grad_scale=1.0 / self.world, p_lp=g["lp"], coef=coef,
                        skip_nonfinite=self.skip_nonfinite, **kw)
            # (a skipped launch left parameters and mirrors as they were: still a matching pair)
            F.bump_weight_epoch([g["mirror"] for g in self.groups if g["mirror"] is not None])
            return
        for g, kw in zip(self.groups, ema_kw):
            if g["sync"] is not None:
                g["sync"].finish(average=False)
            f = g["flat"]
            K.adamw(f.flat_p, f.flat_g, g["m"], g["v"], g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                    g["weight_decay"], self.steps, grad_scale=1.0 / self.world, p_lp=g["lp"], **kw)
        # the AdamW kernel rewrote the bf16 mirrors itself: they stay valid across the epoch bump
        F.bump_weight_epoch([g["mirror"] for g in self.groups if g["mirror"] is not None])

    def _step_fused(self, ema_decay):
        """step() over the arena: one all-reduce stream, one norm over one buffer (no limit on the number of groups),
        one favit_adamw_multi launch per K.ADAMW_MAX_SEGMENTS groups with the groups' CURRENT lr / weight_decay."""
        g0 = self.groups[0]
        if any(tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"] for g in self.groups):
            raise ValueError("FusedAdamW: fuse_groups shares betas and eps among all groups (one launch)")
        if g0["sync"] is not None:
            g0["sync"].finish(average=False)
        coef = None
        if self._guard:
            K.grad_norm([self._arena["g"]], scale=1.0 / self.world, max_norm=self.max_grad_norm or 0.0,
                        out=self._norm_out, skipped=self._skipped, ws=self._norm_ws)
            coef = self._norm_out[1:2]
        for i, j, ends, a in self._launches:
            K.adamw_multi(a["p"], a["g"], a["m"], a["v"], ends, [g["lr"] for g in self.groups[i:j]],
                          [g["weight_decay"] for g in self.groups[i:j]], g0["betas"][0], g0["betas"][1], g0["eps"],
                          self.steps, grad_scale=1.0 / self.world, p_lp=a["lp"], coef=coef,
                          skip_nonfinite=self.skip_nonfinite, ema=a["ema"], ema_decay=ema_decay)
        F.bump_weight_epoch([g0["mirror"]] if g0["mirror"] is not None else [])

    # ---- averaged weights ----
    def _swap_ema(self):
        if self.fuse_groups:
            K.swap_params(self._arena["p"], self._arena["ema"], self._arena["lp"])     # one exchange for every group
        else:
            for g in self.groups:
                K.swap_params(g["flat"].flat_p, g["ema"], g["lp"])
        # as after step(): the parameters changed through raw pointers, the mirrors were rewritten with them
        F.bump_weight_epoch([g["mirror"] for g in self.groups if g["mirror"] is not None])

    @contextlib.contextmanager
    def ema_weights(self):
        """``with opt.ema_weights(): evaluate(model)``: inside, the trainable parameters (and their bf16 mirrors) hold
        the average and `g["ema"]` holds the training weights; one favit_swap_params launch per group (one in all with
        fuse_groups) on entry and on exit (also when the body raises), no address changes -- a captured GraphedStep stays valid.  Frozen
        parameters are untouched.  Nesting and step() inside the context raise RuntimeError."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW.ema_weights(): the optimizer keeps no average (ema_decay=None)")
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.ema_weights() does not nest")
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._ema_swapped = False

    def ema_state_dict(self, model: torch.nn.Module) -> Dict[str, torch.Tensor]:
        """model.state_dict() with the average in place of every trainable parameter (copies; current values for
        frozen parameters and buffers): loadable by model.load_state_dict and by the reference's modules."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW.ema_state_dict(): the optimizer keeps no average (ema_decay=None)")
        slots = _named_slots(self, model)
        out = {}
        for k, t in model.state_dict().items():
            if k in slots:
                gi, o, p_ = slots[k]
                g = self.groups[gi]
                src = g["flat"].flat_p if self._ema_swapped else g["ema"]
                out[k] = src[o:o + p_.numel()].view(p_.shape).clone()
            else:
                out[k] = t.detach().clone()
        return out

    # ---- checkpoint state ----
    def state_dict(self, model: torch.nn.Module) -> Dict:
        """Plain containers and CPU tensors only.  `model` supplies the names (its state_dict keys)."""
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.state_dict() inside ema_weights(): the buffers are exchanged")
        slots = _named_slots(self, model)
        state = {}
        for k, (gi, o, p_) in slots.items():
            g = self.groups[gi]
            cut = lambda t: t[o:o + p_.numel()].view(p_.shape).detach().cpu().clone()
            state[k] = {"m": cut(g["m"]), "v": cut(g["v"])}
            if self.ema_decay is not None:
                state[k]["ema"] = cut(g["ema"])
        groups = [{"lr": float(g["lr"]), "betas": [float(b) for b in g["betas"]], "eps": float(g["eps"]),
                   "weight_decay": float(g["weight_decay"]), "names": [k for k, s_ in slots.items() if s_[0] == gi]}
                  for gi, g in enumerate(self.groups)]
        return {"steps": int(self.steps), "ema_updates": int(self.ema_updates),
                "skipped_steps": None if self.skipped_steps is None else int(self.skipped_steps),
                "max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite,
                "ema_decay": self.ema_decay, "ema_warmup": self.ema_warmup, "groups": groups, "state": state}

    def check_state_dict(self, state: Dict, model: torch.nn.Module):
        """Everything load_state_dict needs to hold, checked without writing: group membership, shapes, and that
        the file has an average if this optimizer keeps one.  ValueError names the offending key."""
        if self._ema_swapped:
            raise RuntimeError("FusedAdamW.load_state_dict() inside ema_weights(): the buffers are exchanged")
        slots = _named_slots(self, model)
        for k in ("steps", "ema_updates", "groups", "state"):
            if k not in state:
                raise ValueError(f"optimizer state: entry '{k}' is missing")
        if len(state["groups"]) != len(self.groups):
            raise ValueError(f"optimizer state: 'groups' has {len(state['groups'])} groups, the optimizer {len(self.groups)}")
        where = {k: gi for gi, g in enumerate(state["groups"]) for k in g["names"]}
        for k, (gi, o, p_) in slots.items():
            if k not in where:
                raise ValueError(f"optimizer state: parameter '{k}' is missing")
            if where[k] != gi:
                raise ValueError(f"optimizer state: parameter '{k}' is in group {where[k]} of the file and in group {gi} "
                                 f"of the optimizer")
            st = state["state"].get(k)
            if st is None:
                raise ValueError(f"optimizer state: no state for parameter '{k}'")
            for key in ("m", "v") + (("ema",) if self.ema_decay is not None else ()):
                if key not in st:
                    raise ValueError(f"optimizer state: parameter '{k}' has no '{key}'"
                                     + (" (the optimizer keeps an average, the file does not)" if key == "ema" else ""))
                if tuple(st[key].shape) != tuple(p_.shape):
                    raise ValueError(f"optimizer state: '{key}' of parameter '{k}' has shape {tuple(st[key].shape)}, the "
                                     f"parameter {tuple(p_.shape)}")
        for k in where:
            if k not in slots:
                raise ValueError(f"optimizer state: parameter '{k}' is not held by the optimizer")
        return slots

    def load_state_dict(self, state: Dict, model: torch.nn.Module) -> None:
        """Restores m, v, the average (copied into their flat slices by offset), the counters and the groups' lr, betas,
        eps and weight_decay.  max_grad_norm, skip_nonfinite, ema_decay and ema_warmup stay as constructed (they decide
        which buffers exist); a file with an average loaded into an optimizer without one drops it."""
        slots = self.check_state_dict(state, model)
        with torch.no_grad():
            for k, (gi, o, p_) in slots.items():
                g, st = self.groups[gi], state["state"][k]
                for key in ("m", "v") + (("ema",) if self.ema_decay is not None else ()):
                    g[key][o:o + p_.numel()].copy_(st[key].reshape(-1))
            if self.skipped_steps is not None:
                self._skipped.fill_(int(state.get("skipped_steps") or 0))
        for g, sg in zip(self.groups, state["groups"]):
            g["lr"], g["betas"] = float(sg["lr"]), (float(sg["betas"][0]), float(sg["betas"][1]))
            g["eps"], g["weight_decay"] = float(sg["eps"]), float(sg["weight_decay"])
        self.steps, self.ema_updates = int(state["steps"]), int(state["ema_updates"])


class WarmupCosine:
    """Learning-rate schedule on the host: linear warm-up, then half a cosine down to min_ratio.

    factor(t), for the optimizer step with index t = 0, 1, ...:
        t <  warmup_steps:  (t + 1) / warmup_steps                       (reaches 1 on the last warm-up step)
        t >= warmup_steps:  min_ratio + (1 - min_ratio) * (1 + cos(pi * x)) / 2,
                            x = min(1, (t - warmup_steps) / max(1, total_steps - warmup_steps))
    Every group's lr is its value at construction times factor(t), so the ratios between groups (param_groups:
    latent_proj at 5x, the head's own rate) are preserved.  The constructor sets the rates of step 0; call step()
    after every optimizer step.  The learning rate is a by-value argument of the eager AdamW launch, so no kernel is
    involved and a GraphedStep picks the new value up at its next call."""

    def __init__(self, opt, warmup_steps: int, total_steps: int, min_ratio: float = 0.0):
        if warmup_steps < 0 or total_steps <= 0 or warmup_steps > total_steps:
            raise ValueError(f"WarmupCosine: need 0 <= warmup_steps <= total_steps and total_steps > 0, got "
                             f"{warmup_steps}, {total_steps}")
        if not 0.0 <= min_ratio <= 1.0:
            raise ValueError(f"WarmupCosine: min_ratio must be in [0, 1], got {min_ratio}")
        self.opt, self.warmup_steps, self.total_steps, self.min_ratio = opt, int(warmup_steps), int(total_steps), float(min_ratio)
        self._groups = opt.groups if hasattr(opt, "groups") else opt.param_groups
        self.base_lrs = [g["lr"] for g in self._groups]
        self.t = 0
        self._apply()

    def factor(self, t: int) -> float:
        import math
        if t < self.warmup_steps:
            return (t + 1) / self.warmup_steps
        x = min(1.0, (t - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps))
        return self.min_ratio + (1.0 - self.min_ratio) * 0.5 * (1.0 + math.cos(math.pi * x))

    def _apply(self):
        f = self.factor(self.t)
        for g, base in zip(self._groups, self.base_lrs):
            g["lr"] = base * f

    def step(self):
        self.t += 1
        self._apply()

    @property
    def last_lr(self):
        return [g["lr"] for g in self._groups]

    def state_dict(self) -> Dict:
        return {"t": int(self.t), "base_lrs": [float(b) for b in self.base_lrs], "warmup_steps": self.warmup_steps,
                "total_steps": self.total_steps, "min_ratio": self.min_ratio}

    def check_state_dict(self, state: Dict) -> None:
        for k in ("t", "base_lrs", "warmup_steps", "total_steps", "min_ratio"):
            if k not in state:
                raise ValueError(f"schedule state: entry '{k}' is missing")
        if len(state["base_lrs"]) != len(self._groups):
            raise ValueError(f"schedule state: 'base_lrs' has {len(state['base_lrs'])} entries, the optimizer "
                             f"{len(self._groups)} groups")

    def load_state_dict(self, state: Dict) -> None:
        """Restores the position and the base rates and re-applies the rates of step t to the optimizer's groups."""
        self.check_state_dict(state)
        self.t, self.base_lrs = int(state["t"]), [float(b) for b in state["base_lrs"]]
        self.warmup_steps, self.total_steps = int(state["warmup_steps"]), int(state["total_steps"])
        self.min_ratio = float(state["min_ratio"])
        self._apply()


class Health:
    """The library's health word (include/favit.h: favit_set_health_word): four device counters in which the
    cross-entropy and AdamW kernels note the FIRST non-finite loss row / gradient / updated parameter they meet, at no
    cost in a clean run.  `poll()` is a host sync; call it every N steps, or once after a timed region.  With
    `opt`, `report()` also walks the optimizer's flat buffers and names the first non-finite tensor."""

    def __init__(self, device=None):
        from . import _abi
        self.words = torch.zeros(4, dtype=torch.int32, device=device if device is not None else torch.cuda.current_device())
        _abi.check(_abi.lib().favit_set_health_word(self.words.data_ptr()), "favit_set_health_word")

    def close(self):
        from . import _abi
        _abi.check(_abi.lib().favit_set_health_word(None), "favit_set_health_word")

    def poll(self):
        """None while everything was finite, else a dict (kinds, first AdamW launch index, launches so far)."""
        f, first_loss, first_grad, launches = (int(v) & 0xFFFFFFFF for v in self.words.tolist())
        if f == 0:
            return None
        kinds = [k for b, k in ((1, "loss"), (2, "gradient"), (4, "parameter")) if f & b]
        return {"non_finite": kinds, "adamw_launch_of_first_bad_loss": first_loss or None,
                "adamw_launch_of_first_bad_gradient_or_parameter": first_grad or None, "adamw_launches": launches}

    def report(self, opt: "FusedAdamW" = None, model: torch.nn.Module = None, extra=()):
        """poll() plus, per optimizer group, the first non-finite entry of flat_p / flat_g / m / v mapped back to a
        parameter name (and of any (name, tensor) in `extra`)."""
        out = self.poll() or {}
        names = {}
        if model is not None:
            names = {id(p): n for n, p in model.named_parameters()}
        found = []
        for gi, g in enumerate(opt.groups if opt is not None else ()):
            flat = g["flat"]
            for key, t in (("flat_g", flat.flat_g), ("flat_p", flat.flat_p), ("m", g["m"]), ("v", g["v"])):
                bad = (~torch.isfinite(t)).nonzero()
                if bad.numel():
                    idx = int(bad[0])
                    who = "?"
                    for p_, o in zip(flat.params, flat.offsets):
                        if o <= idx < o + p_.numel():
                            who = names.get(id(p_), f"param@{o}")
                            break
                    found.append({"group": gi, "buffer": key, "count": int(bad.shape[0]), "first_index": idx, "parameter": who})
        for n, t in extra:
            if t is not None and torch.is_tensor(t) and t.is_floating_point() and not bool(torch.isfinite(t).all()):
                found.append({"tensor": n, "count": int((~torch.isfinite(t)).sum())})
        if found:
            out["tensors"] = found
        return out or None


CHECKPOINT_FORMAT, CHECKPOINT_VERSION = "favit-train-state", 1


def save_checkpoint(path: str, model: torch.nn.Module, opt: Optional[FusedAdamW] = None, schedule=None, loaders=(),
                    extra=None) -> None:
    """Everything a run needs to continue, in one torch.save of plain containers (dict / list / str / int / float /
    None) and CPU tensors -- no pickled class, so ``torch.load(path, map_location="cpu", weights_only=True)`` reads it.
    Written to ``path + ".tmp"`` and moved into place with os.replace: an interrupted save leaves the previous file.

        format "favit-train-state", version 1
        compute_mode   functional.get_compute_mode() at the save
        model          model.state_dict(), fp32; the reference's keys, loadable by either side's modules
        optimizer      FusedAdamW.state_dict(model): m / v / ema per parameter NAME, group hyper-parameters, counters
        schedule       WarmupCosine.state_dict()
        loaders        [x.state_dict() for x in loaders]  (data.DeviceLoader, data.DeviceTransform, datasets.batches(...))
        rng            {"torch_cpu": torch.get_rng_state(), "dropout_epoch": the registered epoch word's value or None}
        extra          the caller's (harness.fit: completed epochs and the history)

    Not saved: the fp8 delayed-scaling histories (functional._FP8_HIST).  After a resume in fp8 mode every site
    measures afresh, as on a run's first step.  Reading the skip counter and the dropout epoch is a host sync.
    Under data parallelism every rank holds the same state (parameters, moments and the average are bitwise equal
    across ranks), and only rank 0 writes; the other ranks return at once."""
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_rank() != 0:
        return
    word = F.get_dropout_epoch()
    obj = {
        "format": CHECKPOINT_FORMAT, "version": CHECKPOINT_VERSION, "compute_mode": F.get_compute_mode(),
        "model": {k: (v.detach().to("cpu", torch.float32) if v.is_floating_point() else v.detach().cpu()).clone()
                  for k, v in model.state_dict().items()},
        "optimizer": None if opt is None else opt.state_dict(model),
        "schedule": None if schedule is None else schedule.state_dict(),
        "loaders": [x.state_dict() for x in loaders],
        "rng": {"torch_cpu": torch.get_rng_state().clone(), "dropout_epoch": None if word is None else int(word.item())},
        "extra": extra,
    }
    tmp = path + ".tmp"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load_checkpoint(path: str, model: torch.nn.Module, opt: Optional[FusedAdamW] = None, schedule=None, loaders=(),
                    use_ema: bool = False):
    """Restore what save_checkpoint wrote into existing objects; returns the file's `extra`.

    Everything is validated before anything is written: format and version, the model's keys and shapes, the
    optimizer's group membership and shapes (and that the file holds an average if `opt` keeps one), the schedule
    and the loader states.  A mismatch raises ValueError naming the key and leaves model and optimizer untouched.
    Then: model.load_state_dict (an in-place copy into the flat-buffer views; the bf16 mirrors see the version
    counters), m / v / ema into their flat slices, the torch CPU generator (the source of the dropout seeds), and the
    dropout epoch word -- written IN PLACE when one is registered (a captured GraphedStep holds its address),
    registered when the file has one and the process none.
    use_ema=True (with opt=None): the averaged weights go into the model, for evaluation or export.
    A compute mode other than the file's is a warning.  The fp8 delayed-scaling histories are not part of the file:
    after a resume in fp8 mode every site measures afresh."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or ck.get("format") != CHECKPOINT_FORMAT:
        raise ValueError(f"{path}: 'format' is {ck.get('format') if isinstance(ck, dict) else type(ck).__name__!r}, "
                         f"expected {CHECKPOINT_FORMAT!r}")
    if ck.get("version") != CHECKPOINT_VERSION:
        raise ValueError(f"{path}: 'version' {ck.get('version')!r} is not supported (this code reads version "
                         f"{CHECKPOINT_VERSION})")
    weights = dict(ck["model"])
    if use_ema:
        if opt is not None:
            raise ValueError("load_checkpoint: use_ema loads the average INTO the model and takes no optimizer (with one, "
                             "load normally and use opt.ema_weights())")
        ost = ck.get("optimizer")
        if ost is None or ost.get("ema_decay") is None:
            raise ValueError(f"{path}: 'optimizer' holds no average (use_ema=True)")
        for k, st in ost["state"].items():
            if "ema" not in st:
                raise ValueError(f"{path}: parameter '{k}' has no 'ema' (use_ema=True)")
            weights[k] = st["ema"]
    own = model.state_dict()
    for k in own:
        if k not in weights:
            raise ValueError(f"{path}: model key '{k}' is missing from the file")
    for k, v in weights.items():
        if k not in own:
            raise ValueError(f"{path}: the file's model key '{k}' does not exist in the model")
        if tuple(v.shape) != tuple(own[k].shape):
            raise ValueError(f"{path}: model key '{k}' has shape {tuple(v.shape)} in the file, {tuple(own[k].shape)} in "
                             f"the model")
    if opt is not None:
        if ck.get("optimizer") is None:
            raise ValueError(f"{path}: 'optimizer' is missing from the file")
        opt.check_state_dict(ck["optimizer"], model)
    if schedule is not None:
        if ck.get("schedule") is None:
            raise ValueError(f"{path}: 'schedule' is missing from the file")
        schedule.check_state_dict(ck["schedule"])
    loaders = list(loaders)
    if loaders and len(ck.get("loaders") or []) != len(loaders):
        raise ValueError(f"{path}: 'loaders' has {len(ck.get('loaders') or [])} entries, {len(loaders)} objects were given")
    for x, st in zip(loaders, ck.get("loaders") or []):
        if hasattr(x, "check_state_dict"):
            x.check_state_dict(st)
    if ck.get("compute_mode") != F.get_compute_mode():
        warnings.warn(f"{path} was written in compute mode {ck.get('compute_mode')!r}, the process runs "
                      f"{F.get_compute_mode()!r}")
    # ---- nothing was written above this line ----
    model.load_state_dict(weights)
    if opt is not None:
        opt.load_state_dict(ck["optimizer"], model)
    if schedule is not None:
        schedule.load_state_dict(ck["schedule"])
    for x, st in zip(loaders, ck.get("loaders") or []):
        x.load_state_dict(st)
    rng = ck.get("rng") or {}
    if rng.get("torch_cpu") is not None:
        torch.set_rng_state(rng["torch_cpu"])
    if rng.get("dropout_epoch") is not None:
        word = F.get_dropout_epoch()
        dev = next(model.parameters()).device
        if word is not None:
            word.fill_(int(rng["dropout_epoch"]))
        elif dev.type == "cuda":
            F.set_dropout_epoch(torch.full((1,), int(rng["dropout_epoch"]), dtype=torch.int64, device=dev))
    return ck.get("extra")


def _check_teacher(teacher, distill):
    if (teacher is None) != (distill is None):
        raise ValueError("a teacher and a Distill go together: got " +
                         ("a teacher without distill=" if distill is None else "distill= without a teacher"))
    if distill is not None and not isinstance(distill, Distill):
        raise TypeError(f"distill must be a train.Distill, got {type(distill).__name__}")


def train_step(model, images, labels, opt: FusedAdamW, label_smoothing: float = 0.0, mix_lam=None, teacher=None,
               distill: Optional[Distill] = None):
    """One step of the reference's hot loop; returns the (device) loss tensor, no host sync.
    mix_lam: the target weights of a batch mixed by data.BatchMix (cross_entropy).
    teacher, distill: a frozen model whose logits on the same (mixed) images enter the loss as `distill` says
    (teacher_logits, cross_entropy); without them the step of before."""
    _check_teacher(teacher, distill)
    opt.zero_grad()
    t_logits = teacher_logits(teacher, images, opt) if teacher is not None else None
    logits = model(images)
    loss = cross_entropy(logits, labels, label_smoothing, mix_lam, t_logits, distill)
    loss.backward()
    opt.step()
    return loss


class GraphedStep:
    """One training step -- zero_grad -> forward -> cross-entropy -> backward -- captured ONCE in HIP graphs and
    replayed per step; the gradient all-reduce and the fused AdamW run eagerly.

    For the small-token configurations (SPPP+MHLA: 17 tokens per image) a step is ~600 kernel launches of a few
    microseconds each and the Python launch path, not the GPU, sets the step time; replayed graphs remove that.

    * Dropout (the reference trains with 0.1, main.py:106): seeds are kernel ARGUMENTS and are frozen into the graph,
      so a device "epoch" word is registered (functional.set_dropout_epoch) that every dropout-drawing kernel mixes
      into its seed when it EXECUTES; the first captured node increments it, i.e. every replay draws fresh masks and the
      forward and backward kernels of one replay agree.  An eager step with the same by-value seeds and the same epoch
      value draws exactly the masks of the replay (tests/test_gpu_modules.py).
    * Data parallelism: with ``segments`` > 1 the backward is captured as that many graphs (the block stack is split
      into consecutive autograd nodes, models/vit.py::run_encoder); after launching segment s the host reports the
      parameters whose gradients segment s completed to dp.GradSync, which puts every finished bucket on the wire
      while segment s + 1 replays.  ``segments = 1`` (default without a process group) defers every bucket to step().

    Requirements: FusedAdamW (its bf16 weight mirror is refreshed by kernels, not by host-side caching), fixed shapes,
    and for SPPP models ``model.assume_num_tokens`` set (the per-forward token-count check is a host sync).
    Fixed shapes include the image size: a step is ONE resolution per capture.  At a resolution other than the model's
    own the captured graphs hold the two pos_embed resampling launches (functional.PrologueOp); their tables are
    uploaded by the eager warm-up steps.  Progressive resizing builds one GraphedStep per size.

    * Mixed batches (data.BatchMix): the target weights change every step, so they cannot be a by-value argument.  With
      ``mix=True`` the step owns a static fp32 [B] buffer that the captured loss kernel (favit_cross_entropy_mix) reads
      when it executes; every call copies its ``mix_lam`` into it, and a call without one fills it with ones, which
      gives the loss and the gradient of the unmixed step bit for bit.
    * Distillation (``teacher=``, ``distill=``): the frozen teacher's forward (eval mode, no tape) is captured in graph 0
      between zero_grad and the student's forward, and its logits live in the graphs' pool.  ``distill.alpha``, ``tau``
      and the kind are by-value kernel arguments frozen into the graph, like ``label_smoothing``: another Distill needs
      another GraphedStep.  The teacher's compute-dtype weight copies are made during warm-up and kept alive with the
      step; the teacher is frozen, so they stay valid (after editing its weights, build a new step).  Combines with
      ``mix=True``.  ``self.kd`` is the mean teacher term of the last replay (a device scalar).  Under data parallelism
      every rank runs its own replica of the teacher, which takes no part in GradSync; like the rest of the RCCL path
      this is untested beyond one rank."""

    def __init__(self, model: torch.nn.Module, opt: FusedAdamW, images: torch.Tensor, labels: torch.Tensor,
                 warmup: int = 3, segments: Optional[int] = None, static_inputs: bool = False,
                 label_smoothing: float = 0.0, mix: bool = False, teacher: Optional[torch.nn.Module] = None,
                 distill: Optional[Distill] = None):
        """static_inputs: `images` / `labels` themselves are the buffers the captured kernels read (no clone at capture,
        no copy per call when the step is called with these same tensors): for a producer that writes every batch into
        fixed device buffers (bench.py's resident synthetic batch).  Default: private copies, one device-to-device copy
        of the batch per call."""
        if K.GEMM_TRACE is not None:
            raise RuntimeError("GraphedStep: disable kernels.GEMM_TRACE (event records cannot be captured)")
        _check_teacher(teacher, distill)
        self.model, self.opt = model, opt
        self.label_smoothing = float(label_smoothing)          # (a by-value kernel argument: frozen into the graph)
        self.teacher, self.distill = teacher, distill          # (alpha, tau, kind: by value as well)
        self.kd = None
        if teacher is not None:
            _check_teacher_frozen(teacher, opt)
        self.x, self.y = (images, labels) if static_inputs else (images.clone(), labels.clone())
        self.lam = torch.ones(labels.shape[0], dtype=torch.float32, device=labels.device) if mix else None
        syncs = [g["sync"] for g in opt.groups if g["sync"] is not None and g["sync"]._active]
        self._syncs = syncs
        if segments is None:
            segments = 3 if syncs else 1
        self.segments = max(1, int(segments))
        for s in syncs:
            s.defer = True                     # nothing goes out while capturing / replaying: launches are explicit
        # (stochastic depth draws with the same generator: a block's plain float attribute drop_path)
        uses_dropout = model.training and any((isinstance(m, torch.nn.Dropout) and m.p > 0) or
                                              float(getattr(m, "drop_path", 0.0) or 0.0) > 0 for m in model.modules())
        self.epoch = None
        if uses_dropout:
            self.epoch = F.get_dropout_epoch()
            if self.epoch is None:
                self.epoch = torch.zeros(1, dtype=torch.int64, device=images.device)
                F.set_dropout_epoch(self.epoch)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # warm-up off the capture stream (lazy kernel attributes, allocator)
            for _ in range(max(1, warmup)):
                self._forward_backward(None)
        torch.cuda.current_stream().wait_stream(side)
        # capture: graph 0 = epoch bump + zero_grad + forward + loss; graphs 1..S = the backward pieces, output side
        # first.  One memory pool: activations saved by graph 0 are read by the backward graphs.
        prev_hook = F._STATE["grad_ready"]
        self._ready: List[List[torch.nn.Parameter]] = []
        self.graphs: List[torch.cuda.CUDAGraph] = []
        try:
            # (one graph and no process group: nobody consumes the notifications, and a registered hook makes the
            # encoder backward flush its batched parameter-gradient launches every four blocks instead of once)
            F.set_grad_ready_hook((lambda p: self._ready[-1].append(p)) if (syncs or self.segments > 1) else None)
            self._forward_backward(self.graphs)
        finally:
            F.set_grad_ready_hook(prev_hook)
        # which parameters are complete after which backward graph: the directly written ones reported themselves;
        # the others (gradients handed to autograd: cls_token, pos_embed, ...) are counted with the last piece
        seen = {id(p) for lst in self._ready for p in lst}
        self._ready[-1].extend(p for g_ in opt.groups for p in g_["flat"].params if id(p) not in seen)
        # Everything allocated OUTSIDE the graphs' pool whose address the captured kernels hold stays alive with the step:
        # the optimizer's flat buffers and bf16 mirrors (self.opt), the dropout epoch and the inputs (self.epoch / x / y),
        # the split-K slab workspace (kernels.py keeps outgrown ones) -- and the installed label maps (their content is
        # changed with SuperpixelSegmentation.update_label_maps; data.DeviceLoader does so once a step is captured).
        self._keep = [K._GROUPED_WS.get(self.x.device.index)]
        if teacher is not None:        # and the teacher with the compute-dtype copies of its weights (functional.wcast)
            self._keep += [teacher] + [getattr(p, "_favit_cast", None) for p in teacher.parameters()]
        self._map_states = []          # label maps + the tensors derived from them (models/sppp.py::_MapState)
        for mod in model.modules():
            seg = getattr(mod, "segmentation", None)
            if seg is not None and getattr(seg, "_state", None) is not None:
                seg._captured = True
                self._map_states.append(seg._state)

    def _forward_backward(self, graphs):
        """zero_grad + forward + loss, then backward piece by piece; with a list, every piece is captured in a graph of
        its own (appended to it), without one it simply runs (warm-up)."""
        import contextlib

        def scope():
            if graphs is None:
                return contextlib.nullcontext()
            g = torch.cuda.CUDAGraph()
            pool = graphs[0].pool() if graphs else None
            graphs.append(g)
            return torch.cuda.graph(g, pool=pool) if pool is not None else torch.cuda.graph(g)

        with scope():
            if self.epoch is not None:
                self.epoch.add_(1)
            self.opt.zero_grad()
            t_logits = teacher_logits(self.teacher, self.x) if self.teacher is not None else None
            with F.encoder_segments(self.segments) as seg:
                if self.distill is None:
                    loss = cross_entropy(self.model(self.x), self.y, self.label_smoothing, self.lam)
                else:
                    loss, kd = cross_entropy_distill(self.model(self.x), self.y, t_logits, self.distill,
                                                     self.label_smoothing, self.lam)
            bounds = list(seg.boundaries)
        if graphs is not None:
            self.loss = loss
            if self.distill is not None:
                self.kd = kd
        heads, grads = [loss], [None]
        for k in range(len(bounds), -1, -1):               # the piece that starts at leaf k-1 (k = 0: the input side)
            if graphs is not None:
                self._ready.append([])
            with scope():
                torch.autograd.backward(heads, grads)
            if k > 0:
                out, leaf = bounds[k - 1]
                heads, grads = [out], [leaf.grad]

    def __call__(self, images: torch.Tensor, labels: torch.Tensor,
                 mix_lam: Optional[torch.Tensor] = None) -> torch.Tensor:
        if images is not self.x:
            self.x.copy_(images, non_blocking=True)
        if labels is not self.y:
            self.y.copy_(labels, non_blocking=True)
        if self.lam is not None:
            if mix_lam is None:
                self.lam.fill_(1.0)
            else:
                self.lam.copy_(mix_lam, non_blocking=True)
        elif mix_lam is not None:
            raise ValueError("GraphedStep: mix_lam needs a step captured with mix=True")
        self.opt.refresh_mirrors()         # (host-side version check; a cast only after an outside edit of the weights)
        for st in self._map_states:        # (likewise: label maps edited in place without update_label_maps)
            st.refresh_if_stale()
        self.graphs[0].replay()
        for g, ready in zip(self.graphs[1:], self._ready):
            g.replay()
            if self._syncs and self.segments > 1:
                for s in self._syncs:
                    s.defer = False
                    for p in ready:
                        s.grad_ready(p)            # buckets completed by this segment go out under the next one
                    s.defer = True
        self.opt.step()            # eager: launches whatever is still deferred, waits, then AdamW
        return self.loss
