"""Measurement / experiment harness: counterparts of the reference's
``utils/metrics.py:152-308`` (measure_inference_time / measure_training_time / measure_memory_usage) and of the
epoch loop + results CSV of ``experiments/mhla_pretrained.py:330-525``.

Differences that matter on a GPU: the reference reads ``time.time()`` around asynchronous launches without ever
synchronising (utils/metrics.py:179-183), so its numbers are launch times; here every timed region is bracketed by
HIP events on the compute stream and one synchronisation.  The epoch loop accumulates loss / accuracy ON THE
DEVICE (the reference calls ``loss.item()`` and ``.sum().item()`` per batch: two host syncs per step)."""
from __future__ import annotations

import csv
import os
import time
from typing import Callable, Dict, Iterable, List, Optional

import torch

from . import functional as F
from . import kernels as K
from . import train as T
from .data import MixedLabels


def _sync_time(fn: Callable[[], None], iters: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def measure_inference_time(model, input_tensor, num_iterations: int = 100, warm_up: int = 250) -> Dict[str, float]:
    """utils/metrics.py:152-193 (same keys), timed with device events."""
    dev = next(model.parameters()).device
    x = input_tensor.to(dev)
    with torch.no_grad():
        for _ in range(warm_up):
            model(x)
        total = _sync_time(lambda: model(x), num_iterations)
    return {"total_time": total, "avg_time": total / num_iterations, "fps": num_iterations / total}


def measure_training_time(model, input_tensor, target, criterion, optimizer, num_iterations: int = 10) -> Dict[str, float]:
    """utils/metrics.py:196-240 (same keys).  optimizer: torch.optim.* or train.FusedAdamW."""
    dev = next(model.parameters()).device
    x, y = input_tensor.to(dev), target.to(dev)

    def step():
        optimizer.zero_grad()
        loss = criterion(model(x), y)
        loss.backward()
        optimizer.step()
    total = _sync_time(step, num_iterations)
    return {"total_time": total, "avg_time": total / num_iterations, "iterations_per_second": num_iterations / total}


def measure_memory_usage(model, input_tensor, backward: bool = False) -> Dict[str, float]:
    """utils/metrics.py:243-308 (same keys; psutil for the host side)."""
    import psutil
    dev = next(model.parameters()).device
    x = input_tensor.to(dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    proc = psutil.Process(os.getpid())
    cpu0, gpu0 = proc.memory_info().rss, torch.cuda.memory_allocated()
    if backward:
        model(x).sum().backward()
    else:
        with torch.no_grad():
            model(x)
    torch.cuda.synchronize()
    cpu1, gpu1, peak = proc.memory_info().rss, torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
    mb = 1024 * 1024
    return {"cpu_memory_before_bytes": cpu0, "cpu_memory_after_bytes": cpu1, "cpu_memory_used_bytes": cpu1 - cpu0,
            "cpu_memory_used_mb": (cpu1 - cpu0) / mb, "gpu_memory_before_bytes": gpu0, "gpu_memory_after_bytes": gpu1,
            "gpu_memory_used_bytes": gpu1 - gpu0, "gpu_memory_used_mb": (gpu1 - gpu0) / mb,
            "gpu_memory_peak_bytes": peak, "gpu_memory_peak_mb": peak / mb}


class EvalMetrics:
    """Evaluation statistics kept ON THE DEVICE (favit_eval_metrics): per-sample and per-batch
    loss, top-k accuracy for up to kernels.EVAL_MAX_TOPK values of k, and on request per-class accuracy and the
    confusion matrix.  ``update`` is two launches and no sync (it can be captured in a HIP graph: GraphedEval);
    ``compute`` is the one host read.  The state is allocated at the first ``update``, so construction and its
    argument checks need no GPU.

    A k >= num_classes is allowed and always hits.  A row whose label is outside [0, num_classes) is ignored (only
    ``ignored`` counts it): a batch padded with labels of -1 is evaluated this way.  A row with a valid label and a
    non-finite loss (NaN / +inf logits, -inf at the label) counts in ``n`` and ``nonfinite``, makes both losses
    non-finite, hits no k and enters neither the per-class hits nor the confusion matrix.

    After an ``update``, ``loss_rows`` / ``pred_rows`` / ``rank_rows`` are that batch's per-sample records on the device
    (cross-entropy; argmax, lowest index on ties; the label's place in a stable descending sort, so top-k hits iff
    rank < k; an ignored row reads NaN, -1, -1)."""

    def __init__(self, num_classes: int, topk=(1, 5), per_class: bool = False, confusion: bool = False):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
            raise ValueError(f"EvalMetrics: num_classes must be an integer >= 1, got {num_classes!r}")
        self.topk = K.check_topk(topk)
        if len(set(self.topk)) != len(self.topk):
            raise ValueError(f"EvalMetrics: topk repeats a value: {tuple(topk)}")
        self.num_classes, self.per_class, self.confusion = num_classes, bool(per_class), bool(confusion)
        self._buf = self._loss = self._pred = self._rank = None
        self._last = 0

    def _views(self):
        W, C = K.EVAL_STATE_WORDS, self.num_classes
        o = W + (2 * C if self.per_class else 0)
        return (self._buf[:W], self._buf[W:W + C] if self.per_class else None,
                self._buf[W + C:W + 2 * C] if self.per_class else None, self._buf[o:] if self.confusion else None)

    def _ensure(self, device, B: int) -> None:
        if self._buf is None:
            C = self.num_classes
            words = K.EVAL_STATE_WORDS + (2 * C if self.per_class else 0) + (C * C if self.confusion else 0)
            self._buf = torch.zeros(words, dtype=torch.int64, device=device)       # one allocation: reset is one fill
        if self._loss is None or self._loss.numel() < B:
            self._loss = torch.empty(B, dtype=torch.float32, device=device)
            self._pred = torch.empty(B, dtype=torch.int32, device=device)
            self._rank = torch.empty(B, dtype=torch.int32, device=device)

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        """Add a batch: logits fp32 [B, num_classes] (rows may be strided), labels int64 [B].  No sync."""
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"EvalMetrics.update: logits must be [B, {self.num_classes}], got {tuple(logits.shape)}")
        B = logits.shape[0]
        self._ensure(logits.device, B)
        state, tot, cor, conf = self._views()
        K.eval_metrics(logits, labels, state, self._loss, self._pred, self._rank, self.topk, tot, cor, conf)
        self._last = B

    def reset(self) -> None:
        """Zero the state (one device fill; nothing to do before the first update)."""
        if self._buf is not None:
            self._buf.zero_()

    loss_rows = property(lambda self: None if self._loss is None else self._loss[:self._last])
    pred_rows = property(lambda self: None if self._pred is None else self._pred[:self._last])
    rank_rows = property(lambda self: None if self._rank is None else self._rank[:self._last])

    def state_words(self) -> Optional[torch.Tensor]:
        """A copy of the whole device state as int64 words (the doubles as their bits), or None before any update."""
        return None if self._buf is None else self._buf.clone()

    def compute(self) -> Dict[str, object]:
        """The one host read.  loss: the mean over the samples; loss_batch_mean: the mean of the batches' means (the
        reference's ``val_loss /= len(loader)``; the two differ when batch sizes do); top{k} in percent; n, ignored,
        nonfinite; per_class_acc (a list, NaN for a class no sample had) and confusion ([C, C] int64 on the CPU, row =
        label, column = prediction) when requested.  Without a counted sample the losses and accuracies are NaN."""
        W, C, S = K.EVAL_STATE_WORDS, self.num_classes, K.EVAL_SLOTS
        host = torch.zeros(W, dtype=torch.int64) if self._buf is None else self._buf.cpu()
        ints, dbl = host[:W].tolist(), host[:W].view(torch.float64).tolist()
        n, nb = ints[S["rows"]], ints[S["batches"]]
        nan = float("nan")
        out: Dict[str, object] = {"loss": dbl[S["loss_sum"]] / n if n else nan,
                                  "loss_batch_mean": dbl[S["batch_mean_sum"]] / nb if nb else nan}
        for i, k in enumerate(self.topk):
            out[f"top{k}"] = 100.0 * ints[S["hits"] + i] / n if n else nan
        out.update(n=n, ignored=ints[S["ignored"]], nonfinite=ints[S["nonfinite"]])
        if self.per_class:
            if self._buf is None:
                out["per_class_acc"] = [nan] * C
            else:
                tot, cor = host[W:W + C].tolist(), host[W + C:W + 2 * C].tolist()
                out["per_class_acc"] = [100.0 * c / t if t else nan for c, t in zip(cor, tot)]
        if self.confusion:
            o = W + (2 * C if self.per_class else 0)
            out["confusion"] = torch.zeros(C, C, dtype=torch.int64) if self._buf is None else host[o:].view(C, C).clone()
        return out


class GraphedEval:
    """The evaluation of one batch -- the model's eval forward (``model.eval()``, ``torch.no_grad()``, the ``training``
    flag restored: train.teacher_logits) and ``metrics.update`` -- captured ONCE in a HIP graph over static input
    buffers and replayed per batch.  For the small-token configurations a forward is a chain of short launches whose
    rate the host sets (DESIGN.md sections 6, 7); the replay removes that, as train.GraphedStep does for training.

    * ``__call__(images, labels)`` copies the batch in and replays.  A batch SHORTER than the captured one goes into the
      leading rows and the trailing labels are set to -1: the metrics kernel ignores those rows (they count in
      ``ignored``; their images are those of an earlier batch, finite), so a loader's short last batch needs no second
      graph.  A longer batch is a ValueError: capture from the largest one.
    * Weights.  A replay reads the compute-dtype copies of the weights that existed at capture.  With ``opt=`` (a
      train.FusedAdamW, the bf16 mirrors of which the AdamW kernels keep current) ``opt.refresh_mirrors()`` runs before
      every replay, as in GraphedStep, and ``opt.ema_weights()`` exchanges in place at fixed addresses: the graph
      follows training and evaluates the average inside that context.  Without ``opt`` the weights count as FROZEN: the
      copies made during warm-up are kept alive with this object, and after editing weights a new GraphedEval is needed.
    * SPPP models need ``assume_num_tokens`` and installed label maps, as GraphedStep does, and full batches (the label
      maps have the captured batch size).
    * One resolution per capture: at an image size other than the model's own the graph holds the pos_embed
      resampling launch (functional.PrologueOp), whose table the warm-up runs upload; another size is another object.
    * The metrics' state is left as found by construction (warm-up runs are undone)."""

    def __init__(self, model: torch.nn.Module, images: torch.Tensor, labels: torch.Tensor, metrics: EvalMetrics,
                 opt: Optional["T.FusedAdamW"] = None, warmup: int = 3):
        if K.GEMM_TRACE is not None:
            raise RuntimeError("GraphedEval: disable kernels.GEMM_TRACE (event records cannot be captured)")
        if not isinstance(metrics, EvalMetrics):
            raise TypeError(f"GraphedEval: metrics must be a harness.EvalMetrics, got {type(metrics).__name__}")
        if opt is not None and not isinstance(opt, T.FusedAdamW):
            raise TypeError("GraphedEval: opt must be a train.FusedAdamW (its kernels keep the weight mirrors current)")
        self.model, self.metrics, self.opt = model, metrics, opt
        self.x, self.y = images.clone(), labels.clone()
        self.batch = int(labels.shape[0])
        metrics._ensure(images.device, self.batch)
        found, last = metrics._buf.clone(), metrics._last
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):          # warm-up off the capture stream (lazy kernel attributes, allocator)
            for _ in range(max(1, warmup)):
                self._run()
        cur.wait_stream(side)
        metrics._buf.copy_(found)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._run()
        metrics._last = last
        # What the captured kernels hold the address of, outside the graph's pool, stays alive with this object: the
        # inputs, the metrics' state and row buffers, the split-K workspace, the compute-dtype copies of the weights.
        self._keep = [K._GROUPED_WS.get(self.x.device.index), metrics._buf, metrics._loss, metrics._pred, metrics._rank]
        self._keep += [getattr(p, "_favit_cast", None) for p in model.parameters()]
        self._map_states = []
        for mod in model.modules():
            seg = getattr(mod, "segmentation", None)
            if seg is not None and getattr(seg, "_state", None) is not None:
                seg._captured = True
                self._map_states.append(seg._state)

    def _run(self):
        self.logits = T.teacher_logits(self.model, self.x)
        self.metrics.update(self.logits, self.y)

    def __call__(self, images: torch.Tensor, labels: torch.Tensor) -> None:
        n = int(labels.shape[0])
        if n > self.batch or images.shape[0] != n:
            raise ValueError(f"GraphedEval: captured for batches of {self.batch}, got {images.shape[0]} images and "
                             f"{n} labels (capture from the largest batch)")
        if images is not self.x:
            self.x[:n].copy_(images, non_blocking=True)
        if labels is not self.y:
            self.y[:n].copy_(labels, non_blocking=True)
        if n < self.batch:
            self.y[n:].fill_(-1)
        if self.opt is not None:
            self.opt.refresh_mirrors()     # (host-side version check; a cast only after an outside edit of the weights)
        for st in self._map_states:
            st.refresh_if_stale()
        self.graph.replay()
        self.metrics._last = self.batch


def _evaluate_metrics(model, loader, batch_size, metrics, graph, opt):
    """evaluate() with an EvalMetrics: per batch the forward and metrics.update (or one graph replay) and an event
    pair, nothing else; the pass's single sync is metrics.compute().  graph: False, True (build a GraphedEval from the
    first batch) or a GraphedEval to reuse.  Returns (result, the GraphedEval or None)."""
    if not isinstance(metrics, EvalMetrics):
        raise TypeError(f"evaluate: metrics must be a harness.EvalMetrics, got {type(metrics).__name__}")
    if 1 not in metrics.topk:
        raise ValueError(f"evaluate: metrics.topk must contain 1 (test_acc is top-1), got {metrics.topk}")
    model.eval()
    graphed = graph if isinstance(graph, GraphedEval) else None
    events, total = [], 0
    with torch.no_grad():
        for images, labels in loader:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if graph:
                if graphed is None:
                    graphed = GraphedEval(model, images, labels, metrics, opt=opt)
                e0.record()
                graphed(images, labels)        # (the timed region holds the metrics' two launches as well)
                e1.record()
            else:
                e0.record()
                out = model(images)
                e1.record()
                metrics.update(out, labels)
            events.append((e0, e1))
            total += labels.numel()
    res = metrics.compute()                    # the pass's one host sync; every event above has completed after it
    infer_s = sum(e0.elapsed_time(e1) for e0, e1 in events) * 1e-3
    n_batches = max(1, len(events))
    bs = batch_size or max(1, total // n_batches)
    out = {"test_loss": res["loss_batch_mean"], "test_acc": res["top1"], "avg_inference_time": infer_s / n_batches,
           "avg_inference_time_per_image": infer_s / n_batches / bs, "test_loss_per_sample": res["loss"]}
    for k in metrics.topk:
        out[f"test_top{k}"] = res[f"top{k}"]
    if metrics.per_class:
        out["test_per_class_acc"] = res["per_class_acc"]
    if metrics.confusion:
        out["test_confusion"] = res["confusion"]
    return out, graphed


def evaluate(model, loader: Iterable, batch_size: Optional[int] = None, metrics: Optional[EvalMetrics] = None,
             graph: bool = False, opt=None) -> Dict[str, float]:
    """experiments/mhla_pretrained.py:436-484: test loss / accuracy / inference time per image.
    metrics (an EvalMetrics; default None: the pass and the keys of before): the statistics are kept on the device by
    favit_eval_metrics and the pass syncs ONCE, at its end, instead of once per batch.  The result has the four keys
    of before -- test_loss is the mean of the batches' mean losses, as before, test_acc is top-1 -- and
    test_loss_per_sample, test_top{k} for every k of the metrics, test_per_class_acc and test_confusion when the
    metrics keep them.  The pass ADDS to the metrics: reset() them first unless the sum over several passes is wanted.
    graph (needs metrics): the forward and the metrics' launches of a batch are one HIP-graph replay (GraphedEval,
    built from the pass's first batch, which must be its largest; a short last batch is padded with ignored rows).
    opt: the train.FusedAdamW training the model, for graph=True (see GraphedEval); without it the weights count as frozen."""
    if metrics is not None:
        return _evaluate_metrics(model, loader, batch_size, metrics, bool(graph), opt)[0]
    if graph:
        raise ValueError("evaluate: graph=True needs metrics= (an EvalMetrics)")
    model.eval()
    dev = next(model.parameters()).device
    loss_sum = torch.zeros((), device=dev)
    correct = torch.zeros((), device=dev, dtype=torch.int64)
    total = n_batches = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    infer_s = 0.0
    with torch.no_grad():
        for images, labels in loader:
            e0.record()
            out = model(images)
            e1.record()
            loss_sum += T.cross_entropy(out, labels)
            correct += (out.argmax(1) == labels).sum()
            total += labels.numel()
            n_batches += 1
            e1.synchronize()
            infer_s += e0.elapsed_time(e1) * 1e-3
    n_batches = max(1, n_batches)
    bs = batch_size or max(1, total // n_batches)
    return {"test_loss": loss_sum.item() / n_batches, "test_acc": 100.0 * correct.item() / max(1, total),
            "avg_inference_time": infer_s / n_batches, "avg_inference_time_per_image": infer_s / n_batches / bs}


def _cls_row_per_key(rec, probs) -> torch.Tensor:
    """[B, L]: row 0 of a head-mean map, the slots of a banded map summed per key."""
    if rec.kind == "dense":
        return probs[:, 0, :].clone()
    idx = F.window_indices(rec.L, rec.W)[0].to(probs.device)
    return torch.zeros((rec.B, rec.L), dtype=torch.float32, device=probs.device).index_add_(1, idx, probs[:, 0, :])


def attention_maps(model, images: torch.Tensor, per_head: bool = False, residual: float = 0.5) -> Dict[str, object]:
    """Where the CLS row of `model` looks for `images`: one eval-mode forward under torch.no_grad() and
    functional.capture_attention (the unpruned Python chains, with the probability kernel on every block's stored
    qkv), then attention rollout of row 0 through all blocks in one launch (K.attn_rollout).  The model's `training`
    flag is restored.  Returns
      logits         the forward's output
      rollout        fp32 [B, L]: r = e_0, and from the last block to the first r <- residual r + (1 - residual) r P_k
                     with P_k the block's head-mean map
      cls_attention  fp32 [B, L]: the last block's CLS row, head mean, slots summed per key
      layers         the blocks' maps in order: head-mean [B, L, W] (MHLA; slot w of row i is key
                     functional.window_indices(L, W)[i, w]) or [B, L, L] (dense); with per_head the per-head maps
                     [B, H, L, W] / [B, H, L, L] (rollout then uses their mean over the heads)
      window         per block its W, 0 for a dense block
      grid           fp32 [B, gh, gw], for models with a patch_embed: rollout[:, 1:] on the patch grid; for a superpixel
                     model every patch gets the value of the token its superpixel became; None for other models.
    A model whose head reads the token mean (set_global_pool('avg')) is refused: these maps follow the CLS row."""
    pool = getattr(getattr(model, "model", model), "global_pool", "token")
    if pool != "token":
        raise ValueError(f"attention_maps: the maps and the rollout describe the CLS row, which the {pool!r}-pooled head "
                         "of this model does not read; set_global_pool('token') gives the CLS head's maps")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), F.capture_attention(per_head=per_head) as cap:
            logits = model(images)
    finally:
        model.train(was_training)
    if not cap.layers:
        raise RuntimeError("attention_maps: the model ran no MHLA or dense attention chain")
    means = [r.probs.mean(dim=1) if per_head else r.probs for r in cap.layers]
    window = [r.W for r in cap.layers]
    rollout = K.attn_rollout(means, window, cls_row=0, residual=residual)
    out = {"logits": logits, "rollout": rollout, "cls_attention": _cls_row_per_key(cap.layers[-1], means[-1]),
           "layers": [r.probs for r in cap.layers], "window": window, "grid": None}
    pe = getattr(model, "patch_embed", None)
    if pe is not None and hasattr(pe, "patch_size") and images.dim() == 4:
        B = images.shape[0]
        gh, gw = images.shape[2] // pe.patch_size, images.shape[3] // pe.patch_size
        if hasattr(model, "patch_mapper"):        # patch p of image b was pooled into token 1 + rank[b, p] (sppp_tokens)
            rank = model.patch_mapper.map_patches_batched(model.segmentation.segment(images).to(images.device))[0]
            out["grid"] = rollout[:, 1:].gather(1, rank.long()).reshape(B, gh, gw)
        elif rollout.shape[1] == gh * gw + 1:
            out["grid"] = rollout[:, 1:].reshape(B, gh, gw).clone()
    return out


def fit(model, train_loader: Iterable, val_loader: Optional[Iterable], optimizer, epochs: int,
        log: Callable[[str], None] = print, label_smoothing: float = 0.0, schedule=None,
        checkpoint: Optional[str] = None, checkpoint_every: int = 1, resume: bool = False,
        eval_ema: bool = False, teacher=None, distill: Optional["T.Distill"] = None,
        eval_metrics: Optional[EvalMetrics] = None, eval_graph: bool = False) -> Dict[str, object]:
    """The reference's epoch loop (experiments/mhla_pretrained.py:350-420) with device-side statistics: one host
    sync per EPOCH.  optimizer: train.FusedAdamW (hot path) or any torch.optim optimizer.
    label_smoothing: the TRAINING loss is nn.CrossEntropyLoss(label_smoothing=...)'s; evaluation keeps the plain one.
    Mixed batches: the train loader may yield (images, data.MixedLabels(labels, lam)) (data.DeviceLoader(mix=...));
    the training loss is then taken against the mixed targets, and train_acc counts a prediction as right when it is
    the row's OWN label (labels[b], not the partner's), so under mixing it reads lower than the accuracy on clean
    images.  Evaluation never mixes.
    schedule: an object with step() (train.WarmupCosine), called after every optimizer step.
    history["grad_norm"] (the epoch mean of the pre-clip global gradient norm, summed on the device) is present
    when the optimizer exposes `grad_norm` (train.FusedAdamW with max_grad_norm or skip_nonfinite).
    checkpoint: a path; train.save_checkpoint after every `checkpoint_every` epochs (and after the last one) with
    extra = {"epoch": completed epochs, "history": ...} and the train loader's state (data.DeviceLoader: the
    transform's generator and the shuffle epoch of datasets.batches).  Needs a train.FusedAdamW.
    resume: with an existing `checkpoint` file, load it and continue from the stored epoch; the history is extended,
    not restarted, and total_training_time covers this process only.  Under data parallelism rank 0 writes.
    eval_ema: the validation pass runs inside optimizer.ema_weights() (train.FusedAdamW with ema_decay).
    teacher, distill: a frozen model and a train.Distill; the training loss is then the distilled one on the teacher's
    logits for the same (mixed) images (train.teacher_logits, train.cross_entropy), and history["train_kd"] is the
    epoch mean of the teacher term, summed on the device (no sync of its own).  Evaluation never uses the teacher.  The
    teacher is not part of the checkpoint -- it is frozen, and the caller rebuilds it before resuming.  Without a
    teacher the loop is the one of before and the history has no such key.
    eval_metrics (an EvalMetrics whose topk contains 1): every validation pass resets them and runs through them
    (evaluate(metrics=...): one host sync per pass); val_loss / val_acc are then their loss_batch_mean / top1, and the
    history gains val_top{k} for every other k -- keys that exist only with metrics, and that checkpoint and resume
    carry like the rest of the history.  After fit they hold the last pass.  eval_graph (needs eval_metrics and a
    train.FusedAdamW): the passes replay ONE GraphedEval, built from the first validation batch with opt=optimizer,
    so it follows the training and, with eval_ema, evaluates the average.  Without eval_metrics: the passes of before."""
    dev = next(model.parameters()).device
    hist: Dict[str, List[float]] = {"train_loss": [], "train_acc": [], "val_loss": [], "val_acc": [], "epoch_time": []}
    track_norm = getattr(optimizer, "grad_norm", None) is not None
    if track_norm:
        hist["grad_norm"] = []
    T._check_teacher(teacher, distill)
    if teacher is not None:
        hist["train_kd"] = []
        T._check_teacher_frozen(teacher, optimizer)
    if checkpoint is not None and not isinstance(optimizer, T.FusedAdamW):
        raise TypeError("fit: checkpoint= needs a train.FusedAdamW (its state is saved by parameter name)")
    if checkpoint is not None and checkpoint_every < 1:
        raise ValueError(f"fit: checkpoint_every must be >= 1, got {checkpoint_every}")
    if eval_ema and getattr(optimizer, "ema_decay", None) is None:
        raise ValueError("fit: eval_ema needs a train.FusedAdamW with ema_decay")
    if eval_metrics is not None:
        if not isinstance(eval_metrics, EvalMetrics) or 1 not in eval_metrics.topk:
            raise ValueError("fit: eval_metrics must be a harness.EvalMetrics whose topk contains 1")
        for k in eval_metrics.topk:
            if k != 1:
                hist[f"val_top{k}"] = []
    if eval_graph and (eval_metrics is None or not isinstance(optimizer, T.FusedAdamW)):
        raise ValueError("fit: eval_graph needs eval_metrics and a train.FusedAdamW")
    graphed = eval_graph                   # True until the first pass has built the GraphedEval, which the others replay

    def validate():
        nonlocal graphed
        if eval_metrics is None:
            return evaluate(model, val_loader)
        eval_metrics.reset()
        ev, built = _evaluate_metrics(model, val_loader, None, eval_metrics, graphed, optimizer if eval_graph else None)
        graphed = built or graphed
        return ev
    stateful = [train_loader] if hasattr(train_loader, "state_dict") else []
    first_ep = 0
    if resume and checkpoint is not None and os.path.exists(checkpoint):
        extra = T.load_checkpoint(checkpoint, model, optimizer, schedule, stateful)
        first_ep, hist = int(extra["epoch"]), {k: list(v) for k, v in extra["history"].items()}
        log(f"Resumed {checkpoint} after epoch {first_ep}")
    t_start = time.perf_counter()
    peak_mb = 0.0
    for ep in range(first_ep, epochs):
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        model.train()
        loss_sum = torch.zeros((), device=dev)
        correct = torch.zeros((), device=dev, dtype=torch.int64)
        total = n_batches = 0
        norm_sum = torch.zeros((), device=dev) if track_norm else None
        kd_sum = torch.zeros((), device=dev) if teacher is not None else None
        for images, labels in train_loader:
            mix_lam = None
            if isinstance(labels, MixedLabels):
                labels, mix_lam = labels
            optimizer.zero_grad()
            if teacher is None:
                out = model(images)
                loss = T.cross_entropy(out, labels, label_smoothing, mix_lam)
            else:
                t_logits = T.teacher_logits(teacher, images)
                out = model(images)
                loss, kd = T.cross_entropy_distill(out, labels, t_logits, distill, label_smoothing, mix_lam)
                kd_sum += kd
            loss.backward()
            optimizer.step()
            if schedule is not None:
                schedule.step()
            if track_norm:
                norm_sum += optimizer.grad_norm
            loss_sum += loss.detach()
            correct += (out.detach().argmax(1) == labels).sum()
            total += labels.numel()
            n_batches += 1
        hist["train_loss"].append(loss_sum.item() / max(1, n_batches))          # the epoch's single sync
        hist["train_acc"].append(100.0 * correct.item() / max(1, total))
        if track_norm:
            hist["grad_norm"].append(norm_sum.item() / max(1, n_batches))
        if teacher is not None:
            hist.setdefault("train_kd", []).append(kd_sum.item() / max(1, n_batches))
        if val_loader is not None:
            if eval_ema:
                with optimizer.ema_weights():
                    ev = validate()
            else:
                ev = validate()
            hist["val_loss"].append(ev["test_loss"])
            hist["val_acc"].append(ev["test_acc"])
            if eval_metrics is not None:
                for k in eval_metrics.topk:
                    if k != 1:
                        hist.setdefault(f"val_top{k}", []).append(ev[f"test_top{k}"])
        torch.cuda.synchronize()
        hist["epoch_time"].append(time.perf_counter() - t0)
        peak_mb = max(peak_mb, torch.cuda.max_memory_allocated() / (1024 * 1024))
        log(f"Epoch {ep + 1}/{epochs} | Train Loss: {hist['train_loss'][-1]:.4f} | Train Acc: {hist['train_acc'][-1]:.2f}% | "
            + (f"Val Loss: {hist['val_loss'][-1]:.4f} | Val Acc: {hist['val_acc'][-1]:.2f}% | " if val_loader is not None else "")
            + f"Time: {hist['epoch_time'][-1]:.2f}s")
        if checkpoint is not None and ((ep + 1) % checkpoint_every == 0 or ep + 1 == epochs):
            T.save_checkpoint(checkpoint, model, optimizer, schedule, stateful, extra={"epoch": ep + 1, "history": hist})
    return {"history": hist, "avg_epoch_time": sum(hist["epoch_time"]) / max(1, len(hist["epoch_time"])),
            "total_training_time": time.perf_counter() - t_start,
            "final_val_acc": hist["val_acc"][-1] if hist["val_acc"] else float("nan"),
            "final_val_loss": hist["val_loss"][-1] if hist["val_loss"] else float("nan"), "peak_gpu_memory_mb": peak_mb}


def save_results_csv(path: str, row: Dict[str, object]) -> None:
    """One-row results CSV like experiments/mhla_pretrained.py:486-525 (pandas-free)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(row.keys()))
        w.writeheader()
        w.writerow(row)
