"""Evaluation metrics on the GPU: favit_eval_metrics against the float64 reference of tests/_eval_ref.py (rows, ties,
ignored and non-finite rows, the folding loop, accumulation, determinism, per-class counts, refused arguments), and
the paths built on it: harness.evaluate with metrics, GraphedEval, harness.fit and the runner."""
import csv
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOSS_TOL = 1e-5          # |loss - ref| <= LOSS_TOL * max(1, |ref|): the bound of test_gpu_distill.py / test_gpu_mix.py
TOPK = (1, 2, 5, 2000)


def _tol(ref):
    return LOSS_TOL * max(1.0, abs(ref))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _state(favit, m):
    """The named words of the metrics' device state: ints, and the two sums as doubles."""
    S, W = favit.kernels.EVAL_SLOTS, favit.kernels.EVAL_STATE_WORDS
    w = m.state_words()[:W].cpu()
    ints, dbl = w.tolist(), w.view(torch.float64).tolist()
    out = {k: ints[i] for k, i in S.items() if k not in ("loss_sum", "batch_mean_sum", "hits")}
    out.update(loss_sum=dbl[S["loss_sum"]], batch_mean_sum=dbl[S["batch_mean_sum"]],
               hits=ints[S["hits"]:S["hits"] + len(m.topk)])
    return out


def _case(B, Cn, scale, seed=0):
    g = torch.Generator(device=DEV).manual_seed(1000 * B + Cn + seed)
    x = (torch.rand(B, Cn, device=DEV, generator=g) * 2 - 1) * scale
    return x, torch.randint(0, Cn, (B,), device=DEV, generator=g)


def _check_rows(m, ref_rows, B):
    loss, pred, rank, _ = ref_rows
    got = m.loss_rows.double().cpu().tolist()
    assert m.pred_rows.cpu().tolist() == pred and m.rank_rows.cpu().tolist() == rank
    worst = 0.0
    for b in range(B):
        if math.isfinite(loss[b]):
            assert abs(got[b] - loss[b]) <= _tol(loss[b]), (b, got[b], loss[b])
            worst = max(worst, abs(got[b] - loss[b]) / max(1.0, abs(loss[b])))
        elif math.isnan(loss[b]):
            assert math.isnan(got[b]), (b, got[b])
        else:
            assert got[b] == loss[b], (b, got[b])
    return worst


def _check_state(favit, m, ref):
    st = _state(favit, m)
    assert (st["rows"], st["batches"], st["ignored"], st["nonfinite"]) == \
        (ref.rows, ref.batches, ref.ignored, ref.nonfinite)
    assert st["hits"] == ref.hits
    for got, want in ((st["loss_sum"], ref.loss_sum), (st["batch_mean_sum"], ref.batch_mean_sum)):
        if math.isfinite(want):
            assert abs(got - want) <= _tol(want), (got, want)
        else:
            assert not math.isfinite(got), (got, want)
    return st


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("scale", [8.0, 80.0])
@pytest.mark.parametrize("B,Cn", [(1, 1), (5, 10), (4, 64), (7, 65), (3, 100), (6, 1000)])
def test_rows_match_the_reference(favit, B, Cn, scale, strided):
    x, y = _case(B, Cn, scale)
    top, near = torch.arange(B, device=DEV)[1::3], torch.arange(B, device=DEV)[2::3]
    x[top, y[top]] = scale                       # every third row's label is the maximum (or ties with it),
    x[near, y[near]] = 0.9999 * scale            # another third's sits just below: some k hit, whatever the draw
    if strided:                                  # rows of ld = C + 3 with other values between them
        big = torch.full((B, Cn + 3), 1e30, device=DEV)
        big[:, :Cn] = x
        x = big[:, :Cn]
        assert x.stride(0) == Cn + 3
    m = favit.harness.EvalMetrics(Cn, topk=TOPK)
    ref = R.Reference(Cn, TOPK)
    m.update(x, y)
    worst = _check_rows(m, ref.update(x, y), B)
    st = _check_state(favit, m, ref)
    out, want = m.compute(), ref.compute()
    print(f"B={B} C={Cn} scale={scale} strided={strided}: worst row error {worst:.2e}; loss {out['loss']!r} ref "
          f"{want['loss']!r}; hits {st['hits']}")
    assert abs(out["loss"] - want["loss"]) <= _tol(want["loss"])
    assert abs(out["loss_batch_mean"] - want["loss_batch_mean"]) <= _tol(want["loss_batch_mean"])
    for k in TOPK:
        assert out[f"top{k}"] == want[f"top{k}"]
    assert out["top2000"] == 100.0, "a k >= C always hits"
    assert (out["n"], out["ignored"], out["nonfinite"]) == (B, 0, 0)


def test_ties_rank_by_index(favit):
    rows = torch.tensor([r for r, _, _, _ in R.TIE_ROWS], device=DEV)
    y = torch.tensor([l for _, l, _, _ in R.TIE_ROWS], device=DEV)
    m = favit.harness.EvalMetrics(4, topk=(1, 2, 3))
    m.update(rows, y)
    assert m.rank_rows.cpu().tolist() == [r for _, _, r, _ in R.TIE_ROWS]
    assert m.pred_rows.cpu().tolist() == [p for _, _, _, p in R.TIE_ROWS]
    ref = R.Reference(4, (1, 2, 3))
    ref.update(rows, y)
    _check_state(favit, m, ref)
    # the maximum three times, in another lane and in another loop iteration of the wave: indices 3, 64 and 129
    g = torch.Generator(device=DEV).manual_seed(3)
    row = torch.rand(130, device=DEV, generator=g) * 4 - 2
    row[3] = row[64] = row[129] = 5.0
    x = row.repeat(3, 1)
    y = torch.tensor([3, 64, 129], device=DEV)
    m = favit.harness.EvalMetrics(130, topk=(1, 2, 3))
    m.update(x, y)
    assert m.rank_rows.cpu().tolist() == [0, 1, 2] and m.pred_rows.cpu().tolist() == [3, 3, 3]
    ref = R.Reference(130, (1, 2, 3))
    _check_rows(m, ref.update(x, y), 3)
    assert _check_state(favit, m, ref)["hits"] == [1, 2, 3]


def test_ignored_rows_move_only_their_counter(favit):
    Cn = 7
    x, y = _case(6, Cn, 8.0)
    y[1], y[3], y[4] = -1, Cn, 2 ** 40
    m = favit.harness.EvalMetrics(Cn, topk=(1, 3), per_class=True, confusion=True)
    ref = R.Reference(Cn, (1, 3))
    m.update(x, y)
    _check_rows(m, ref.update(x, y), 6)
    st = _check_state(favit, m, ref)
    assert (st["rows"], st["ignored"], st["batches"]) == (3, 3, 1)
    out = m.compute()
    assert int(out["confusion"].sum()) == 3 and torch.equal(out["confusion"], ref.confusion)
    # a launch of ignored rows only: no batch, the sums keep their bits
    before = m.state_words().cpu()
    m.update(x[:3], torch.tensor([-1, -5, Cn + 1], device=DEV))
    after = m.state_words().cpu()
    S = favit.kernels.EVAL_SLOTS
    moved = [i for i in range(after.numel()) if after[i] != before[i]]
    assert moved == [S["ignored"]] and int(after[S["ignored"]]) == 6
    assert math.isnan(m.loss_rows[0].item()) and m.pred_rows.cpu().tolist() == [-1] * 3 == m.rank_rows.cpu().tolist()
    # ignored rows alone on an empty state: NaN losses, no division error
    e = favit.harness.EvalMetrics(Cn)
    e.update(x[:2], torch.tensor([-1, -1], device=DEV))
    out = e.compute()
    assert math.isnan(out["loss"]) and math.isnan(out["loss_batch_mean"]) and math.isnan(out["top1"])
    assert (out["n"], out["ignored"]) == (0, 2)


def test_nonfinite_rows_count_but_hit_nothing(favit):
    inf, nan = math.inf, math.nan
    x = torch.tensor([[0.5, 1.5, -0.5],          # fine
                      [nan, 1.5, -0.5],          # NaN at a non-label class
                      [0.5, inf, -0.5],          # +inf at the label
                      [0.5, -inf, -0.5],         # -inf at the label
                      [-inf, -inf, -inf],        # all -inf
                      [-inf, 1.0, -inf],         # -inf at two non-label classes: stays finite
                      [2.5, 1.0, -inf]],         # the same with the label ranked second
                     device=DEV)
    y = torch.tensor([1, 1, 1, 1, 1, 1, 1], device=DEV)
    m = favit.harness.EvalMetrics(3, topk=(1, 2), per_class=True, confusion=True)
    ref = R.Reference(3, (1, 2))
    m.update(x, y)
    want = ref.update(x, y)
    assert want[3] == ["ok"] + ["nonfinite"] * 4 + ["ok", "ok"] and want[2] == [0, -1, -1, -1, -1, 0, 1]
    _check_rows(m, want, 7)
    st = _check_state(favit, m, ref)
    assert (st["rows"], st["nonfinite"], st["hits"]) == (7, 4, [2, 3])
    assert math.isnan(st["loss_sum"]), "a NaN row shows in the loss"
    out = m.compute()
    assert torch.equal(out["confusion"], ref.confusion) and int(out["confusion"].sum()) == 3
    assert out["per_class_acc"][1] == 100.0 * 2 / 7 and math.isnan(out["per_class_acc"][0])
    # the finite rows are those of a launch without the bad ones, bit for bit
    keep = [0, 5, 6]
    c = favit.harness.EvalMetrics(3, topk=(1, 2))
    c.update(x[keep].contiguous(), y[keep].contiguous())
    assert torch.equal(_bits(c.loss_rows), _bits(m.loss_rows[keep]))
    # -inf at the label alone: the loss is +inf, not NaN
    assert m.loss_rows[3].item() == inf


def test_folding_loop_accumulation_and_reset(favit):
    Cn = 10
    m = favit.harness.EvalMetrics(Cn, topk=(1, 5), per_class=True)
    ref = R.Reference(Cn, (1, 5))
    means = []
    for i, B in enumerate((5, 1030, 1)):         # 1030 rows: more than four passes of the folding workgroup
        x, y = _case(B, Cn, 8.0, seed=i)
        m.update(x, y)
        rows = ref.update(x, y)
        _check_rows(m, rows, B)
        means.append(sum(rows[0]) / B)
    st = _check_state(favit, m, ref)
    assert (st["rows"], st["batches"]) == (1036, 3)
    out, want = m.compute(), ref.compute()
    assert abs(out["loss_batch_mean"] - sum(means) / 3) <= _tol(sum(means) / 3)
    assert abs(out["loss"] - want["loss"]) <= _tol(want["loss"])
    assert abs(want["loss"] - want["loss_batch_mean"]) > 1e-3, "the case tells the two means apart"
    assert out["top1"] == want["top1"] and out["top5"] == want["top5"]
    assert out["per_class_acc"] == want["per_class_acc"]
    m.reset()
    assert not bool(m.state_words().any()), "reset zeroes every word"
    assert m.compute()["n"] == 0


def test_same_updates_give_the_same_bits(favit):
    Cn = 10
    batches = [_case(B, Cn, 8.0, seed=i) for i, B in enumerate((5, 1030, 1))]
    m = favit.harness.EvalMetrics(Cn, topk=(1, 5), per_class=True, confusion=True)
    runs = []
    for _ in range(2):
        m.reset()
        for x, y in batches:
            m.update(x, y)
        runs.append(m.state_words().cpu())
    assert torch.equal(runs[0], runs[1]), "the double slots included, compared as int64"
    assert int(runs[0][favit.kernels.EVAL_SLOTS["rows"]]) == 1036


def test_per_class_counts_and_confusion_match_the_reference(favit):
    Cn, B = 10, 257
    x, y = _case(B, Cn, 8.0)
    y[y == 7] = 8                                # class 7 never occurs
    x[torch.arange(0, B, 3, device=DEV), y[::3]] += 20.0         # and a third of the rows are surely right
    for per_class, confusion in ((True, False), (True, True), (False, True)):
        m = favit.harness.EvalMetrics(Cn, topk=(1,), per_class=per_class, confusion=confusion)
        ref = R.Reference(Cn, (1,))
        m.update(x, y)
        ref.update(x, y)
        out, want = m.compute(), ref.compute()
        if per_class:
            W = favit.kernels.EVAL_STATE_WORDS
            words = m.state_words().cpu()
            assert torch.equal(words[W:W + Cn], ref.class_total) and torch.equal(words[W + Cn:W + 2 * Cn], ref.class_correct)
            assert math.isnan(out["per_class_acc"][7])
            assert [v for i, v in enumerate(out["per_class_acc"]) if i != 7] == \
                [v for i, v in enumerate(want["per_class_acc"]) if i != 7]
        if confusion:
            assert torch.equal(out["confusion"], ref.confusion) and int(out["confusion"].sum()) == B
            assert int(out["confusion"].diagonal().sum()) == int(ref.class_correct.sum()) > B // 3 - 1
        assert ("per_class_acc" in out, "confusion" in out) == (per_class, confusion)


def test_refused_arguments_launch_nothing(favit):
    lib, INV = favit._abi.lib(), favit._abi.ERR_INVALID
    B, Cn = 5, 10
    x, y = _case(B, Cn, 8.0)
    W = favit.kernels.EVAL_STATE_WORDS
    state = torch.arange(1, W + 1, dtype=torch.int64, device=DEV) * 1000003
    loss = torch.full((B,), -7.0, device=DEV)
    pred = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    rank = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    tot = torch.full((Cn,), 11, dtype=torch.int64, device=DEV)
    before = state.clone()

    def call(x=x, y=y, loss=loss, pred=pred, rank=rank, state=state, b=B, c=Cn, ld=Cn, n=2, ks=(1, 5, 0, 0)):
        return lib.favit_eval_metrics(_P(x), ld, _P(y), _P(loss), _P(pred), _P(rank), _P(state), _P(tot), None, None,
                                      b, c, n, ks[0], ks[1], ks[2], ks[3], _st())
    assert call(x=None) == INV and call(y=None) == INV and call(state=None) == INV
    assert call(loss=None) == INV and call(pred=None) == INV and call(rank=None) == INV
    assert call(c=0) == INV and call(c=-1) == INV and call(b=-1) == INV and call(ld=Cn - 1) == INV
    assert call(n=5) == INV and call(n=-1) == INV
    assert call(ks=(1, 0, 0, 0)) == INV and call(n=4, ks=(1, 2, 3, -4)) == INV
    assert call(b=0) == 0, "an empty batch is fine and changes nothing"
    torch.cuda.synchronize()
    assert torch.equal(state, before) and bool((tot == 11).all())
    assert bool((loss == -7).all()) and bool((pred == -7).all()) and bool((rank == -7).all())
    # the same buffers, accepted: the k beyond n_topk are not read
    state.zero_()
    tot.zero_()
    assert call(n=1, ks=(1, -9, -9, -9)) == 0
    torch.cuda.synchronize()
    S = favit.kernels.EVAL_SLOTS
    assert int(state[S["rows"]]) == B and int(tot.sum()) == B and not bool((pred == -7).any())


# ---- the paths built on the kernel ----
def _tiny(favit, seed=11):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=8, num_classes=10, embed_dim=64, depth=2,
                                                       num_heads=2, use_mhla=True).to(DEV)


def _loader(sizes=(8, 8, 3), seed=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [(torch.randn(b, 3, 32, 32, device=DEV, generator=g), torch.randint(0, 10, (b,), device=DEV, generator=g))
            for b in sizes]


OLD_KEYS = {"test_loss", "test_acc", "avg_inference_time", "avg_inference_time_per_image"}


def test_evaluate_with_metrics_equals_evaluate_without(favit):
    H = favit.harness
    model, loader = _tiny(favit), _loader()
    old = H.evaluate(model, loader)
    assert set(old) == OLD_KEYS, "without metrics: the keys of before"
    m = H.EvalMetrics(10, topk=(1, 5), per_class=True, confusion=True)
    new = H.evaluate(model, loader, metrics=m)
    print(f"old {old['test_loss']!r} / {old['test_acc']!r}; new {new['test_loss']!r} / {new['test_acc']!r}; "
          f"per sample {new['test_loss_per_sample']!r}; top5 {new['test_top5']!r}")
    assert set(new) == OLD_KEYS | {"test_loss_per_sample", "test_top1", "test_top5", "test_per_class_acc",
                                    "test_confusion"}
    assert new["test_acc"] == old["test_acc"] == new["test_top1"], "a ratio of integers"
    assert abs(new["test_loss"] - old["test_loss"]) <= 2 * LOSS_TOL * max(1.0, abs(old["test_loss"]))
    assert new["test_acc"] <= new["test_top5"] <= 100.0 and int(new["test_confusion"].sum()) == 19
    assert new["avg_inference_time"] > 0 and new["avg_inference_time_per_image"] > 0
    out = m.compute()
    assert (out["n"], out["ignored"], out["nonfinite"]) == (19, 0, 0)
    assert new["test_loss"] == out["loss_batch_mean"] and new["test_loss_per_sample"] == out["loss"]
    # the pass ADDS to the metrics: a second one doubles the counts and keeps the means
    again = H.evaluate(model, loader, metrics=m)
    assert m.compute()["n"] == 38 and again["test_acc"] == new["test_acc"]
    assert abs(again["test_loss"] - new["test_loss"]) <= 1e-12 * max(1.0, abs(new["test_loss"]))


def test_graphed_evaluate_equals_eager(favit, monkeypatch):
    H, T = favit.harness, favit.train
    model, loader = _tiny(favit), _loader()
    eager_m = H.EvalMetrics(10, topk=(1, 5))
    H.evaluate(model, loader, metrics=eager_m)
    eager = _state(favit, eager_m)

    class Counting(H.GraphedEval):
        built, rows = 0, []

        def __init__(self, *a, **kw):
            Counting.built += 1
            Counting.made = self
            super().__init__(*a, **kw)

        def __call__(self, images, labels):
            super().__call__(images, labels)
            Counting.rows.append((self.metrics.loss_rows.clone(), self.x.clone(), self.y.clone()))
    monkeypatch.setattr(H, "GraphedEval", Counting)
    graph_m = H.EvalMetrics(10, topk=(1, 5))
    res = H.evaluate(model, loader, metrics=graph_m, graph=True)
    graphed = _state(favit, graph_m)
    print(f"eager {eager}\ngraphed {graphed}")
    assert Counting.built == 1 and len(Counting.rows) == 3, "the short batch needs no second capture"
    assert graphed["ignored"] == 5 and eager["ignored"] == 0
    for k in ("rows", "batches", "nonfinite", "hits"):
        assert graphed[k] == eager[k], k
    assert res["test_top1"] == 100.0 * eager["hits"][0] / 19
    # the short batch went into the leading rows, the rest is padding: labels of -1 and the previous batch's images
    _, x_last, y_last = Counting.rows[2]
    assert y_last.tolist() == loader[2][1].tolist() + [-1] * 5
    assert torch.equal(x_last[:3], loader[2][0]) and torch.equal(x_last[3:], loader[1][0][3:])
    # row losses: bit-identical to the eager launches on the same inputs (for the short batch, the padded one)
    hand = H.EvalMetrics(10, topk=(1, 5))
    for rows, x, y in Counting.rows:
        hand.update(T.teacher_logits(model, x), y)
        assert torch.equal(_bits(hand.loss_rows), _bits(rows))
    assert torch.equal(hand.state_words(), graph_m.state_words()), "and so is the whole state"
    with pytest.raises(ValueError):          # a batch longer than the captured one is refused, before any copy
        Counting.made(torch.cat([loader[0][0], loader[1][0]]), torch.cat([loader[0][1], loader[1][1]]))


def test_graphed_eval_follows_training_and_the_average(favit):
    H, T = favit.harness, favit.train
    favit.set_compute_dtype("bf16")              # the mode that has weight mirrors
    try:
        model = _tiny(favit).train()
        opt = T.FusedAdamW(T.param_groups(model, lr=1e-2, head_lr=1e-2), lr=1e-2, weight_decay=0.05, distributed=False,
                           ema_decay=0.5)
        (x, y), = _loader((8,))
        m = H.EvalMetrics(10, topk=(1, 5))
        ge = H.GraphedEval(model, x, y, m, opt=opt)
        assert model.training and m.compute()["n"] == 0, "warm-up leaves the flag and the metrics as found"

        def fresh():
            f = H.EvalMetrics(10, topk=(1, 5))
            f.update(T.teacher_logits(model, x), y)
            return f.loss_rows.clone()
        ge(x, y)
        first = m.loss_rows.clone()
        assert torch.equal(_bits(first), _bits(fresh()))
        for _ in range(2):
            T.train_step(model, x, y, opt)
        ge(x, y)
        second = m.loss_rows.clone()
        assert torch.equal(_bits(second), _bits(fresh())), "the replay reads the updated weights"
        assert not torch.equal(_bits(second), _bits(first))
        with opt.ema_weights():
            ge(x, y)
            averaged = m.loss_rows.clone()
            assert torch.equal(_bits(averaged), _bits(fresh())), "inside ema_weights(): the average"
        assert not torch.equal(_bits(averaged), _bits(second))
        ge(x, y)
        assert torch.equal(_bits(m.loss_rows), _bits(second)), "and the training weights again after it"
        assert m.compute()["n"] == 32
        print(f"row 0: first {first[0].item()!r} trained {second[0].item()!r} averaged {averaged[0].item()!r}")
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def _opt(T, model, lr):
    return T.FusedAdamW(T.param_groups(model, lr=lr, head_lr=lr), lr=lr, weight_decay=0.05, distributed=False)


def test_fit_with_eval_metrics(favit, tmp_path):
    H, T = favit.harness, favit.train
    quiet = lambda s: None
    train, val = _loader((8, 8), seed=4), _loader()
    path = str(tmp_path / "fit.pt")
    model = _tiny(favit)
    m = H.EvalMetrics(10, topk=(1, 5))
    res = H.fit(model, train, val, _opt(T, model, 1e-3), 1, log=quiet, eval_metrics=m, checkpoint=path)
    h = res["history"]
    out = m.compute()
    assert set(h) == {"train_loss", "train_acc", "val_loss", "val_acc", "epoch_time", "val_top5"}
    assert h["val_acc"] == [out["top1"]] and h["val_top5"] == [out["top5"]] and h["val_loss"] == [out["loss_batch_mean"]]
    assert out["n"] == 19 and h["val_acc"][0] <= h["val_top5"][0] <= 100.0
    # resumed: the history is extended, the new key with it, and every pass starts from reset metrics
    model2 = _tiny(favit, seed=5)
    both = H.fit(model2, train, val, _opt(T, model2, 1e-3), 2, log=quiet, eval_metrics=m, checkpoint=path,
                 resume=True)["history"]
    assert both["val_top5"][:1] == h["val_top5"] and len(both["val_top5"]) == 2 == len(both["val_acc"])
    assert m.compute()["n"] == 19
    # without metrics: the keys and the pass of before
    model3 = _tiny(favit)
    plain = H.fit(model3, train, val, _opt(T, model3, 1e-3), 1, log=quiet)["history"]
    assert set(plain) == {"train_loss", "train_acc", "val_loss", "val_acc", "epoch_time"}
    with pytest.raises(ValueError):
        H.fit(model3, train, val, _opt(T, model3, 1e-3), 1, log=quiet, eval_metrics=H.EvalMetrics(10, topk=(5,)))
    with pytest.raises(ValueError):
        H.fit(model3, train, val, _opt(T, model3, 1e-3), 1, log=quiet, eval_graph=True)


def test_fit_replays_one_graphed_eval(favit, monkeypatch):
    """At a learning rate of zero the weights stay, so the graphed passes must repeat the eager ones exactly."""
    H, T = favit.harness, favit.train
    quiet = lambda s: None
    train, val = _loader((8,), seed=4), _loader()
    model = _tiny(favit)
    eager = H.fit(model, train, val, _opt(T, model, 0.0), 2, log=quiet, eval_metrics=H.EvalMetrics(10))["history"]
    built = []

    class Counting(H.GraphedEval):
        def __init__(self, *a, **kw):
            built.append(1)
            super().__init__(*a, **kw)
    monkeypatch.setattr(H, "GraphedEval", Counting)
    model = _tiny(favit)
    m = H.EvalMetrics(10)
    graphed = H.fit(model, train, val, _opt(T, model, 0.0), 2, log=quiet, eval_metrics=m, eval_graph=True)["history"]
    assert len(built) == 1, "one capture for both passes"
    assert graphed["val_acc"] == eager["val_acc"] and graphed["val_top5"] == eager["val_top5"]
    assert graphed["val_acc"][0] == graphed["val_acc"][1]
    for a, b in zip(graphed["val_loss"], eager["val_loss"]):
        assert abs(a - b) <= 2 * LOSS_TOL * max(1.0, abs(b))
    out = m.compute()
    assert (out["n"], out["ignored"]) == (19, 5)


def test_runner_writes_topk_columns_and_the_confusion_matrix(tmp_path):
    res, cm = tmp_path / "results", tmp_path / "cm" / "confusion.npy"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_experiment.py"), "--experiment", "mhla", "--img_size", "32",
           "--patch_size", "8", "--embed_dim", "64", "--depth", "2", "--num_heads", "2", "--epochs", "1", "--batch_size",
           "64", "--results_dir", str(res), "--eval_topk", "1", "5", "--eval_graph", "--eval_confusion", str(cm)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    with open(res / "exp_mhla.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1 and "test_top5" in rows[0] and "test_top1" in rows[0]
    acc, top5 = float(rows[0]["test_acc"]), float(rows[0]["test_top5"])
    print(f"test_acc {acc} test_top5 {top5} test_loss {rows[0]['test_loss']}")
    assert acc == float(rows[0]["test_top1"]) and acc <= top5 <= 100.0 and np.isfinite(float(rows[0]["test_loss"]))
    mat = np.load(cm)
    assert mat.shape == (10, 10) and mat.dtype == np.int64 and int(mat.sum()) == 512, "the synthetic test split"
    assert 100.0 * np.trace(mat) / mat.sum() == acc
