"""Evaluation metrics without a GPU: the float64 reference of tests/_eval_ref.py against torch's own top-k and argmax
and against hand-written tie rows, where ignored and non-finite rows go, the two loss means, the argument checks of
harness.EvalMetrics, the runner's flags and the header's declarations."""
import ctypes
import importlib.util
import math
import os

import pytest
import torch

import _eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tie_free(B, Cn, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cn, generator=g, dtype=torch.float64) * 8
    # a condition on the input, not something to tolerate: no two entries of a row are equal
    assert all(len(set(r.tolist())) == Cn for r in x), "the seed gives a tie: pick another"
    return x, torch.randint(0, Cn, (B,), generator=g)


@pytest.mark.parametrize("B,Cn", [(1, 1), (5, 10), (7, 65), (6, 1000)])
def test_reference_agrees_with_torch_topk_and_argmax_on_tie_free_rows(B, Cn):
    x, y = _tie_free(B, Cn, 100 * B + Cn)
    loss, pred, rank, kind = R.rows(x, y)
    assert kind == ["ok"] * B
    assert pred == x.argmax(1).tolist()
    for k in (1, 2, 5, 2000):
        top = x.topk(min(k, Cn), dim=1).indices
        member = (top == y[:, None]).any(1).tolist()
        assert [r < k for r in rank] == member, k
    want = torch.nn.functional.cross_entropy(x, y, reduction="none")
    assert max(abs(a - b) for a, b in zip(loss, want.tolist())) < 1e-12
    assert [r == 0 for r in rank] == [p == t for p, t in zip(pred, y.tolist())]


def test_reference_gives_the_specified_ranks_on_tie_rows():
    for row, label, rank, pred in R.TIE_ROWS:
        _, p, r, kind = R.rows(torch.tensor([row]), torch.tensor([label]))
        assert (p, r, kind) == ([pred], [rank], ["ok"]), (row, label)
    # the rank counts the strictly greater entries and the equal ones with a lower index, nothing else
    for row, label, rank, _ in R.TIE_ROWS:
        xy = row[label]
        assert rank == sum(v > xy for v in row) + sum(v == xy for v in row[:label])


def test_ignored_and_nonfinite_rows_go_where_the_specification_says():
    inf, nan = math.inf, math.nan
    x = torch.tensor([[0.5, 1.5, -0.5],          # fine, label 1: a hit
                      [0.5, 1.5, -0.5],          # ignored: label -1
                      [0.5, 1.5, -0.5],          # ignored: label C
                      [0.5, 1.5, -0.5],          # ignored: label 2**40
                      [nan, 1.5, -0.5],          # NaN at a non-label class
                      [0.5, inf, -0.5],          # +inf at the label
                      [0.5, -inf, -0.5],         # -inf at the label
                      [-inf, -inf, -inf],        # all -inf
                      [-inf, 1.0, -inf]],        # -inf at two non-label classes: legitimate
                     dtype=torch.float64)
    y = torch.tensor([1, -1, 3, 2 ** 40, 1, 1, 1, 1, 1])
    ref = R.Reference(3, (1, 2))
    loss, pred, rank, kind = ref.update(x, y)
    assert kind == ["ok"] + ["ignored"] * 3 + ["nonfinite"] * 4 + ["ok"]
    assert pred == [1, -1, -1, -1, -1, -1, -1, -1, 1] and rank == [0, -1, -1, -1, -1, -1, -1, -1, 0]
    assert all(math.isnan(loss[b]) for b in (1, 2, 3, 4, 5, 7)) and loss[6] == inf
    assert abs(loss[8]) < 1e-15 and math.isfinite(loss[0])
    assert (ref.rows, ref.ignored, ref.nonfinite, ref.batches) == (6, 3, 4, 1)
    assert ref.hits == [2, 2] and math.isnan(ref.loss_sum) and math.isnan(ref.batch_mean_sum)
    assert ref.class_total.tolist() == [0, 6, 0] and ref.class_correct.tolist() == [0, 2, 0]
    assert int(ref.confusion.sum()) == 2 and int(ref.confusion[1, 1]) == 2
    # a launch of ignored rows only is no batch
    before = (ref.batches, ref.rows)
    ref.update(x[1:4], y[1:4])
    assert (ref.batches, ref.rows) == before and ref.ignored == 6
    empty = R.Reference(3, (1,)).compute()
    assert math.isnan(empty["loss"]) and math.isnan(empty["loss_batch_mean"]) and math.isnan(empty["top1"])


def test_batch_mean_equals_the_sample_mean_only_for_equal_batches():
    x, y = _tie_free(8, 10, 5)
    rows = torch.tensor(R.rows(x, y)[0], dtype=torch.float64)
    equal, unequal = R.Reference(10, (1,)), R.Reference(10, (1,))
    for lo, hi in ((0, 4), (4, 8)):
        equal.update(x[lo:hi], y[lo:hi])
    for lo, hi in ((0, 6), (6, 8)):
        unequal.update(x[lo:hi], y[lo:hi])
    e, u = equal.compute(), unequal.compute()
    sample = rows.mean().item()
    assert abs(e["loss"] - sample) < 1e-12 and abs(u["loss"] - sample) < 1e-12
    assert abs(e["loss_batch_mean"] - sample) < 1e-12
    want = 0.5 * (rows[:6].mean().item() + rows[6:].mean().item())
    assert abs(u["loss_batch_mean"] - want) < 1e-12
    assert abs(u["loss_batch_mean"] - sample) > 1e-3, "the case must tell the two definitions apart"


def test_eval_metrics_validates_on_construction(favit):
    E = favit.harness.EvalMetrics
    m = E(10)
    assert (m.num_classes, m.topk, m.per_class, m.confusion) == (10, (1, 5), False, False)
    assert E(3, topk=(1, 2, 5, 2000)).topk == (1, 2, 5, 2000), "a k above the class count is allowed"
    for bad in (dict(num_classes=0), dict(num_classes=-3), dict(num_classes=2.5), dict(num_classes=10, topk=(0,)),
                dict(num_classes=10, topk=(1, -2)), dict(num_classes=10, topk=(1, 2.0)),
                dict(num_classes=10, topk=(1, 2, 3, 4, 5)), dict(num_classes=10, topk=(1, 5, 5))):
        with pytest.raises(ValueError):
            E(**bad)
    # nothing was allocated: reset and compute work on the empty state, without a division error
    m = E(4, topk=(1, 3), per_class=True, confusion=True)
    m.reset()
    out = m.compute()
    assert list(out) == ["loss", "loss_batch_mean", "top1", "top3", "n", "ignored", "nonfinite", "per_class_acc",
                         "confusion"]
    assert math.isnan(out["loss"]) and math.isnan(out["loss_batch_mean"]) and math.isnan(out["top1"])
    assert (out["n"], out["ignored"], out["nonfinite"]) == (0, 0, 0)
    assert len(out["per_class_acc"]) == 4 and all(math.isnan(v) for v in out["per_class_acc"])
    assert out["confusion"].shape == (4, 4) and out["confusion"].dtype == torch.int64
    assert m.loss_rows is None and m.state_words() is None
    assert "per_class_acc" not in E(4).compute() and "confusion" not in E(4).compute()
    H = favit.harness
    with pytest.raises(ValueError):
        H.evaluate(torch.nn.Linear(2, 2), [], graph=True)            # a graph needs metrics
    with pytest.raises(ValueError):
        H.evaluate(torch.nn.Linear(2, 2), [], metrics=E(4, topk=(5,)))   # test_acc is top-1
    with pytest.raises(TypeError):
        H.evaluate(torch.nn.Linear(2, 2), [], metrics=object())
    with pytest.raises(ValueError):
        H.fit(torch.nn.Linear(2, 2), [], None, None, 0, eval_graph=True)


def _runner():
    spec = importlib.util.spec_from_file_location("favit_run_experiment_eval",
                                                  os.path.join(ROOT, "tools", "run_experiment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_runner_flags_default_to_off(capsys):
    tool = _runner()
    a = tool.parse_args(["--experiment", "mhla"])
    assert a.eval_topk is None and a.eval_per_class is False and a.eval_confusion is None and a.eval_graph is False
    a = tool.parse_args(["--experiment", "mhla", "--eval_topk", "1", "5", "--eval_per_class", "--eval_confusion",
                         "cm.npy", "--eval_graph"])
    assert (a.eval_topk, a.eval_per_class, a.eval_confusion, a.eval_graph) == ([1, 5], True, "cm.npy", True)
    assert tool.parse_args(["--experiment", "mhla", "--eval_topk", "5"]).eval_topk == [1, 5], "top-1 is always kept"
    assert tool.parse_args(["--experiment", "mhla", "--eval_topk", "1", "2000"]).eval_topk == [1, 2000]
    for bad in (["--eval_topk", "0"], ["--eval_topk", "1", "2", "3", "4", "5"], ["--eval_topk"]):
        with pytest.raises(SystemExit):
            tool.parse_args(["--experiment", "mhla"] + bad)
    capsys.readouterr()


def test_header_declares_the_entry_point_and_dense_state_slots(favit):
    A = favit._abi
    with open(A.HEADER_PATH) as fh:
        consts, _, sigs = A.parse_header(fh.read())
    assert "favit_eval_metrics" in A.declared_symbols()
    args, res = sigs["favit_eval_metrics"]
    P, I = ctypes.c_void_p, ctypes.c_int32
    assert args == [P, ctypes.c_int64] + [P] * 8 + [I] * 7 + [P] and res is ctypes.c_int
    assert consts["FAVIT_EVAL_MAX_TOPK"] == 4 == A.EVAL_MAX_TOPK
    slots = sorted((v, k) for k, v in consts.items() if k.startswith("FAVIT_EVAL_SLOT_"))
    assert [v for v, _ in slots] == list(range(len(slots))), "the state slot enumerators are dense from 0"
    assert [k[len("FAVIT_EVAL_SLOT_"):].lower() for _, k in slots] == list(A.EVAL_SLOTS) == [
        "loss_sum", "batch_mean_sum", "rows", "batches", "ignored", "nonfinite", "hits"]
    # hits is the last slot and FAVIT_EVAL_MAX_TOPK words long
    assert consts["FAVIT_EVAL_STATE_WORDS"] == consts["FAVIT_EVAL_SLOT_HITS"] + consts["FAVIT_EVAL_MAX_TOPK"]
    K = favit.kernels
    assert (K.EVAL_MAX_TOPK, K.EVAL_STATE_WORDS, K.EVAL_SLOTS["hits"]) == (4, 10, 6)
