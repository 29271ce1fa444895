"""Float64 CPU reference of the evaluation metrics, written from their specification (include/favit.h,
favit_eval_metrics), not from the kernel:

    loss[b] = logsumexp(x_b) - x_b[y_b]
    pred[b] = argmax x_b, the lowest index on ties
    rank[b] = the position of y_b in a STABLE descending sort of x_b (equal entries keep their index order)
    a label outside [0, C): the row is ignored -- loss NaN, pred = rank = -1, only `ignored` counts it
    a valid label and a NaN or +inf anywhere in the row, or -inf at the label (which covers the all -inf row): the row is
    non-finite -- pred = rank = -1; it counts in rows, nonfinite and class_total, adds its loss (NaN, or +inf when only
    the label's logit is -inf) to the sums, hits no k and enters neither class_correct nor the confusion matrix

Every case is decided explicitly here; the kernel decides them all by "the loss is not finite"."""
import math

import torch


def lowest_argmax(x):
    """argmax over dim 1 with the lowest index on ties, spelled out (torch.argmax does not promise an order)."""
    Cn = x.shape[1]
    idx = torch.arange(Cn, dtype=torch.int64).expand_as(x)
    return torch.where(x == x.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, Cn)).min(dim=1).values


def rows(logits, labels):
    """Per row, as Python lists: loss (float), pred, rank (int), kind ("ok" | "ignored" | "nonfinite")."""
    x = logits.detach().double().cpu()
    y = labels.detach().cpu().tolist()
    B, Cn = x.shape
    loss, pred, rank, kind = [], [], [], []
    for b in range(B):
        r = x[b]
        if not 0 <= y[b] < Cn:
            loss.append(math.nan), pred.append(-1), rank.append(-1), kind.append("ignored")
            continue
        bad = bool(torch.isnan(r).any()) or bool((r == math.inf).any())
        if bad or r[y[b]].item() == -math.inf:
            loss.append(math.nan if bad or bool((r == -math.inf).all()) else math.inf)
            pred.append(-1), rank.append(-1), kind.append("nonfinite")
            continue
        loss.append((torch.logsumexp(r, 0) - r[y[b]]).item())
        pred.append(int(lowest_argmax(r[None])[0]))
        order = torch.sort(r, descending=True, stable=True).indices.tolist()
        rank.append(order.index(y[b]))
        kind.append("ok")
    return loss, pred, rank, kind


class Reference:
    """The accumulated state; update() adds a batch as one launch does."""

    def __init__(self, num_classes, topk):
        self.C, self.topk = num_classes, tuple(topk)
        self.loss_sum = self.batch_mean_sum = 0.0
        self.rows = self.batches = self.ignored = self.nonfinite = 0
        self.hits = [0] * len(self.topk)
        self.class_total = torch.zeros(num_classes, dtype=torch.int64)
        self.class_correct = torch.zeros(num_classes, dtype=torch.int64)
        self.confusion = torch.zeros(num_classes, num_classes, dtype=torch.int64)

    def update(self, logits, labels):
        loss, pred, rank, kind = rows(logits, labels)
        y = labels.detach().cpu().tolist()
        s, n = 0.0, 0
        for b, k in enumerate(kind):
            if k == "ignored":
                self.ignored += 1
                continue
            n += 1
            s += loss[b]
            self.class_total[y[b]] += 1
            if k == "nonfinite":
                self.nonfinite += 1
                continue
            for i, kk in enumerate(self.topk):
                self.hits[i] += rank[b] < kk
            self.class_correct[y[b]] += pred[b] == y[b]
            self.confusion[y[b], pred[b]] += 1
        if n:
            self.loss_sum += s
            self.batch_mean_sum += s / n
            self.rows += n
            self.batches += 1
        return loss, pred, rank, kind

    def compute(self):
        nan = math.nan
        out = {"loss": self.loss_sum / self.rows if self.rows else nan,
               "loss_batch_mean": self.batch_mean_sum / self.batches if self.batches else nan}
        for i, k in enumerate(self.topk):
            out[f"top{k}"] = 100.0 * self.hits[i] / self.rows if self.rows else nan
        out.update(n=self.rows, ignored=self.ignored, nonfinite=self.nonfinite)
        out["per_class_acc"] = [100.0 * c / t if t else nan
                                for c, t in zip(self.class_correct.tolist(), self.class_total.tolist())]
        out["confusion"] = self.confusion.clone()
        return out


# Hand-written tie rows: (row, label, rank, pred).  The label tied with a lower index sorts behind it, tied with a higher
# index in front of it; with all entries equal the rank is the label itself.
TIE_ROWS = [
    ([1.0, 3.0, 3.0, 0.0], 2, 1, 1),        # label tied with a lower index
    ([1.0, 3.0, 3.0, 0.0], 1, 0, 1),        # label tied with a higher index
    ([2.0, 2.0, 2.0, 2.0], 3, 3, 0),        # all equal
    ([2.0, 2.0, 2.0, 2.0], 0, 0, 0),
    ([5.0, 1.0, 1.0, 1.0], 2, 2, 0),        # one greater, one equal in front
]
