"""Float64 CPU reference of the distilled loss, written from the formulas of its specification (include/favit.h,
favit_cross_entropy_distill), not from the kernel:

    loss = mean_b((1 - alpha) * base[b] + alpha * kd[b])
    base = -(t * log_softmax(x)).sum(1),  t = (1 - eps) (lam onehot(y) + (1 - lam) onehot(y flipped)) + eps / C
    soft kd = tau^2 * (softmax(z / tau) * (log_softmax(z / tau) - log_softmax(x / tau))).sum(1)
    hard kd = -log_softmax(x)[argmax z], the lowest index on ties

The gradient with respect to x comes from autograd; `closed_form_grad` is the expression the header states."""
import torch


def lowest_argmax(z):
    """argmax over dim 1 with the lowest index on ties, spelled out (torch.argmax does not promise an order)."""
    Cn = z.shape[1]
    idx = torch.arange(Cn, dtype=torch.int64).expand_as(z)
    return torch.where(z == z.max(dim=1, keepdim=True).values, idx, torch.full_like(idx, Cn)).min(dim=1).values


def targets(labels, lam, eps, Cn):
    hot = torch.nn.functional.one_hot(labels.cpu(), Cn).double()
    if lam is None:
        return (1.0 - eps) * hot + eps / Cn
    l = lam.double().cpu()[:, None]
    return (1.0 - eps) * (l * hot + (1.0 - l) * hot.flip(0)) + eps / Cn


def rows(x, z, labels, lam, eps, alpha, tau, kind):
    """(loss_rows, kd_rows) in float64 on the CPU; x may require grad."""
    z = z.detach().double().cpu()
    t = targets(labels, lam, eps, x.shape[1])
    base = -(t * torch.log_softmax(x, dim=1)).sum(1)
    if kind == "soft":
        lq, lp = torch.log_softmax(z / tau, dim=1), torch.log_softmax(x / tau, dim=1)
        kd = tau * tau * (torch.softmax(z / tau, dim=1) * (lq - lp)).sum(1)
    elif kind == "hard":
        kd = -torch.log_softmax(x, dim=1).gather(1, lowest_argmax(z)[:, None])[:, 0]
    else:
        raise ValueError(kind)
    return (1.0 - alpha) * base + alpha * kd, kd


def reference(logits, teacher, labels, lam, eps, alpha, tau, kind):
    """dict(loss, grad, kd, loss_rows, kd_rows): the mean loss, its autograd gradient with respect to the logits, the
    mean teacher term and the rows."""
    x = logits.detach().double().cpu().requires_grad_(True)
    loss_rows, kd_rows = rows(x, teacher, labels, lam, eps, alpha, tau, kind)
    loss = loss_rows.mean()
    loss.backward()
    return {"loss": loss.item(), "grad": x.grad, "kd": kd_rows.mean().item(), "loss_rows": loss_rows.detach(),
            "kd_rows": kd_rows.detach()}


def closed_form_grad(logits, teacher, labels, lam, eps, alpha, tau, kind, grad_scale):
    """dlogits as the header writes it: grad_scale * ((1 - alpha) * (softmax(x) - target) + alpha * d), soft
    d = tau * (p - q), hard d = softmax(x) - onehot(argmax z)."""
    x, z = logits.detach().double().cpu(), teacher.detach().double().cpu()
    sm = torch.softmax(x, dim=1)
    if kind == "soft":
        d = tau * (torch.softmax(x / tau, dim=1) - torch.softmax(z / tau, dim=1))
    else:
        d = sm - torch.nn.functional.one_hot(lowest_argmax(z), x.shape[1]).double()
    return grad_scale * ((1.0 - alpha) * (sm - targets(labels, lam, eps, x.shape[1])) + alpha * d)
