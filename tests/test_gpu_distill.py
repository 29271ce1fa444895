"""Knowledge distillation on the GPU: favit_cross_entropy_distill against the float64 reference of tests/_distill_ref.py,
its contract (alpha = 0, optional outputs, ties, bad labels, a non-finite teacher, refused arguments), and the teacher in
the eager step, the graphed step and harness.fit."""
import ctypes

import pytest
import torch

import _distill_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

LOSS_TOL = 1e-5          # |loss - ref| < LOSS_TOL * max(1, |ref|): test_cross_entropy_mix's bound, relative (a +-80 row)
GRAD_TOL = 2e-5          # rel-L2 of dlogits, as there


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


def _bits(t):
    return t.contiguous().view(torch.int32)


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _case(B, Cn):
    """Student logits, labels and lam as test_gpu_mix.py::_ce_case builds them (one student row of +-80 alternating),
    and teacher logits with, for B > 1, ANOTHER row of +-80 alternating."""
    g = torch.Generator(device=DEV).manual_seed(1000 * B + Cn)
    logits = torch.randn(B, Cn, device=DEV, generator=g) * 3
    alt = 80.0 * (1 - 2 * (torch.arange(Cn, device=DEV) % 2))
    if B > 1:
        logits[min(5, B - 2)] = alt
    labels = torch.randint(0, Cn, (B,), device=DEV, generator=g)
    if B > 1:
        labels[B - 1] = labels[0]
    lam = torch.tensor([(0.0, 0.3, 1.0, 0.75)[b % 4] for b in range(B)], device=DEV)
    teacher = torch.randn(B, Cn, device=DEV, generator=g) * 3
    if B > 1:
        teacher[(min(5, B - 2) + 1) % B] = alt
    return logits, teacher, labels, lam


# C: the issue's 1 (kd = 0), 2 (one lane busy), 65 (one lane past a full wave), 1000; rows of 129 .. 1024 classes are
# held in registers and the others walked in memory, so both sides of both thresholds: 128 | 129 and 1024 | 1100 (not a
# multiple of 64).  B: a partly filled last workgroup.
@pytest.mark.parametrize("kind,tau", [("soft", 1.0), ("soft", 3.0), ("hard", 1.0)])
@pytest.mark.parametrize("Cn", [1, 2, 65, 128, 129, 1000, 1024, 1100])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_kernel_matches_the_reference(favit, K, B, Cn, kind, tau):
    logits, teacher, labels, lam_pat = _case(B, Cn)
    hard = kind == "hard"
    worst = [0.0, 0.0, 0.0]
    for alpha in (0.5, 1.0):
        for eps in (0.0, 0.1):
            for lam in (None, lam_pat):
                ref = R.reference(logits, teacher, labels, lam, eps, alpha, tau, kind)
                rows, dlog, kd = K.cross_entropy_distill(logits, teacher, labels, grad_scale=1.0 / B, label_smoothing=eps,
                                                         mix_lam=lam, alpha=alpha, tau=tau, hard=hard)
                loss, kdm = rows.double().mean().item(), kd.double().mean().item()
                e_loss = abs(loss - ref["loss"]) / max(1.0, abs(ref["loss"]))
                e_kd = abs(kdm - ref["kd"]) / max(1.0, abs(ref["kd"]))
                e_grad = rel_l2(dlog, ref["grad"])
                print(f"B={B} C={Cn} {kind} tau={tau} alpha={alpha} eps={eps} lam={'mix' if lam is not None else None}: "
                      f"loss {loss!r} ref {ref['loss']!r} ({e_loss:.2e}); kd {kdm!r} ref {ref['kd']!r} ({e_kd:.2e}); "
                      f"dlogits rel-L2 {e_grad:.2e}")
                worst = [max(a, b) for a, b in zip(worst, (e_loss, e_kd, e_grad))]
                assert e_loss < LOSS_TOL and e_kd < LOSS_TOL and e_grad < GRAD_TOL
                # K.cross_entropy(..., teacher=) is the same launch without kd_rows
                rows_b, dlog_b = K.cross_entropy(logits, labels, grad_scale=1.0 / B, label_smoothing=eps, mix_lam=lam,
                                                 teacher=teacher, distill_alpha=alpha, distill_tau=tau, distill_hard=hard)
                assert torch.equal(_bits(rows_b), _bits(rows)) and torch.equal(_bits(dlog_b), _bits(dlog))
    if Cn == 1:
        assert float(kd.abs().max()) == 0.0, "one class: both distributions are the point mass"
    print(f"worst: loss {worst[0]:.2e} kd {worst[1]:.2e} dlogits {worst[2]:.2e}")


@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("B,Cn", [(5, 65), (37, 300)])
def test_autograd_wrapper(favit, B, Cn, kind):
    T = favit.train
    logits, teacher, labels, lam = _case(B, Cn)
    d = T.Distill(0.5, 3.0, kind)
    ref = R.reference(logits, teacher, labels, lam, 0.1, d.alpha, d.tau, kind)
    x = logits.clone().requires_grad_(True)
    z = teacher.clone().requires_grad_(True)              # (a teacher tensor that could take a gradient: it gets none)
    loss = T.cross_entropy(x, labels, 0.1, lam, teacher_logits=z, distill=d)
    loss.backward()
    print(f"loss {loss.item()!r} ref {ref['loss']!r}; grad rel-L2 {rel_l2(x.grad, ref['grad']):.2e}")
    assert abs(loss.item() - ref["loss"]) < LOSS_TOL * max(1.0, abs(ref["loss"]))
    assert rel_l2(x.grad, ref["grad"]) < GRAD_TOL
    assert z.grad is None
    loss2, kd = T.cross_entropy_distill(logits, labels, teacher, d, 0.1, lam)
    assert loss2.item() == loss.item() and not kd.requires_grad
    assert abs(kd.item() - ref["kd"]) < LOSS_TOL * max(1.0, abs(ref["kd"]))
    # distill=None is the call of before, whatever the teacher argument holds
    plain = T.cross_entropy(logits, labels, 0.1, lam)
    assert T.cross_entropy(logits, labels, 0.1, lam, teacher_logits=teacher, distill=None).item() == plain.item()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
def test_alpha_zero_is_the_loss_without_a_teacher(K, eps, mixed):
    B, Cn = 37, 300
    logits, _, labels, lam = _case(B, Cn)
    lam = lam if mixed else None
    nan_teacher = torch.full((B, Cn), float("nan"), device=DEV)
    want_rows, want_dlog = K.cross_entropy(logits, labels, grad_scale=1.0 / B, label_smoothing=eps, mix_lam=lam)
    rows, dlog, kd = K.cross_entropy_distill(logits, nan_teacher, labels, grad_scale=1.0 / B, label_smoothing=eps,
                                             mix_lam=lam, alpha=0.0, tau=2.0)
    assert torch.equal(_bits(rows), _bits(want_rows)) and torch.equal(_bits(dlog), _bits(want_dlog))
    assert bool((kd == 0).all())
    rows, dlog = K.cross_entropy(logits, labels, grad_scale=1.0 / B, label_smoothing=eps, mix_lam=lam,
                                 teacher=nan_teacher, distill_alpha=0.0)
    assert torch.equal(_bits(rows), _bits(want_rows)) and torch.equal(_bits(dlog), _bits(want_dlog))


@pytest.mark.parametrize("hard", [0, 1])
@pytest.mark.parametrize("Cn", [65, 300])
def test_optional_outputs_and_refused_arguments(favit, Cn, hard):
    B = 5
    lib, INV = favit._abi.lib(), favit._abi.ERR_INVALID
    logits, teacher, labels, lam = _case(B, Cn)
    new = lambda *s: torch.full(s, -7.0, device=DEV)

    def call(rows, kd, dlog, alpha=0.5, tau=3.0, eps=0.1, z=teacher, x=logits, y=labels, b=B, c=Cn):
        return lib.favit_cross_entropy_distill(_P(x), _P(z), _P(y), _P(lam), _P(rows), _P(kd), _P(dlog), b, c, 1.0 / B, eps,
                                               alpha, tau, hard, _st())
    rows, kd, dlog = new(B), new(B), new(B, Cn)
    assert call(rows, kd, dlog) == 0
    rows_a, kd_a = new(B), new(B)
    assert call(rows_a, kd_a, None) == 0                     # dlogits = NULL
    assert torch.equal(_bits(rows_a), _bits(rows)) and torch.equal(_bits(kd_a), _bits(kd))
    rows_b, dlog_b = new(B), new(B, Cn)
    assert call(rows_b, None, dlog_b) == 0                   # kd_rows = NULL
    assert torch.equal(_bits(rows_b), _bits(rows)) and torch.equal(_bits(dlog_b), _bits(dlog))
    # refused before any launch: the outputs keep their fill
    r, k, d = new(B), new(B), new(B, Cn)
    assert call(r, k, d, alpha=1.5) == INV and call(r, k, d, alpha=-0.1) == INV and call(r, k, d, alpha=float("nan")) == INV
    assert call(r, k, d, eps=1.0) == INV and call(r, k, d, eps=-0.1) == INV
    assert call(r, k, d, z=None) == INV and call(r, k, d, z=None, alpha=1.0) == INV
    assert call(r, k, d, x=None) == INV and call(r, k, d, y=None) == INV and call(None, k, d) == INV
    assert call(r, k, d, b=0) == INV and call(r, k, d, c=0) == INV
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        assert call(r, k, d, tau=tau) == (0 if hard else INV), tau      # a hard teacher does not use tau
    if not hard:
        torch.cuda.synchronize()
        assert bool((r == -7).all()) and bool((k == -7).all()) and bool((d == -7).all())
    else:
        assert torch.equal(_bits(r), _bits(rows)) and torch.equal(_bits(d), _bits(dlog))


@pytest.mark.parametrize("Cn", [70, 300, 1100])
def test_hard_ties_take_the_lowest_index(K, Cn):
    B = 6
    logits, teacher, labels, _ = _case(B, Cn)
    teacher[0] = 0.25                                        # constant: class 0
    teacher[1] = -1.0
    teacher[1, 3] = teacher[1, 64] = 2.0                     # two maxima, in different lanes and strides: class 3
    teacher[2] = -1.0
    teacher[2, 64] = teacher[2, 65] = teacher[2, Cn - 1] = 2.0          # the lowest index sits in the second stride
    want = torch.tensor([0, 3, 64], device=DEV)
    rows, dlog, kd = K.cross_entropy_distill(logits, teacher, labels, grad_scale=1.0, alpha=1.0, hard=True)
    lsm = torch.log_softmax(logits.double(), 1)
    for b in range(3):
        picked = -lsm[b]                                     # kd if class c had been taken
        assert abs(kd[b].item() - picked[want[b]].item()) < 1e-5 * max(1.0, abs(picked[want[b]].item())), b
        # alpha = 1: dlogits = softmax - onehot(argmax z): the one entry below zero names the class
        neg = (dlog[b] < -0.5).nonzero().flatten().tolist()
        assert neg in ([int(want[b])], []), (b, neg)
        assert int(torch.argmin(dlog[b] - torch.softmax(logits[b], 0))) == int(want[b])
    assert R.lowest_argmax(teacher.double().cpu())[:3].tolist() == want.tolist()


@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("B,Cn", [(5, 65), (37, 300), (6, 1100)])
def test_bad_labels_and_a_non_finite_teacher_stay_in_their_rows(K, B, Cn, kind):
    logits, teacher, labels, lam = _case(B, Cn)
    kw = dict(grad_scale=1.0 / B, label_smoothing=0.1, alpha=0.5, tau=3.0, hard=kind == "hard")
    rows, dlog, kd = K.cross_entropy_distill(logits, teacher, labels, mix_lam=lam, **kw)
    assert bool(torch.isfinite(rows).all())
    for i in sorted({0, B // 2}):                            # as test_cross_entropy_mix: own and partner rows are NaN
        lab2 = labels.clone()
        lab2[i] = -100 if i == 0 else Cn
        rows2, dlog2, kd2 = K.cross_entropy_distill(logits, teacher, lab2, mix_lam=lam, **kw)
        bad = sorted({i, B - 1 - i})
        keep = [b for b in range(B) if b not in bad]
        assert bool(torch.isnan(rows2[bad]).all()), (i, rows2)
        assert torch.equal(_bits(rows2[keep]), _bits(rows[keep])) and torch.equal(_bits(dlog2[keep]), _bits(dlog[keep]))
        assert bool(torch.isfinite(dlog2).all())
        # unmixed, the partner's label is not read: only the own row
        rows3, dlog3, _ = K.cross_entropy_distill(logits, teacher, lab2, **kw)
        assert torch.isnan(rows3).nonzero().flatten().tolist() == [i] and bool(torch.isfinite(dlog3).all())
    for val in (float("nan"), float("inf"), float("-inf")):
        t2 = teacher.clone()
        t2[B // 2, Cn - 1] = val
        rows4, _, kd4 = K.cross_entropy_distill(logits, t2, labels, mix_lam=lam, **kw)
        keep = [b for b in range(B) if b != B // 2]
        assert torch.isnan(rows4).nonzero().flatten().tolist() == [B // 2], (val, rows4)
        assert torch.equal(_bits(rows4[keep]), _bits(rows[keep])) and torch.equal(_bits(kd4[keep]), _bits(kd[keep]))


def test_health_word_flags_a_non_finite_teacher_row(favit, K):
    logits, teacher, labels, lam = _case(5, 65)
    health = favit.train.Health()
    try:
        lab2 = labels.clone()
        lab2[1] = -100                                       # an out-of-range label alone: a NaN row, no flag
        K.cross_entropy_distill(logits, teacher, lab2, alpha=0.5, tau=2.0)
        assert health.poll() is None
        teacher[2, 7] = float("nan")
        K.cross_entropy_distill(logits, teacher, labels, alpha=0.5, tau=2.0)
        got = health.poll()
        assert got is not None and got["non_finite"] == ["loss"], got
    finally:
        health.close()


# ----------------------------------------------------------------------------------------------------------------
def _vit(favit, seed=11):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                       num_heads=4, use_mhla=True).to(DEV).train()


def _teacher(favit, seed=23):
    """A dense ViT of the student's dimensions, seeded differently, frozen -- and left in training mode with dropout
    layers, so that a teacher run outside eval() would show."""
    torch.manual_seed(seed)
    t = favit.models.vit.VisionTransformer(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2, num_heads=4,
                                           dropout=0.1).to(DEV).train()
    for p in t.parameters():
        p.requires_grad = False
    return t


@pytest.fixture(scope="module")
def step_case():
    g = torch.Generator(device=DEV).manual_seed(2)
    xs = [torch.randn(8, 3, 32, 32, device=DEV, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device=DEV, generator=g) for _ in range(3)]
    lams = [torch.tensor([0.3, 1.0, 0.0, 0.6, 0.6, 0.9, 0.5, 0.3], device=DEV),
            torch.tensor([0.9, 0.2, 0.7, 0.0, 1.0, 0.1, 0.4, 0.8], device=DEV), None]
    return xs, ys, lams


def _opt(T, m, lr=1e-3):
    return T.FusedAdamW(T.param_groups(m, lr=lr, head_lr=lr), lr=lr, weight_decay=0.05, distributed=False)


def test_graphed_distilled_step_matches_eager(favit, step_case):
    xs, ys, lams = step_case
    T = favit.train
    d = T.Distill(0.5, 3.0)
    favit.set_compute_dtype("bf16")
    try:
        m1, t1 = _vit(favit), _teacher(favit)
        o1 = _opt(T, m1)
        before = [p.detach().clone() for p in t1.parameters()]
        eager = [T.train_step(m1, x, y, o1, label_smoothing=0.1, mix_lam=l, teacher=t1, distill=d).item()
                 for x, y, l in zip(xs, ys, lams)]
        assert t1.training, "the teacher's training flag is left as found"
        m2, t2 = _vit(favit), _teacher(favit)
        o2 = _opt(T, m2)
        step = T.GraphedStep(m2, o2, xs[0], ys[0], label_smoothing=0.1, mix=True, teacher=t2, distill=d)
        graphed = [step(x, y, l).item() for x, y, l in zip(xs, ys, lams)]
        print(f"eager {eager} graphed {graphed} kd {step.kd.item()}")
        for a, b in zip(eager, graphed):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (eager, graphed)
        w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
        w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        assert rel_l2(w2.cpu(), w1.cpu()) < 1e-3
        assert t2.training and any(t is t2 for t in step._keep)
        for t in (t1, t2):
            for p, p0 in zip(t.parameters(), before):
                assert torch.equal(_bits(p), _bits(p0)) and p.grad is None
        assert bool(torch.isfinite(step.kd)) and step.kd.item() > 0
        # the teacher changed the loss: the same steps without it give another one
        m3 = _vit(favit)
        plain = T.train_step(m3, xs[0], ys[0], _opt(T, m3), label_smoothing=0.1, mix_lam=lams[0]).item()
        assert abs(plain - eager[0]) > 1e-2, (plain, eager[0])
        # a teacher and a Distill go together; a trainable teacher inside the optimizer is refused
        with pytest.raises(ValueError):
            T.train_step(m1, xs[0], ys[0], o1, teacher=t1)
        with pytest.raises(ValueError):
            T.GraphedStep(m2, o2, xs[0], ys[0], distill=d)
        with pytest.raises(ValueError, match="frozen"):
            T.teacher_logits(m1, xs[0], o1)
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_teacher_logits_runs_in_eval_without_a_tape(favit, step_case):
    xs, _, _ = step_case
    T = favit.train
    t = _teacher(favit)
    a, b = T.teacher_logits(t, xs[0]), T.teacher_logits(t, xs[0])
    assert t.training and a.dtype == torch.float32 and not a.requires_grad
    assert torch.equal(_bits(a), _bits(b)), "eval(): no dropout draw"
    t.eval()
    assert torch.equal(_bits(T.teacher_logits(t, xs[0])), _bits(a)) and not t.training


def test_twenty_steps_of_pure_distillation_lower_kd(favit, step_case):
    xs, ys, _ = step_case
    T = favit.train
    d = T.Distill(1.0, 2.0)
    favit.set_compute_dtype("bf16")
    try:
        m, t = _vit(favit), _teacher(favit)
        opt = _opt(T, m)

        def kd_now():
            m.eval()
            with torch.no_grad():
                kd = T.cross_entropy_distill(m(xs[0]), ys[0], T.teacher_logits(t, xs[0]), d)[1].item()
            m.train()
            return kd
        first = kd_now()
        for _ in range(20):
            T.train_step(m, xs[0], ys[0], opt, teacher=t, distill=d)
        last = kd_now()
        print(f"kd before {first!r} after {last!r}")
        assert last < first
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_fit_with_and_without_a_teacher(favit, step_case):
    xs, ys, _ = step_case
    T, H = favit.train, favit.harness
    quiet = lambda s: None
    loader, val = list(zip(xs, ys)), list(zip(xs[:1], ys[:1]))
    favit.set_compute_dtype("bf16")
    try:
        m, t = _vit(favit), _teacher(favit)
        res = H.fit(m, loader, val, _opt(T, m), 2, log=quiet, label_smoothing=0.1, teacher=t, distill=T.Distill(0.5, 3.0))
        h = res["history"]
        print(f"train_kd {h['train_kd']} train_loss {h['train_loss']}")
        assert len(h["train_kd"]) == 2 and all(v == v and abs(v) != float("inf") and v > 0 for v in h["train_kd"])
        assert len(h["val_loss"]) == 2 and t.training
        # Without a teacher: no such key, and the loop of before, i.e. the losses of the same steps taken by hand as
        # fit took them before it knew a teacher.  Bit for bit where the step is deterministic: the weight-gradient
        # GEMMs add their K-splits with fp32 atomics, so two runs of ONE loop from one seed already differ in the last
        # bits once an update has gone through them (measured here: second-epoch means of 2.114934762318929 and
        # 2.1149369875590005, each seen from fit and from the loop by hand in different runs).  So the bitwise
        # comparison runs at a learning rate of zero, where every loss is a forward pass on the initial weights, and
        # the trained run is held to the tolerance the graphed step is held to against the eager one.
        def by_fit(lr):
            m1 = _vit(favit)
            return H.fit(m1, loader, val, _opt(T, m1, lr), 2, log=quiet, label_smoothing=0.1)["history"]

        def by_hand(lr):
            m2 = _vit(favit)
            o2 = _opt(T, m2, lr)
            out = []
            for _ in range(2):
                m2.train()
                s = torch.zeros((), device=DEV)
                for x, y in loader:
                    o2.zero_grad()
                    loss = T.cross_entropy(m2(x), y, 0.1, None)
                    loss.backward()
                    o2.step()
                    s += loss.detach()
                out.append(s.item() / len(loader))
                H.evaluate(m2, val)                          # (the loop's validation pass, between the epochs as there)
            return out
        frozen = by_fit(0.0)
        assert "train_kd" not in frozen
        assert frozen["train_loss"] == by_hand(0.0), "lr 0: the losses of the loop of before, bit for bit"
        plain, hand = by_fit(1e-3), by_hand(1e-3)
        print(f"trained without a teacher: fit {plain['train_loss']} by hand {hand}")
        assert "train_kd" not in plain and plain["train_loss"][0] != plain["train_loss"][1]
        for u, v in zip(plain["train_loss"], hand):
            assert abs(u - v) < 2e-3 * max(1.0, abs(v)), (plain["train_loss"], hand)
        assert plain["train_loss"] != h["train_loss"]
        with pytest.raises(ValueError):
            H.fit(m, loader, val, _opt(T, m), 1, log=quiet, teacher=t)
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_fit_resumes_with_a_rebuilt_teacher(favit, step_case, tmp_path):
    """The teacher is not in the checkpoint: the caller rebuilds it, and the history -- train_kd included -- is extended."""
    xs, ys, _ = step_case
    T, H = favit.train, favit.harness
    quiet = lambda s: None
    loader, path, d = list(zip(xs, ys)), str(tmp_path / "fit.pt"), T.Distill(0.5, 3.0)
    favit.set_compute_dtype("bf16")
    try:
        m = _vit(favit)
        first = H.fit(m, loader, None, _opt(T, m), 1, log=quiet, teacher=_teacher(favit), distill=d, checkpoint=path)
        saved = torch.load(path, map_location="cpu", weights_only=True)
        assert set(saved["model"]) == set(m.state_dict()), "the student's keys and nothing of the teacher"
        m = _vit(favit, seed=5)
        both = H.fit(m, loader, None, _opt(T, m), 2, log=quiet, teacher=_teacher(favit), distill=d, checkpoint=path,
                     resume=True)["history"]
        assert both["train_kd"][:1] == first["history"]["train_kd"] and len(both["train_kd"]) == 2
        assert len(both["train_loss"]) == 2 and all(v == v for v in both["train_kd"])
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
