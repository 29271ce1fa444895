"""Batch mixing on the GPU: favit_batch_mix against an fp64 reference built from explicit lam / box, the mixed-target
loss favit_cross_entropy_mix against fp64 autograd, the graphed step that reads lam at replay, and the loader."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


def _bits(t):
    return t.contiguous().view(torch.int32)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------------------------------------------
def check_mix(before, after, lam, box):
    """`after` against the mix of `before` (fp32 [B,C,H,W], both on any device) by host lam [B] / box [B,4]: CutMix and
    unchanged pixels bit for bit, Mixup pixels within 4 * 2^-24 * (|a| + |q|) of the fp64 value (three fp32 roundings:
    1 - lam, the product, the fused or unfused sum).  Returns the largest Mixup error over its bound."""
    x, out = before.detach().cpu(), after.detach().cpu()
    B = x.shape[0]
    worst = 0.0
    for b in range(B):
        p = B - 1 - b
        y0, y1, x0, x1 = (int(v) for v in box[b])
        if p != b and y0 < y1 and x0 < x1:
            want = x[b].clone()
            ys, xs = slice(max(y0, 0), max(y1, 0)), slice(max(x0, 0), max(x1, 0))
            want[:, ys, xs] = x[p][:, ys, xs]
            assert torch.equal(_bits(out[b]), _bits(want)), f"row {b} (CutMix {y0, y1, x0, x1}) is not bit-exact"
        elif p == b or float(lam[b]) == 1.0:
            assert torch.equal(_bits(out[b]), _bits(x[b])), f"row {b} (unchanged) is not bit-exact"
        else:
            l64 = float(np.float32(lam[b]))
            a, q = x[b].double(), x[p].double()
            err = (out[b].double() - (l64 * a + (1.0 - l64) * q)).abs()
            bound = 4.0 * 2.0 ** -24 * (a.abs() + q.abs())
            assert bool((err <= bound).all()), f"row {b} (Mixup lam {l64}): error {err.max().item():.3e} over the bound"
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


def _mix_case(B, S):
    """lam / box rows that cover, within one batch: empty / whole-image / single-pixel boxes, x0 = 1 .. x1 = S-1, a box
    reaching the last row and column, a pair with two different boxes, a Mixup row paired with an unchanged one,
    lam in {0, 0.3, 1}."""
    whole, pixel = (0, S, 0, S), (S // 2, S // 2 + 1, 5, 6)
    inner, corner, none = (0, S, 1, S - 1), (S - 5, S, S - 3, S), (0, 0, 0, 0)
    if B == 8:      # pairs (0,7) (1,6) (2,5) (3,4)
        rows = [(0.3, none), (0.5, whole), (0.7, inner), (0.0, none),
                (0.3, none), (0.9, corner), (0.99, pixel), (1.0, none)]
    elif B == 5:    # pairs (0,4) (1,3); row 2 is the middle row: whatever it carries, it never changes
        rows = [(1.0, none), (0.7, inner), (0.3, corner), (0.3, none), (1.0, none)]
    elif B == 2:    # a box that overhangs the image on every side next to a row that takes its partner whole (lam 0)
        rows = [(0.5, (-3, S // 2, S - 6, S + 9)), (0.0, none)]
    else:
        rows = [(0.3, whole)]
    lam = np.array([r[0] for r in rows], dtype=np.float32)
    box = np.array([r[1] for r in rows], dtype=np.int32)
    return lam, box


@pytest.mark.parametrize("S", [30, 32])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B", [1, 2, 5, 8])
def test_batch_mix(K, B, C, S):
    g = torch.Generator(device=DEV).manual_seed(100 * B + 10 * C + S)
    x = torch.randn(B, C, S, S, device=DEV, generator=g)
    lam, box = _mix_case(B, S)
    if B == 8:      # special bit patterns in rows that are only copied: they must survive as they are
        x[1, 0, 0, :4] = torch.tensor([-0.0, float("inf"), float("nan"), 1e-45], device=DEV)
        x[6, 0, S // 2, 4:8] = torch.tensor([-0.0, float("-inf"), 3e38, -1e-45], device=DEV)
    d_lam, d_box = torch.from_numpy(lam).to(DEV), torch.from_numpy(box).to(DEV)
    y1, y2 = x.clone(), x.clone()
    assert K.batch_mix(y1, d_lam, d_box) is y1
    K.batch_mix(y2, d_lam, d_box)
    worst = check_mix(x, y1, lam, box)
    print(f"B={B} C={C} S={S}: largest Mixup error / bound {worst:.3f}")
    assert torch.equal(_bits(y1), _bits(y2)), "the same call on the same input gives the same bits"
    if B > 1:
        assert not torch.equal(_bits(y1), _bits(x)), "the case mixes something"


def test_batch_mix_unaligned_base_and_arguments(favit, K):
    # W % 4 == 0 but a base address that is not 16-byte aligned: the 4-byte path
    B, C, S = 4, 2, 32
    g = torch.Generator(device=DEV).manual_seed(3)
    buf = torch.randn(B * C * S * S + 1, device=DEV, generator=g)
    x = buf[1:].view(B, C, S, S)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    lam = np.array([0.3, 0.6, 1.0, 0.25], dtype=np.float32)
    box = np.array([[0, 0, 0, 0], [3, 17, 2, 31], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    before, guard = x.clone(), buf[:1].clone()
    K.batch_mix(x, torch.from_numpy(lam).to(DEV), torch.from_numpy(box).to(DEV))
    check_mix(before, x, lam, box)
    assert torch.equal(_bits(buf[:1]), _bits(guard)), "the float in front of the batch is not touched"
    # arguments
    lib, E = favit._abi.lib(), favit._abi.ERR_INVALID
    d_lam, d_box, st = torch.ones(B, device=DEV), torch.zeros(B, 4, dtype=torch.int32, device=DEV), _st()
    assert lib.favit_batch_mix(None, _P(d_lam), _P(d_box), B, C, S, S, st) == E
    assert lib.favit_batch_mix(_P(x), None, _P(d_box), B, C, S, S, st) == E
    assert lib.favit_batch_mix(_P(x), _P(d_lam), None, B, C, S, S, st) == E
    for dims in ((0, C, S, S), (B, 0, S, S), (B, C, -1, S), (B, C, S, 0)):
        assert lib.favit_batch_mix(_P(x), _P(d_lam), _P(d_box), *dims, st) == E
    one = x[:1].clone()
    assert lib.favit_batch_mix(_P(one), _P(torch.zeros(1, device=DEV)), _P(d_box), 1, C, S, S, st) == 0
    assert torch.equal(_bits(one), _bits(x[:1])), "B == 1 succeeds and does nothing"
    with pytest.raises(TypeError):
        K.batch_mix(x.double(), d_lam, d_box)
    with pytest.raises(TypeError):
        K.batch_mix(x, d_lam[:2], d_box)
    with pytest.raises(TypeError):
        K.batch_mix(x, d_lam, d_box.long())


# ----------------------------------------------------------------------------------------------------------------
def _ce_case(B, Cn):
    g = torch.Generator(device=DEV).manual_seed(1000 * B + Cn)
    logits = torch.randn(B, Cn, device=DEV, generator=g) * 3
    if B > 1:
        logits[min(5, B - 2)] = 80.0 * (1 - 2 * (torch.arange(Cn, device=DEV) % 2))          # one row of +-80
    labels = torch.randint(0, Cn, (B,), device=DEV, generator=g)
    if B > 1:
        labels[B - 1] = labels[0]                                   # a pair with y_b == y_p (besides an odd middle row)
    lam = torch.tensor([(0.0, 0.3, 1.0, 0.75)[b % 4] for b in range(B)], device=DEV)
    return logits, labels, lam


def _ce_reference(logits, labels, lam, eps):
    """fp64 -sum t log_softmax, mean over rows, t = (1 - eps) (lam onehot(y) + (1 - lam) onehot(y flipped)) + eps / C."""
    B, Cn = logits.shape
    z = logits.double().cpu().requires_grad_(True)
    hot = torch.nn.functional.one_hot(labels.cpu(), Cn).double()
    l = lam.double().cpu()[:, None]
    t = (1.0 - eps) * (l * hot + (1.0 - l) * hot.flip(0)) + eps / Cn
    loss = -(t * torch.log_softmax(z, dim=1)).sum(1).mean()
    loss.backward()
    return loss.item(), z.grad


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("Cn", [10, 65, 1000])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_cross_entropy_mix(favit, K, B, Cn, eps):
    logits, labels, lam = _ce_case(B, Cn)
    ref, ref_grad = _ce_reference(logits, labels, lam, eps)
    rows, dlog = K.cross_entropy(logits, labels, grad_scale=1.0 / B, label_smoothing=eps, mix_lam=lam)
    print(f"B={B} C={Cn} eps={eps}: loss {rows.double().mean().item()!r} ref {ref!r}; "
          f"dlogits rel-L2 {rel_l2(dlog, ref_grad):.3e}")
    assert abs(rows.double().mean().item() - ref) < 1e-5
    assert rel_l2(dlog, ref_grad) < 2e-5
    rows_only, none = K.cross_entropy(logits, labels, label_smoothing=eps, mix_lam=lam)       # dlogits may be null
    assert none is None and torch.equal(_bits(rows_only), _bits(rows))
    # lam all ones: the bits of the unmixed kernels with the same eps
    ones = torch.ones(B, device=DEV)
    rows1, dlog1 = K.cross_entropy(logits, labels, grad_scale=1.0 / B, label_smoothing=eps, mix_lam=ones)
    rows0, dlog0 = K.cross_entropy(logits, labels, grad_scale=1.0 / B, label_smoothing=eps)
    assert torch.equal(_bits(rows1), _bits(rows0)) and torch.equal(_bits(dlog1), _bits(dlog0))
    # A label out of range makes its own row NaN (own label) and the row paired with it NaN (partner label); every
    # other row keeps its bits.  In the middle row of an odd batch the two coincide: exactly one NaN row.
    for i in sorted({0, B // 2}):
        lab2 = labels.clone()
        lab2[i] = -100 if i == 0 else Cn
        rows2, dlog2 = K.cross_entropy(logits, lab2, grad_scale=1.0 / B, label_smoothing=eps, mix_lam=lam)
        bad = sorted({i, B - 1 - i})
        keep = [b for b in range(B) if b not in bad]
        assert bool(torch.isnan(rows2[bad]).all()), (i, rows2)
        assert torch.equal(_bits(rows2[keep]), _bits(rows[keep])) and torch.equal(_bits(dlog2[keep]), _bits(dlog[keep]))
        assert bool(torch.isfinite(dlog2).all())
    # label_smoothing = 1 is refused by the library itself
    lib = favit._abi.lib()
    assert lib.favit_cross_entropy_mix(_P(logits), _P(labels), _P(lam), _P(rows1), _P(dlog1), B, Cn, 1.0 / B, 1.0,
                                       _st()) == favit._abi.ERR_INVALID
    assert lib.favit_cross_entropy_mix(_P(logits), _P(labels), None, _P(rows1), _P(dlog1), B, Cn, 1.0 / B, eps,
                                       _st()) == favit._abi.ERR_INVALID
    # the autograd wrapper
    x = logits.clone().requires_grad_(True)
    loss = favit.train.cross_entropy(x, labels, label_smoothing=eps, mix_lam=lam)
    loss.backward()
    assert abs(loss.item() - ref) < 1e-5 and rel_l2(x.grad, ref_grad) < 2e-5


# ----------------------------------------------------------------------------------------------------------------
def _vit(favit, seed=11):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                       num_heads=4, use_mhla=True).to(DEV).train()


@pytest.fixture(scope="module")
def step_case():
    g = torch.Generator(device=DEV).manual_seed(2)
    xs = [torch.randn(8, 3, 32, 32, device=DEV, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device=DEV, generator=g) for _ in range(3)]
    lams = [torch.tensor([0.3, 1.0, 0.0, 0.6, 0.6, 0.9, 0.5, 0.3], device=DEV),
            torch.tensor([0.9, 0.2, 0.7, 0.0, 1.0, 0.1, 0.4, 0.8], device=DEV), None]
    return xs, ys, lams


def test_graphed_mix_step_matches_eager(favit, step_case):
    """Three replays -- two different lam vectors, then none -- against eager train_step(..., mix_lam=) from the same
    state, compared as tests/test_gpu_stabilisers.py compares its graphed step with the eager one."""
    xs, ys, lams = step_case
    T = favit.train
    favit.set_compute_dtype("bf16")

    def build():
        m = _vit(favit)
        return m, T.FusedAdamW(T.param_groups(m, lr=1e-3), lr=1e-3, weight_decay=0.05, distributed=False)
    try:
        m1, o1 = build()
        eager = [T.train_step(m1, x, y, o1, label_smoothing=0.1, mix_lam=l).item() for x, y, l in zip(xs, ys, lams)]
        m2, o2 = build()
        step = T.GraphedStep(m2, o2, xs[0], ys[0], label_smoothing=0.1, mix=True)
        graphed = [step(x, y, l).item() for x, y, l in zip(xs, ys, lams)]
        print(f"eager {eager} graphed {graphed}")
        for a, b in zip(eager, graphed):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (eager, graphed)
        w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
        w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        assert rel_l2(w2.cpu(), w1.cpu()) < 1e-3
        # a step captured without mix takes no lam
        m3, o3 = build()
        plain = T.GraphedStep(m3, o3, xs[0], ys[0], label_smoothing=0.1)
        with pytest.raises(ValueError, match="mix=True"):
            plain(xs[0], ys[0], lams[0])
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_graphed_step_reads_lam_at_replay(favit, step_case):
    """With a learning rate of zero the weights stand still, so two replays on the same batch differ through lam alone:
    each equals the eager loss of its own lam, and the second differs from the first.  Without lam the replay is the
    unmixed step.

    (At initialisation the logits of all rows are nearly alike, and then the mean loss barely depends on which rows
    carry which labels.  So the head's bias is set to the class index, the first half of the batch gets low labels and
    the second half high ones, and the second lam moves only the first half onto its partners' labels: the mean target
    logit goes from about 4.5 to about 7.5, a loss difference of about 3 against a comparison tolerance of 0.01.)"""
    xs, ys, _ = step_case
    T = favit.train
    x, y = xs[0], torch.tensor([0, 1, 2, 3, 9, 8, 7, 6], device=DEV)
    lam_a, lam_b = torch.ones(8, device=DEV), torch.tensor([0.0] * 4 + [1.0] * 4, device=DEV)
    favit.set_compute_dtype("bf16")
    try:
        m = _vit(favit)
        with torch.no_grad():
            m.head.bias.copy_(torch.arange(10.0))
        opt = T.FusedAdamW(T.param_groups(m, lr=0.0, head_lr=0.0), lr=0.0, weight_decay=0.05, distributed=False)
        w0 = torch.cat([p.detach().flatten() for p in m.parameters()]).clone()
        with torch.no_grad():
            logits = m(x)
            want = [T.cross_entropy(logits, y, 0.0, l).item() for l in (lam_a, lam_b, None)]
        step = T.GraphedStep(m, opt, x, y, mix=True)
        got = [step(x, y, l).item() for l in (lam_a, lam_b, None)]
        print(f"eager {want} graphed {got}")
        assert torch.equal(w0, torch.cat([p.detach().flatten() for p in m.parameters()])), "lr 0: the weights stand still"
        for a, b in zip(want, got):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (want, got)
        tol = 2e-3 * max(1.0, abs(got[0]))
        assert abs(got[1] - got[0]) > 100 * tol, "lam is read when the graph replays, not frozen into it"
        assert abs(got[2] - got[0]) < tol, "no lam under mix=True: the buffer holds ones, the unmixed step"
        assert want[2] == want[0], "lam of ones: the bits of the unmixed loss"
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


# ----------------------------------------------------------------------------------------------------------------
def test_device_loader_mixes_after_the_transform(favit):
    D = favit.data
    B, S, half = 6, 32, (0.5, 0.5, 0.5)
    rs = np.random.RandomState(0)
    host = [(rs.randint(0, 256, size=(B, 40, 40, 3)).astype(np.uint8), rs.randint(0, 10, size=B)) for _ in range(3)]

    def parts(seed_tf, seed_mix):
        return (D.DeviceTransform("resize_flip", S, half, half, seed=seed_tf),
                D.BatchMix(0.8, 1.0, prob=0.9, mode="elem", seed=seed_mix))

    tf, mix = parts(7, 9)
    loader = D.DeviceLoader(host, tf, mix=mix)
    tf_ref, mix_ref = parts(7, 9)                          # the same streams, drawn by hand
    seen, state = [], None
    for k, (images, mixed) in enumerate(loader):
        assert isinstance(mixed, D.MixedLabels)
        clean = tf_ref(torch.from_numpy(host[k][0]).to(DEV))
        lam, box = mix_ref.params(B, S)
        check_mix(clean, images, lam, box)
        assert torch.equal(mixed.labels.cpu(), torch.from_numpy(host[k][1]).long())
        assert mixed.lam.dtype == torch.float32 and np.array_equal(mixed.lam.cpu().numpy(), lam)
        seen.append((images.clone(), lam, box))
        if k == 1:
            state = loader.state_dict()                    # mid-run: two batches drawn, one to come
    assert len(seen) == 3 and any((s[1] < 1).any() for s in seen)
    # a fresh loader with other seeds, given that state, draws the third batch's parameters and yields its bits
    tf2, mix2 = parts(70, 90)
    loader2 = D.DeviceLoader(host[2:], tf2, mix=mix2)
    loader2.load_state_dict(state)
    (images, mixed), = list(loader2)
    assert np.array_equal(mixed.lam.cpu().numpy(), seen[2][1]) and torch.equal(_bits(images), _bits(seen[2][0]))
    probe = D.BatchMix(0.8, 1.0, prob=0.9, mode="elem", seed=123)
    probe.load_state_dict(state["mix"])
    lam, box = probe.params(B, S)
    assert np.array_equal(lam, seen[2][1]) and np.array_equal(box, seen[2][2])
    # without mix: plain labels and the state of before
    plain = D.DeviceLoader(host[:1], parts(7, 9)[0])
    (images, labels), = list(plain)
    assert torch.is_tensor(labels) and set(plain.state_dict().keys()) == {"transform", "batches"}
    with pytest.raises(ValueError, match="mix"):
        plain.load_state_dict(state)
