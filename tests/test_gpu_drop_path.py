"""Stochastic depth (DropPath) on the GPU: the kernel pair against the host restatement of its draw, then whole models
against float64 references built with the masks rebuilt from the documented seed order (functional.EncoderOp).

Tolerances.  Kernels: bit equality, except the kept rows of the forward, |out - (x + y * scale)| <= 2 * 2^-23 *
(|x| + |y * scale|) against float64 -- two fp32 roundings.  Whole models, fp32 mode: 2e-4 rel-L2 for the logits and for
every parameter gradient, the figure tests/test_gpu_cls_only.py uses against the oracle and between the pruned and the
full path.  bf16 mode: 2e-2 for the logits (the stated bf16 tolerance of tests/test_gpu_modules.py) and 4e-2 for every
parameter gradient (the gradient figure of its bf16 block test).  Graph against eager: 2e-3 on the losses and 1e-3
rel-L2 on the weights, as tests/test_gpu_modules.py::test_graphed_step_with_dropout_matches_eager_steps."""
import ctypes

import numpy as np
import pytest
import torch

import _dropout_ref as DR
import _drop_path_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
KERNEL_SEEDS = (3, 226934135264)        # (host restatement: samples 0..2 hold a kept and a dropped one at p = 0.1 and 0.5)
MODEL_SEED = 0                          # torch seed of the whole-model forwards (checked below against the rebuilt masks)
FP32_TOL, BF16_LOGITS, BF16_GRADS = 2e-4, 2e-2, 4e-2


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


@pytest.fixture(autouse=True)
def _clean_state(favit):
    favit.set_compute_dtype("fp32")
    favit.functional.set_dropout_epoch(None)
    yield
    favit.functional.set_dropout_epoch(None)
    favit.set_compute_dtype("fp32")
    favit.functional.clear_lp_mirrors()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", KERNEL_SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_kernels_match_the_host_restatement(K, B, p, seed):
    keep = R.sample_keep(seed, B, p)
    if B >= 3:
        assert keep.any() and not keep.all(), "choose a seed with a kept and a dropped sample"
    keep_t = torch.from_numpy(keep)
    scale32 = torch.tensor(DR.keep_scale(p), dtype=F32)
    lp_p, lp_seed = 0.25, seed + 12345
    lp_scale32 = torch.tensor(DR.keep_scale(lp_p), dtype=F32)
    g_ = torch.Generator().manual_seed(1000 * B + int(100 * p))
    for n in (1, 5, 17):
        for D in (64, 192, 384):
            x = torch.randn(B, n, D, generator=g_)
            y = torch.randn(B, n, D, generator=g_)
            g = torch.randn(B, n, D, generator=g_)
            tag = (B, n, D, p, seed)
            xd = x.reshape(B * n, D).to(DEV)
            # forward: dropped samples copy x bit for bit and never read y (NaN there); kept ones within two roundings
            for ydt in (F32, BF16):
                yq = y.to(ydt)
                y_nan = yq.clone()
                y_nan[~keep_t] = float("nan")
                yd = y_nan.reshape(B * n, D).to(DEV)
                out_d = K.drop_path_add(xd, yd, B, n, D, p, seed)
                out = out_d.cpu().reshape(B, n, D)
                assert torch.equal(_bits(out[~keep_t]), _bits(x[~keep_t])), (tag, ydt, "dropped rows")
                ys = yq[keep_t].double() * float(scale32)
                ref = x[keep_t].double() + ys
                err = (out[keep_t].double() - ref).abs()
                bound = 2.0 * 2.0 ** -23 * (x[keep_t].double().abs() + ys.abs())
                assert bool((err <= bound).all()), (tag, ydt, float((err - bound).max()))
                x2 = xd.clone()
                assert K.drop_path_add(x2, yd, B, n, D, p, seed, out=x2) is x2
                assert torch.equal(_bits(x2), _bits(out_d)), (tag, ydt, "out aliasing x")
                if ydt == F32:
                    y2 = yd.clone()
                    K.drop_path_add(xd, y2, B, n, D, p, seed, out=y2)
                    assert torch.equal(_bits(y2), _bits(out_d)), (tag, "out aliasing y")
            # backward: the scaled copy in both dtypes, zeros for dropped samples (whose rows of g hold NaN)
            g_nan = g.clone()
            g_nan[~keep_t] = float("nan")
            gd = g_nan.reshape(B * n, D).to(DEV)
            prod = g * scale32
            lp_keep = torch.from_numpy(DR.keep_mask(lp_seed, B * n * D, lp_p).reshape(B, n, D))
            for dt in (F32, BF16):
                want = prod.clone()
                want[~keep_t] = 0.0
                got = K.drop_path_bwd(gd, dt, B, n, D, p, seed).cpu().reshape(B, n, D)
                assert got.dtype == dt and torch.equal(_bits(got), _bits(want.to(dt))), (tag, dt, "backward")
                want = torch.where(lp_keep, prod * lp_scale32, torch.zeros(()))
                want[~keep_t] = 0.0
                got = K.drop_path_bwd(gd, dt, B, n, D, p, seed, lp_drop=(lp_p, lp_seed)).cpu().reshape(B, n, D)
                assert torch.equal(_bits(got), _bits(want.to(dt))), (tag, dt, "backward with the output-dropout mask")


def test_refusals_launch_nothing(K, favit):
    A = favit._abi
    lib = A.lib()
    B, n, D = 3, 5, 64
    x = torch.randn(B * n, D, device=DEV)
    y = torch.randn(B * n, D, device=DEV)
    g = torch.randn(B * n, D, device=DEV)
    out = torch.full((B * n, D), 7.0, device=DEV)
    lp = torch.full((B * n, D), 7.0, device=DEV, dtype=BF16)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = K._st()
    add = lambda B=B, n=n, D=D, p=0.5, xp=P(x): lib.favit_drop_path_add(xp, P(y), A.F32, P(out), B, n, D, p, 3, st)
    bwd = lambda B=B, n=n, D=D, p=0.5, lpp=0.0, gp=P(g): lib.favit_drop_path_bwd(gp, P(lp), A.BF16, B, n, D, p, 3, lpp, 4, st)
    for fn in (add, bwd):
        assert fn(p=1.0) == fn(p=-0.25) == fn(B=0) == fn(n=-1) == fn(D=0) == A.ERR_INVALID
        assert fn(D=60) == fn(D=4) == A.ERR_UNSUPPORTED
    assert add(xp=None) == bwd(gp=None) == bwd(lpp=1.0) == A.ERR_INVALID
    with pytest.raises(RuntimeError, match="favit_drop_path_add"):
        K.drop_path_add(x, y, B, n, D, 1.0, 3, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lp == 7.0).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------------------
# whole models
# ------------------------------------------------------------------------------------------------------------------
B_, P_, D_, H_, W_, DEPTH, RATE = 6, 4, 64, 2, 7, 4, 0.5


def _mhla_model(favit, rate=None, seed=11):
    torch.manual_seed(seed)
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=P_, num_classes=10, embed_dim=D_, depth=DEPTH,
                                                    num_heads=H_, window_size=W_, use_mhla=True)
    x = torch.randn(B_, 3, 32, 32)
    y = torch.randint(0, 10, (B_,))
    return (m if rate is None else m.set_drop_path_rate(rate)), x, y


def _step(favit, m, xd, yd, torch_seed=MODEL_SEED):
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(torch_seed)
    logits = m(xd)
    favit.train.cross_entropy(logits, yd).backward()
    torch.cuda.synchronize()
    return logits.detach().float().cpu(), {k: p.grad.detach().float().cpu() for k, p in m.named_parameters()}


def _mhla_scales():
    """The [B] scales of the eight halves under MODEL_SEED: block 0 has rate 0 and draws nothing; blocks 1..3 draw one
    seed for the attention half, then one for the MLP half (no element dropout: no other seed in between)."""
    rates = R.linear_rates(RATE, DEPTH)
    seeds = iter(R.expected_seeds(MODEL_SEED, 2 * (DEPTH - 1)))
    scales = [(torch.ones(B_, dtype=torch.float64),) * 2]
    for i in range(1, DEPTH):
        scales.append((R.sample_scale(next(seeds), B_, rates[i]), R.sample_scale(next(seeds), B_, rates[i])))
    return scales


@pytest.fixture(scope="module")
def mhla_ref(favit):
    """float64 logits and gradients of the drop-path model under the rebuilt masks: computed once, read by every test."""
    scales = _mhla_scales()
    for i in range(1, DEPTH):
        assert any(bool((s == 0).any()) and bool((s != 0).any()) for s in scales[i]), \
            f"block {i}: choose a torch seed that drops and keeps a sample in one of its halves"
    m, x, y = _mhla_model(favit, RATE)
    logits, grads = R.reference(m, x, y, P_, H_, "mhla", scales, W_)
    return logits, grads


def _check(got, ref, tol_logits, tol_grads, what):
    (lg, gr), (rl, rg) = got, ref
    e = rel_l2(lg, rl)
    worst = max((rel_l2(gr[k], rg[k]), k) for k in gr)
    print(f"\n[{what}] logits rel-L2 {e:.2e}; worst gradient {worst[0]:.2e} ({worst[1]})", end="")
    assert e < tol_logits, (what, e)
    assert worst[0] < tol_grads, (what, worst)


class _Count:
    def __init__(self, K, monkeypatch, *names):
        self.n = {k: 0 for k in names}
        for name in names:
            monkeypatch.setattr(K, name, self._wrap(name, getattr(K, name)))

    def _wrap(self, name, orig):
        def counted(*a, **k):
            self.n[name] += 1
            return orig(*a, **k)
        return counted


def test_fp32_model_pruned_and_full_against_the_reference(favit, K, monkeypatch, mhla_ref):
    m, x, y = _mhla_model(favit, RATE)
    m.to(DEV).train()
    xd, yd = x.to(DEV), y.to(DEV)
    cnt = _Count(K, monkeypatch, "rows_cut_fwd", "drop_path_add", "drop_path_bwd")
    monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
    monkeypatch.delenv("FAVIT_NO_MLP_NARROW", raising=False)
    pruned = _step(favit, m, xd, yd)
    assert cnt.n["rows_cut_fwd"] == DEPTH, "L = 65: every block of this model is pruned, with a drop-path rate too"
    assert cnt.n["drop_path_add"] == cnt.n["drop_path_bwd"] == 2 * (DEPTH - 1), "one pair per half with a rate > 0"
    _check(pruned, mhla_ref, FP32_TOL, FP32_TOL, "fp32 pruned vs float64")
    monkeypatch.setenv("FAVIT_NO_PRUNE", "1")
    full = _step(favit, m, xd, yd)
    assert cnt.n["rows_cut_fwd"] == DEPTH, "FAVIT_NO_PRUNE=1 takes the full path"
    _check(full, mhla_ref, FP32_TOL, FP32_TOL, "fp32 full vs float64")
    _check(pruned, full, FP32_TOL, FP32_TOL, "fp32 pruned vs full: the same draw in both row layouts")
    # another torch seed draws other masks
    other = _step(favit, m, xd, yd, torch_seed=MODEL_SEED + 1)
    assert rel_l2(other[0], full[0]) > 1e-3


@pytest.mark.parametrize("narrow", [True, False])
def test_bf16_model_against_the_reference(favit, K, monkeypatch, mhla_ref, narrow):
    favit.set_compute_dtype("bf16")
    m, x, y = _mhla_model(favit, RATE)
    m.to(DEV).train()
    monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
    if narrow:
        monkeypatch.delenv("FAVIT_NO_MLP_NARROW", raising=False)
    else:
        monkeypatch.setenv("FAVIT_NO_MLP_NARROW", "1")
    cnt = _Count(K, monkeypatch, "rows_cut_fwd", "drop_path_add")
    got = _step(favit, m, x.to(DEV), y.to(DEV))
    assert cnt.n["rows_cut_fwd"] == DEPTH and cnt.n["drop_path_add"] == 2 * (DEPTH - 1)
    _check(got, mhla_ref, BF16_LOGITS, BF16_GRADS, f"bf16 narrow={narrow} vs float64")


def test_combined_with_element_dropout(favit, K, monkeypatch):
    """dropout = 0.1 (both MLP sites) and drop_path_rate = 0.5 on a dense-attention VisionTransformer of depth 2, fp32:
    block 0 draws (fc1, fc2); block 1 draws (attention drop path), (fc1, fc2), (MLP drop path) -- the seed order -- and
    its fc2 mask reaches backward through favit_drop_path_bwd (the premasked chain)."""
    H, hidden, L = 4, 4 * D_, 65
    torch.manual_seed(5)
    m = favit.models.vit.VisionTransformer(img_size=32, patch_size=P_, num_classes=10, embed_dim=D_, depth=2,
                                           num_heads=H, dropout=0.1).set_drop_path_rate(RATE)
    x = torch.randn(B_, 3, 32, 32)
    y = torch.randint(0, 10, (B_,))
    s = R.expected_seeds(MODEL_SEED, 6)
    M = B_ * L
    ones = torch.ones(B_, dtype=torch.float64)
    sa, sm = R.sample_scale(s[2], B_, RATE), R.sample_scale(s[5], B_, RATE)
    for t in (sa, sm):
        assert bool((t == 0).any()) and bool((t != 0).any()), "choose a torch seed that drops and keeps a sample"
    scales = [(ones, ones), (sa, sm)]
    drops = [(R.element_keep(s[0], M, hidden, 0.1), R.element_keep(s[1], M, D_, 0.1)),
             (R.element_keep(s[3], M, hidden, 0.1), R.element_keep(s[4], M, D_, 0.1))]
    ref = R.reference(m, x, y, P_, H, "dense", scales, mlp_drops=drops)
    m.to(DEV).train()
    cnt = _Count(K, monkeypatch, "drop_path_add", "drop_path_bwd", "dropout")
    got = _step(favit, m, x.to(DEV), y.to(DEV))
    assert cnt.n["drop_path_add"] == cnt.n["drop_path_bwd"] == 2
    assert cnt.n["dropout"] == 0, "no separate masking pass: every output-dropout mask rides in a copy that is written anyway"
    _check(got, ref, FP32_TOL, FP32_TOL, "fp32 dense, dropout 0.1 + drop path 0.5 vs float64")


def test_off_means_off(favit, K, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a drop-path kernel was launched with no rate in force")
    monkeypatch.setattr(K, "drop_path_add", boom)
    monkeypatch.setattr(K, "drop_path_bwd", boom)
    plain, x, y = _mhla_model(favit)
    xd, yd = x.to(DEV), y.to(DEV)
    plain.to(DEV)
    # eval mode with a rate
    rated, _, _ = _mhla_model(favit, 0.3)
    rated.to(DEV).eval()
    plain.eval()
    st = torch.get_rng_state()
    with torch.no_grad():
        a, b = rated(xd), plain(xd)
    assert torch.equal(_bits(a.float()), _bits(b.float()))
    assert torch.equal(st, torch.get_rng_state()), "no seed is drawn"
    # training mode with rate 0
    zero, _, _ = _mhla_model(favit, 0.0)
    zero.to(DEV).train()
    plain.train()
    st = torch.get_rng_state()
    logits = zero(xd)
    assert torch.equal(st, torch.get_rng_state()), "no seed is drawn"
    favit.train.cross_entropy(logits, yd).backward()
    want = plain(xd)
    favit.train.cross_entropy(want, yd).backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(logits.detach()), _bits(want.detach()))
    # Gradients: the same kernels with the same arguments, but not all of them are reproducible to the bit from one
    # backward pass to the next of ONE model: favit_mhla_fold_bwd adds the latent_proj gradient with fp32 atomics across
    # workgroups (measured here: one element of blocks.0.attn.latent_proj.weight one ulp apart between two such passes).
    # So: bit-equal, or within the bound tests/test_gpu_cls_only.py states for two runs of the same kernels whose fp32
    # atomic adds arrive in another order (1e-5 rel-L2: a reordered sum of a few hundred terms is about 1e-6).  Other
    # gradients are summed with fp32 atomics as well (cls_token, pos_embed, split-K weight gradients in fp32 mode), so
    # no count of bit-equal tensors is asserted; it is printed.
    exact = 0
    for (k, p), q in zip(zero.named_parameters(), plain.parameters()):
        same = torch.equal(_bits(p.grad), _bits(q.grad))
        exact += int(same)
        assert same or rel_l2(p.grad, q.grad) < 1e-5, (k, rel_l2(p.grad, q.grad))
    n_par = len(list(plain.parameters()))
    print(f"\n[off means off] {exact} of {n_par} gradients bit-identical", end="")


def test_fp8_mode_with_an_active_rate_is_a_clear_error(favit):
    favit.set_compute_dtype("fp8")
    m, x, y = _mhla_model(favit, RATE)
    m.to(DEV).train()
    with pytest.raises(NotImplementedError, match="fp8"):
        m(x.to(DEV))
    m.eval()
    with torch.no_grad():
        assert m(x.to(DEV)).shape == (B_, 10)


def test_graphed_step_draws_fresh_masks_and_matches_eager(favit, monkeypatch):
    favit.set_compute_dtype("bf16")
    F = favit.functional
    counter = {"n": 0}

    def fake_seed():
        counter["n"] += 1
        return 0x5DEECE66D * counter["n"] + 11

    monkeypatch.setattr(F, "_seed", fake_seed)

    def build():
        m, _, _ = _mhla_model(favit, RATE)
        m.to(DEV).train()
        opt = favit.train.FusedAdamW(favit.train.param_groups(m, lr=1e-3), lr=1e-3, weight_decay=0.05, distributed=False)
        return m, opt, [g["lr"] for g in opt.groups]

    def set_lr(opt, lrs):
        for g, lr in zip(opt.groups, lrs):
            g["lr"] = lr

    gen = torch.Generator(device=DEV).manual_seed(2)
    xs = [torch.randn(8, 3, 32, 32, device=DEV, generator=gen) for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device=DEV, generator=gen) for _ in range(3)]
    # steps 0 and 1: the same batch at learning rate 0 (identical weights); steps 2 and 3: two more batches at 1e-3
    plan = [(0, 0.0), (0, 0.0), (1, None), (2, None)]
    m2, o2, lrs = build()
    counter["n"] = 0
    step = favit.train.GraphedStep(m2, o2, xs[0], ys[0], warmup=1)
    assert step.epoch is not None and F.get_dropout_epoch() is step.epoch, "a drop-path rate registers the epoch word"
    n = counter["n"] // 2
    assert n == 2 * (DEPTH - 1) and counter["n"] == 2 * n
    graphed = []
    for b, lr in plan:
        set_lr(o2, [0.0] * len(lrs) if lr == 0.0 else lrs)
        graphed.append(step(xs[b], ys[b]).item())
    assert int(step.epoch.item()) == 2 + len(plan) - 1
    assert graphed[0] != graphed[1], "two replays from identical weights on one batch: the epoch word reaches the new kernels"
    m1, o1, _ = build()
    eager = []
    for k, (b, lr) in enumerate(plan):
        counter["n"] = n
        step.epoch.fill_(k + 2)
        set_lr(o1, [0.0] * len(lrs) if lr == 0.0 else lrs)
        eager.append(favit.train.train_step(m1, xs[b], ys[b], o1).item())
    print(f"\n[graph vs eager] {graphed} {eager}", end="")
    for a, b in zip(eager, graphed):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (eager, graphed)
    w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
    w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
    assert rel_l2(w2.cpu(), w1.cpu()) < 1e-3
