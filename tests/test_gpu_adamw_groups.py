"""GPU tests of the segmented AdamW launch (favit_adamw_multi) and of what is built on it: train.FusedAdamW with
fuse_groups=True (one arena, one launch, one norm, one mirror, one GradSync) under the fine-tuning groups of
train.param_groups (layer-wise learning-rate decay, weight-decay exemptions).

The kernel's reference is the single-group launch it must reproduce BIT FOR BIT: a loop of kernels.adamw over the
segments' slices of a second copy of the same state.  The optimizer's references are the per-group FusedAdamW (bitwise,
from injected gradients -- a second backward would reorder the last bits of the kernels' atomics) and torch in float64 at
the bounds tests/test_gpu_stabilisers.py uses for the per-group optimizer."""
import ctypes
import importlib
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS = 0.9, 0.999, 1e-8
UNIT = 256


def _bits(t):
    t = t.detach()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().clone()


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


class _Layout:
    """Segment ends, per-segment rates (with zeros among them) and the shared, never written inputs of one layout."""

    def __init__(self, units, seed):
        self.ends, at = [], 0
        for u in units:
            at += u * UNIT
            self.ends.append(at)
        self.n = at
        self.lrs = [1e-3 * (s % 5) for s in range(len(units))]                 # 0.0 for every fifth segment
        self.wds = [0.05 * ((s + 1) % 3) for s in range(len(units))]           # 0.0 for every third
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.p0 = torch.randn(self.n, device=DEV, generator=g)
        self.g = [torch.randn(self.n, device=DEV, generator=g) * 2, torch.randn(self.n, device=DEV, generator=g)]

    def state(self):
        p = self.p0.clone()
        return {"p": p, "m": torch.zeros_like(p), "v": torch.zeros_like(p), "lp": p.to(torch.bfloat16), "ema": p.clone()}


@pytest.fixture(scope="module")
def layouts():
    small = _Layout([1, 3, 1, 40, 2], 21)
    rs = torch.Generator().manual_seed(22)
    units = torch.randint(1, 1024, (64,), generator=rs).tolist()
    units[-1] += max(0, (1 << 23) // UNIT - sum(units))
    big = _Layout(units, 23)
    # (above 2^23 elements: more than 4096 workgroups of 256 lanes x 16 B cover in one pass, whatever the grid rule)
    assert len(big.ends) == 64 and big.n >= 1 << 23 and big.n > 4096 * 256 * 4
    return {"small": small, "big": big}


def _coef(variant):
    return {"coef025": 0.25, "coef1": 1.0, "clip_ema": 0.25}.get(variant)


def _multi(K, lay, st, step, g, variant, coef=None, skip=False, ends=None):
    ema = variant in ("ema", "clip_ema")
    K.adamw_multi(st["p"], g, st["m"], st["v"], lay.ends if ends is None else ends, lay.lrs, lay.wds, B1, B2, EPS, step,
                  grad_scale=0.5, p_lp=st["lp"], coef=coef, skip_nonfinite=skip, ema=st["ema"] if ema else None,
                  ema_decay=0.9 if ema else 0.0)


def _loop(K, lay, st, step, g, variant, coef=None, skip=False):
    ema = variant in ("ema", "clip_ema")
    a = 0
    for s, b in enumerate(lay.ends):
        kw = {} if coef is None else dict(coef=coef, skip_nonfinite=skip)
        if ema:
            kw.update(ema=st["ema"][a:b], ema_decay=0.9)
        K.adamw(st["p"][a:b], g[a:b], st["m"][a:b], st["v"][a:b], lay.lrs[s], B1, B2, EPS, lay.wds[s], step,
                grad_scale=0.5, p_lp=st["lp"][a:b], **kw)
        a = b


def _same(x, y, what):
    for k in ("p", "m", "v", "lp", "ema"):
        assert torch.equal(_bits(x[k]), _bits(y[k])), f"{what}: {k} differs from the per-segment launches"


@pytest.mark.parametrize("variant", ["plain", "coef025", "coef1", "ema", "clip_ema"])
@pytest.mark.parametrize("which", ["small", "big"])
def test_segmented_launch_has_the_bits_of_the_per_segment_launches(K, layouts, which, variant):
    lay = layouts[which]
    c = _coef(variant)
    coef = None if c is None else torch.full((1,), c, device=DEV)
    one, ref = lay.state(), lay.state()
    for step in (1, 2):
        _multi(K, lay, one, step, lay.g[step - 1], variant, coef)
        _loop(K, lay, ref, step, lay.g[step - 1], variant, coef)
        _same(one, ref, f"{which}/{variant} step {step}")
    assert not torch.equal(_bits(one["p"]), _bits(lay.p0)) and bool(torch.isfinite(one["p"]).all())
    assert torch.equal(_bits(one["lp"]), _bits(one["p"].to(torch.bfloat16)))
    zero_rate = [s for s, (lr, wd) in enumerate(zip(lay.lrs, lay.wds)) if lr == 0.0]
    a = 0 if zero_rate[0] == 0 else lay.ends[zero_rate[0] - 1]
    assert torch.equal(_bits(one["p"][a:lay.ends[zero_rate[0]]]), _bits(lay.p0[a:lay.ends[zero_rate[0]]])), "rate 0 moves nothing"
    if variant in ("ema", "clip_ema"):
        assert not torch.equal(_bits(one["ema"]), _bits(lay.p0))
    else:
        assert torch.equal(_bits(one["ema"]), _bits(lay.p0)), "without ema the buffer is not part of the launch"


def test_nonfinite_coefficient_skips_or_propagates(favit, K, layouts):
    lay = layouts["small"]
    nan = torch.full((1,), float("nan"), device=DEV)
    health = favit.train.Health()
    try:
        st = lay.state()
        before = {k: _bits(t) for k, t in st.items()}
        _multi(K, lay, st, 1, lay.g[0], "clip_ema", nan, skip=True)
        for k, t in st.items():
            assert torch.equal(_bits(t), before[k]), f"a skipped launch wrote {k}"
        rep = health.poll()
        assert rep is not None and rep["non_finite"] == ["gradient"]
        assert rep["adamw_launches"] == 1, "the arena is one AdamW launch, also when skipped"
        health.words.zero_()
        one, ref = lay.state(), lay.state()
        _multi(K, lay, one, 1, lay.g[0], "clip_ema", nan, skip=False)
        _loop(K, lay, ref, 1, lay.g[0], "clip_ema", nan, skip=False)
        for k in ("p", "m", "v", "lp", "ema"):
            assert torch.equal(torch.isnan(one[k].float()).cpu(), torch.isnan(ref[k].float()).cpu()), k
        assert bool(torch.isnan(one["m"]).all())
        rep = health.poll()
        assert rep is not None and "gradient" in rep["non_finite"] and "parameter" in rep["non_finite"]
        assert rep["adamw_launches"] == 1 + len(lay.ends)
        # a clean launch performs no atomic but its own count
        health.words.zero_()
        _multi(K, lay, lay.state(), 1, lay.g[0], "plain")
        assert health.poll() is None and int(health.words[3]) == 1
    finally:
        health.close()


def test_refused_tables_raise_and_write_nothing(favit, K, layouts):
    lay = layouts["small"]
    st = lay.state()
    before = {k: _bits(t) for k, t in st.items()}
    n = lay.n
    bad = {
        "an end of 128": [128] + lay.ends[1:],
        "a descending end": [lay.ends[1], lay.ends[0]] + lay.ends[2:],
        "end[-1] != n": lay.ends[:-1] + [n - UNIT],
        "end[-1] beyond n": lay.ends[:-1] + [n + UNIT],
    }
    for what, ends in bad.items():
        with pytest.raises(ValueError):
            _multi(K, lay, st, 1, lay.g[0], "ema", ends=ends)
    with pytest.raises(ValueError):           # count = 65
        K.adamw_multi(st["p"][:65 * UNIT], lay.g[0][:65 * UNIT], st["m"][:65 * UNIT], st["v"][:65 * UNIT],
                      [UNIT * (i + 1) for i in range(65)], [1e-3] * 65, [0.0] * 65, B1, B2, EPS, 1)
    with pytest.raises(ValueError):           # a pointer that is not 16-byte aligned
        K.adamw_multi(st["p"][1:][:UNIT], lay.g[0][:UNIT], st["m"][:UNIT], st["v"][:UNIT], [UNIT], [1e-3], [0.0],
                      B1, B2, EPS, 1)
    # the library itself refuses the same tables, before it launches anything
    A = favit._abi
    lib, P = A.lib(), lambda t: t.data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def desc(ends, count=None):
        d = A.AdamwMulti()
        d.p, d.g, d.m, d.v, d.p_bf16, d.ema = P(st["p"]), P(lay.g[0]), P(st["m"]), P(st["v"]), P(st["lp"]), P(st["ema"])
        d.n, d.count = n, len(ends) if count is None else count
        for s, e in enumerate(ends[:A.ADAMW_MAX_SEGMENTS]):
            d.end[s], d.lr[s], d.weight_decay[s] = e, 1e-3, 0.05
        d.beta1, d.beta2, d.eps, d.bias_c1, d.bias_c2, d.grad_scale, d.ema_decay = B1, B2, EPS, 1 - B1, 1 - B2, 1.0, 0.9
        return d
    for what, ends in bad.items():
        assert lib.favit_adamw_multi(ctypes.byref(desc(ends)), stream) == A.ERR_INVALID, what
    for count in (0, 65):
        assert lib.favit_adamw_multi(ctypes.byref(desc(lay.ends, count)), stream) == A.ERR_INVALID, f"count = {count}"
    for field, off in (("p", 4), ("ema", 8), ("p_bf16", 4)):
        d = desc(lay.ends)
        setattr(d, field, getattr(d, field) + off)
        assert lib.favit_adamw_multi(ctypes.byref(d), stream) == A.ERR_INVALID, f"misaligned {field}"
    d = desc(lay.ends)
    d.v = None
    assert lib.favit_adamw_multi(ctypes.byref(d), stream) == A.ERR_INVALID, "null v"
    torch.cuda.synchronize()
    for k, t in st.items():
        assert torch.equal(_bits(t), before[k]), f"a refused call wrote {k}"
    assert lib.favit_adamw_multi(ctypes.byref(desc(lay.ends)), stream) == 0          # and the good table is taken
    torch.cuda.synchronize()
    assert not torch.equal(_bits(st["p"]), before["p"])


# ----------------------------------------------------------------------------------------------------------------
def _vit(favit, seed=11):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                       num_heads=4, use_mhla=True).to(DEV).train()


def _recipe(favit, model, lr=1e-4, head_lr=1e-3, d=0.75):
    """The fine-tuning groups at the recipe's own rates (tools/run_experiment.py's defaults).  The float64 comparisons
    below are made at these rates on purpose: the single-group kernel, whose bits the segmented one must have, forms
    1 - beta2 in fp32 (0.99900001 -> 1.00005e-3, 4.7e-5 off), i.e. it errs by ~2.4e-5 of every UPDATE; relative to the
    weights that is 2.4e-5 * 3 lr / |w|, far below the 1e-6 bound at these rates and above it from lr ~ 1e-2 on.  What
    the bound must catch stays far above it: a group stepping at its neighbour's rate (0.75 x) is off by 0.25 * 3 lr
    ~ 1e-4 against weights of ~2e-2, a decay applied to an exempt tensor by 3 * lr * 0.05 = 1.5e-5 of it."""
    return favit.train.param_groups(model, lr=lr, head_lr=head_lr, layer_decay=d, no_weight_decay="auto")


def _inject(models, seed, scale=1.0):
    """The same seeded gradient into every model's .grad, per parameter name."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    grads = {n: torch.randn(p.shape, device=DEV, generator=g) * scale for n, p in models[0].named_parameters()}
    for m in models:
        for n, p in m.named_parameters():
            p.grad.copy_(grads[n])
    return grads


def _torch64(model, groups, weight_decay):
    """torch.optim.AdamW in float64 on the CPU over the same groups; returns (optimizer, {name: parameter})."""
    names = {id(p): n for n, p in model.named_parameters()}
    ref = {n: torch.nn.Parameter(p.detach().double().cpu()) for n, p in model.named_parameters()}
    opt = torch.optim.AdamW([{"params": [ref[names[id(p)]] for p in g["params"]], "lr": g["lr"],
                              "weight_decay": g.get("weight_decay", weight_decay)} for g in groups],
                            lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=weight_decay)
    return opt, ref


def _mirror_of(opt, p):
    for g in opt.groups:
        for q, o in zip(g["flat"].params, g["flat"].offsets):
            if q is p:
                return g["lp"][o:o + p.numel()]
    raise KeyError


def test_fused_optimizer_has_the_bits_of_the_per_group_one(favit):
    T = favit.train
    try:
        m1, m2 = _vit(favit), _vit(favit)
        g1, g2 = _recipe(favit, m1), _recipe(favit, m2)
        assert len(g1) > 3
        ref_opt, ref = _torch64(m2, g2, 0.05)
        per = T.FusedAdamW(g1, lr=1e-4, weight_decay=0.05, distributed=False, ema_decay=0.9)
        fused = T.FusedAdamW(g2, lr=1e-4, weight_decay=0.05, distributed=False, ema_decay=0.9, fuse_groups=True)
        assert all(g["sync"] is None for g in fused.groups)
        assert [g["mirror"] is not None for g in fused.groups] == [True] + [False] * (len(g2) - 1)
        for step in range(3):
            per.zero_grad()
            fused.zero_grad()
            grads = _inject([m1, m2], 100 + step)
            per.step()
            fused.step()
            for n, r in ref.items():
                r.grad = grads[n].double().cpu()
            ref_opt.step()
        e1, e2 = per.ema_state_dict(m1), fused.ema_state_dict(m2)
        for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(_bits(p), _bits(q)), n
            assert torch.equal(_bits(_mirror_of(per, p)), _bits(_mirror_of(fused, q))), n
            assert torch.equal(_bits(_mirror_of(fused, q)), _bits(q.detach().flatten().to(torch.bfloat16))), n
            assert torch.equal(_bits(e1[n]), _bits(e2[n])), n
        got = torch.cat([p.detach().flatten() for p in m2.parameters()])
        want = torch.cat([ref[n].detach().flatten() for n, _ in m2.named_parameters()])
        print(f"fused AdamW, 3 steps, {len(g2)} groups: parameters rel-L2 to float64 torch {rel_l2(got, want):.3e}")
        assert rel_l2(got, want) < 1e-6
        # the padding between the groups is still zero everywhere
        a = fused._arena
        used = torch.zeros(a["p"].numel(), dtype=torch.bool, device=DEV)
        for g, s in zip(fused.groups, fused._starts):
            for p, o in zip(g["flat"].params, g["flat"].offsets):
                used[s + o:s + o + p.numel()] = True
        for k in ("p", "g", "m", "v", "ema"):
            assert not bool(a[k][~used].any()), k
    finally:
        favit.functional.clear_lp_mirrors()


def test_more_groups_than_one_launch_takes(favit):
    """70 one-tensor groups: two consecutive launches (64 + 6), the bits of 70 per-group launches."""
    T = favit.train
    try:
        def build():
            torch.manual_seed(4)
            ps = [torch.nn.Parameter(torch.randn(3 + 37 * i, device=DEV)) for i in range(70)]
            return ps, [{"params": [p], "lr": 1e-3 * (1 + i % 7), "weight_decay": 0.01 * (i % 3)} for i, p in enumerate(ps)]
        (p1, g1), (p2, g2) = build(), build()
        per = T.FusedAdamW(g1, distributed=False)
        fused = T.FusedAdamW(g2, distributed=False, fuse_groups=True)
        assert [(i, j) for i, j, _, _ in fused._launches] == [(0, 64), (64, 70)]
        health = T.Health()
        try:
            for step in range(2):
                gen = torch.Generator(device=DEV).manual_seed(step)
                for a, b in zip(p1, p2):
                    a.grad.copy_(torch.randn(a.shape, device=DEV, generator=gen))
                    b.grad.copy_(a.grad)
                count = int(health.words[3])
                fused.step()
                assert int(health.words[3]) - count == 2, "two launches per step"
                per.step()
        finally:
            health.close()
        for a, b in zip(p1, p2):
            assert torch.equal(_bits(a), _bits(b))
    finally:
        favit.functional.clear_lp_mirrors()


def test_more_than_sixteen_groups_with_clipping(favit):
    T = favit.train
    try:
        def groups(m):
            return [{"params": [p], "lr": 1e-4 * (1 + i % 3), "weight_decay": 0.05 if p.ndim > 1 else 0.0}
                    for i, (n, p) in enumerate(m.named_parameters())]
        m1, m2 = _vit(favit), _vit(favit)
        assert len(groups(m1)) > 16
        with pytest.raises(ValueError, match="at most 16"):
            T.FusedAdamW(groups(m1), distributed=False, max_grad_norm=1.0)
        ref_opt, ref = _torch64(m2, groups(m2), 0.05)
        mx = 0.25 * float(torch.sqrt(torch.tensor(float(sum(p.numel() for p in m2.parameters())))))    # E|g|^2 = numel
        opt = T.FusedAdamW(groups(m2), distributed=False, max_grad_norm=mx, fuse_groups=True)
        for step, scale in enumerate((1.0, 0.5, 2.0)):
            opt.zero_grad()
            grads = _inject([m2], 200 + step, scale)
            opt.step()
            for n, r in ref.items():
                r.grad = grads[n].double().cpu()
            total = float(torch.nn.utils.clip_grad_norm_(list(ref.values()), mx))
            ref_opt.step()
            got = float(opt.grad_norm)
            print(f"step {step}: opt.grad_norm {got!r} float64 {total!r} rel {abs(got - total) / total:.3e} max_norm {mx!r}")
            assert abs(got - total) <= 1e-6 * total and total > mx, "clipping is active in every step"
        got = torch.cat([p.detach().flatten() for p in m2.parameters()])
        want = torch.cat([ref[n].detach().flatten() for n, _ in m2.named_parameters()])
        print(f"{len(opt.groups)} groups, clipped, 3 steps: parameters rel-L2 {rel_l2(got, want):.3e}")
        assert rel_l2(got, want) < 1e-6
        assert int(opt.skipped_steps) == 0
    finally:
        favit.functional.clear_lp_mirrors()


# ----------------------------------------------------------------------------------------------------------------
def _grad_norm64(model):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))


@pytest.fixture(scope="module")
def vit_case(favit):
    """Three batches and n0, the un-clipped gradient norm of the first one at initialisation (bf16 mode)."""
    g = torch.Generator(device=DEV).manual_seed(2)
    xs = [torch.randn(8, 3, 32, 32, device=DEV, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device=DEV, generator=g) for _ in range(3)]
    favit.set_compute_dtype("bf16")
    try:
        m = _vit(favit)
        favit.train.cross_entropy(m(xs[0]), ys[0]).backward()
        n0 = _grad_norm64(m)
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
    assert n0 > 0
    return xs, ys, n0


def test_fused_training_steps_match_torch(favit, vit_case):
    xs, ys, n0 = vit_case
    mx = n0 / 4
    T = favit.train
    favit.set_compute_dtype("bf16")
    try:
        m1 = _vit(favit)
        o1 = T.FusedAdamW(_recipe(favit, m1, 1e-3, 1e-3), lr=1e-3, weight_decay=0.05, distributed=False, max_grad_norm=mx,
                          fuse_groups=True)
        norms = []
        for x, y in zip(xs, ys):
            T.train_step(m1, x, y, o1)
            norms.append(o1.grad_norm.clone())
        m2 = _vit(favit)
        o2, ref = _torch64(m2, _recipe(favit, m2, 1e-3, 1e-3), 0.05)
        for x, y in zip(xs, ys):
            m2.zero_grad(set_to_none=True)
            T.cross_entropy(m2(x), y).backward()
            for n, p in m2.named_parameters():
                ref[n].grad = p.grad.double().cpu() if p.grad is not None else torch.zeros_like(ref[n])
            torch.nn.utils.clip_grad_norm_(list(ref.values()), mx)
            o2.step()
            with torch.no_grad():
                for n, p in m2.named_parameters():
                    p.copy_(ref[n].detach().float())
        norms = [float(n) for n in norms]
        assert all(n > mx for n in norms), "clipping was active at every step"
        assert abs(norms[0] - n0) <= 1e-5 * n0 and int(o1.skipped_steps) == 0
        w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
        w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        print(f"weights rel-L2 after three clipped fused steps: {rel_l2(w1, w2):.3e}")
        assert rel_l2(w1, w2) < 1e-3
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_graphed_step_and_schedule_on_a_fused_optimizer(favit, vit_case):
    xs, ys, n0 = vit_case
    xs, ys = xs + xs[:1], ys + ys[:1]
    T = favit.train
    favit.set_compute_dtype("bf16")

    def build():
        m = _vit(favit)
        o = T.FusedAdamW(_recipe(favit, m, 1e-3, 1e-3), lr=1e-3, weight_decay=0.05, distributed=False,
                         max_grad_norm=n0 / 4, skip_nonfinite=True, fuse_groups=True)
        # factor 1, 1, 0.5, 0 at steps 0..3: the last update runs at rate 0
        return m, o, T.WarmupCosine(o, 1, 3)
    try:
        m1, o1, s1 = build()
        eager = []
        for x, y in zip(xs, ys):
            eager.append(T.train_step(m1, x, y, o1).item())
            s1.step()
        m2, o2, s2 = build()
        step = T.GraphedStep(m2, o2, xs[0], ys[0])
        graphed, moved, before = [], [], None
        for x, y in zip(xs, ys):
            before = torch.cat([p.detach().flatten() for p in m2.parameters()]).clone()
            graphed.append(step(x, y).item())
            moved.append(float((torch.cat([p.detach().flatten() for p in m2.parameters()]) - before).norm()))
            s2.step()
        for a, b in zip(eager, graphed):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (eager, graphed)
        w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
        w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        assert rel_l2(w2.cpu(), w1.cpu()) < 1e-3
        assert int(o1.skipped_steps) == 0 and int(o2.skipped_steps) == 0
        print(f"update sizes per step {moved}")
        # the rates are by-value arguments of the eager launch: every replayed step runs at the schedule's CURRENT rate.
        # Rate 0 in the fourth step: step = 0 and decay = 1, so that update is exactly nothing.
        assert moved[0] > 0 and moved[1] > 0 and moved[2] > 0 and moved[3] == 0.0
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_checkpoint_moves_between_fused_and_per_group(favit, tmp_path):
    T = favit.train
    try:
        def trained(fuse, seed):
            m = _vit(favit, seed)
            o = T.FusedAdamW(_recipe(favit, m), lr=1e-2, weight_decay=0.05, distributed=False, ema_decay=0.9,
                             fuse_groups=fuse)
            for step in range(2):
                o.zero_grad()
                _inject([m], 300 + step)
                o.step()
            return m, o
        for fuse in (True, False):
            m1, o1 = trained(fuse, 11)
            path = str(tmp_path / f"ck{int(fuse)}.pt")
            T.save_checkpoint(path, m1, o1)
            m2 = _vit(favit, 12)
            o2 = T.FusedAdamW(_recipe(favit, m2), lr=1e-2, weight_decay=0.05, distributed=False, ema_decay=0.9,
                              fuse_groups=not fuse)
            T.load_checkpoint(path, m2, o2)
            s1, s2 = o1.state_dict(m1), o2.state_dict(m2)
            assert s2["steps"] == 2 and s2["ema_updates"] == 2 and s1["groups"] == s2["groups"]
            for n, p in m1.named_parameters():
                for key in ("m", "v", "ema"):
                    assert torch.equal(_bits(s1["state"][n][key]), _bits(s2["state"][n][key])), (n, key)
                assert s1["state"][n]["m"].abs().sum() > 0
            # and both continue alike from there
            for o, m in ((o1, m1), (o2, m2)):
                o.zero_grad()
            _inject([m1, m2], 310)
            o1.step()
            o2.step()
            for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
                assert torch.equal(_bits(p), _bits(q)), n
    finally:
        favit.functional.clear_lp_mirrors()


def test_ema_weights_swap_once_and_restore(favit):
    T = favit.train
    try:
        m = _vit(favit)
        o = T.FusedAdamW(_recipe(favit, m), lr=1e-2, weight_decay=0.05, distributed=False, ema_decay=0.5, fuse_groups=True)
        for step in range(2):
            o.zero_grad()
            _inject([m], 400 + step)
            o.step()
        train_w = {n: _bits(p) for n, p in m.named_parameters()}
        avg = {n: _bits(t) for n, t in o.ema_state_dict(m).items()}
        lp = _bits(o._arena["lp"])
        with o.ema_weights():
            for n, p in m.named_parameters():
                assert torch.equal(_bits(p), avg[n]) and not torch.equal(_bits(p), train_w[n]), n
            assert torch.equal(_bits(o._arena["lp"]), _bits(o._arena["p"].to(torch.bfloat16)))
            assert all(torch.equal(_bits(t), avg[n]) for n, t in o.ema_state_dict(m).items())
            with pytest.raises(RuntimeError):
                o.step()
        for n, p in m.named_parameters():
            assert torch.equal(_bits(p), train_w[n]), n
        assert torch.equal(_bits(o._arena["lp"]), lp)
        assert all(torch.equal(_bits(t), avg[n]) for n, t in o.ema_state_dict(m).items())
    finally:
        favit.functional.clear_lp_mirrors()


def test_health_report_names_the_parameter_in_a_fused_optimizer(favit):
    T = favit.train
    try:
        m = _vit(favit)
        o = T.FusedAdamW(_recipe(favit, m), lr=1e-2, distributed=False, fuse_groups=True)
        health = T.Health()
        try:
            o.zero_grad()
            _inject([m], 500)
            m.blocks[1].mlp.fc1.weight.grad[3, 5] = float("inf")
            o.step()
            rep = health.report(o, m)
            assert rep is not None and "gradient" in rep["non_finite"] and rep["adamw_launches"] == 1
            assert any(t["buffer"] == "flat_g" and t["parameter"] == "blocks.1.mlp.fc1.weight" for t in rep["tensors"])
        finally:
            health.close()
    finally:
        favit.functional.clear_lp_mirrors()


# ----------------------------------------------------------------------------------------------------------------
def _dp_model(pkg):
    torch.manual_seed(3)
    return pkg.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                     num_heads=4, window_size=7, use_mhla=True).cuda().train()


def _dp_batch():
    g = torch.Generator().manual_seed(5)
    return torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)


def _dp_worker(rank, world, port, out, max_norm):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = importlib.import_module("focused-attention-vit_amd")
    pkg.set_compute_dtype("fp32")
    m = _dp_model(pkg)
    groups = pkg.train.param_groups(m, lr=1e-2, layer_decay=0.75, no_weight_decay="auto")
    opt = pkg.train.FusedAdamW(groups, lr=1e-2, weight_decay=0.05, bucket_mb=0.05, max_grad_norm=max_norm, fuse_groups=True)
    syncs = [g["sync"] for g in opt.groups]
    x, y = _dp_batch()
    lo = rank * 4
    xs, ys = x[lo:lo + 4].cuda(), y[lo:lo + 4].cuda()
    norms = []
    for _ in range(2):
        pkg.train.train_step(m, xs, ys, opt)
        norms.append(opt.grad_norm.clone())
    torch.cuda.synchronize()
    w = torch.cat([p.detach().flatten().cpu() for p in m.parameters()])
    torch.save({"w": w, "norms": [float(n) for n in norms], "skipped": int(opt.skipped_steps), "groups": len(groups),
                "syncs": [s is not None for s in syncs], "buckets": len(syncs[0].buckets)}, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_dp_two_ranks_share_one_gradient_sync(favit, tmp_path):
    favit.set_compute_dtype("fp32")
    try:
        m = _dp_model(favit)
        x, y = _dp_batch()
        favit.train.cross_entropy(m(x.cuda()), y.cuda()).backward()
        n_ref = _grad_norm64(m)
    finally:
        favit.functional.clear_lp_mirrors()
    out = str(tmp_path / "dpfused")
    mp.spawn(_dp_worker, args=(2, 40500 + (os.getpid() % 2000), out, n_ref / 4), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=True), torch.load(out + ".1", weights_only=True)
    print(f"whole-batch norm {n_ref!r}; rank norms {r0['norms']} {r1['norms']}; {r0['groups']} groups, {r0['buckets']} buckets")
    for r in (r0, r1):
        assert r["groups"] > 3 and r["syncs"] == [True] + [False] * (r["groups"] - 1)
        assert r["buckets"] > 1
        assert abs(r["norms"][0] - n_ref) <= 2e-5 * n_ref
        assert r["norms"][0] > n_ref / 4 and r["skipped"] == 0
    assert r0["norms"] == r1["norms"], "both ranks reduce the same all-reduced gradient in the same order"
    assert torch.equal(r0["w"], r1["w"]), "the two ranks diverged"
