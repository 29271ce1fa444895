"""GPU tests of the weight EMA fused into AdamW (favit_adamw_ema / favit_adamw_clip_ema), of favit_swap_params, and of
their way up through train.FusedAdamW (ema_weights, ema_state_dict), train.GraphedStep, the resumable checkpoint and
harness.fit.  Bitwise claims are asserted on bits; the one accuracy bound (the EMA update against float64) is derived
where it is used."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENS = [1, 63, 64, 65, 255, 257, 1023, 10007, 300001, 0]
ADAM = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.05)
LRS = (1e-3, 5e-3)


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


def _bits(t):
    return t.detach().cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).clone()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _odd(i, values):
    """A copy of `values` whose start is one float past a 16-byte boundary for odd i (a scalar head in front of any
    vector body), on a boundary for even i."""
    off = i % 2
    t = torch.empty(values.numel() + off, dtype=values.dtype, device=DEV)[off:]
    t.copy_(values)
    assert values.numel() == 0 or values.dtype != torch.float32 or (t.data_ptr() % 16 != 0) == (off == 1)
    return t


@pytest.fixture(scope="module")
def bufs():
    """Gradients of two steps and a start state per length (never written: every test copies)."""
    g = torch.Generator(device=DEV).manual_seed(7)
    mk = lambda n, s=1.0: torch.randn(n, device=DEV, generator=g) * s
    return {"g": [[mk(n, 2.0) for n in LENS] for _ in range(2)], "p": [mk(n) for n in LENS],
            "e": [mk(n) for n in LENS], "m": [mk(n, 0.1) for n in LENS], "v": [mk(n, 0.1) ** 2 for n in LENS]}


def _state(bufs):
    return {k: [_odd(i, t) for i, t in enumerate(bufs[k])] for k in ("p", "e", "m", "v")} | \
           {"lp": [_odd(i, t.to(torch.bfloat16)) for i, t in enumerate(bufs["p"])]}


def _launch(K, s, i, g, step, coef=None, skip=False, ema=False, d=0.0):
    kw = {} if coef is None else dict(coef=coef, skip_nonfinite=skip)
    if ema:
        kw.update(ema=s["e"][i], ema_decay=d)
    elif coef is None and s["p"][i].numel() == 0:
        return                                   # (favit_adamw refuses the null pointer of an empty tensor)
    K.adamw(s["p"][i], g, s["m"][i], s["v"][i], LRS[i % 2], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], step,
            p_lp=s["lp"][i], **kw)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("d", [0.5, 0.9, 0.999])
def test_adamw_ema_kernel(K, bufs, d, clip):
    coef = torch.tensor([0.37], device=DEV) if clip else None
    a, b = _state(bufs), _state(bufs)            # a: with the average, b: the entry point without it
    d32 = float(torch.tensor(d, dtype=torch.float32))
    omd = 1.0 - d32                              # exact in fp32 for d in [0.5, 1]: the kernel's 1.0f - d is this number
    assert float(torch.tensor(omd, dtype=torch.float32)) == omd
    worst = 0.0
    for step in (1, 2):
        for i in range(len(LENS)):
            g = _odd(i, bufs["g"][step - 1][i])
            e_old = a["e"][i].double()
            _launch(K, a, i, g, step, coef=coef, ema=True, d=d)
            _launch(K, b, i, g, step, coef=coef)
            for key in ("p", "m", "v", "lp"):
                assert _same(a[key][i], b[key][i]), (key, LENS[i], step)
            p_new = a["p"][i].double()
            e64 = d32 * e_old + omd * p_new
            # one rounding of the product (1 - d) * p and one of the fused multiply-add, each at most 2^-24 of a
            # quantity bounded by |e_old| + |p_new|
            bound = 2.0 ** -23 * (e_old.abs() + p_new.abs())
            err = (a["e"][i].double() - e64).abs()
            assert bool((err <= bound).all()), (LENS[i], step, float((err - bound).max()))
            if err.numel():
                worst = max(worst, float((err / bound).max()))
            assert _same(b["e"][i], bufs["e"][i]), "the entry point without the average never touches it"
    print(f"d={d} clip={clip}: worst |e - e64| / bound = {worst:.3f}")
    for i, n in enumerate(LENS):                 # the launches really updated something
        assert n == 0 or not _same(a["e"][i], bufs["e"][i])


def test_adamw_ema_decay_zero_copies_and_skip_leaves_untouched(K, bufs):
    a = _state(bufs)
    for i in range(len(LENS)):
        _launch(K, a, i, _odd(i, bufs["g"][0][i]), 1, ema=True, d=0.0)
        assert _same(a["e"][i], a["p"][i]), LENS[i]
    # skip_nonfinite and a NaN coefficient: nothing is stored, the average included
    a = _state(bufs)
    nan = torch.full((1,), float("nan"), device=DEV)
    for i in range(len(LENS)):
        _launch(K, a, i, _odd(i, bufs["g"][0][i]), 1, coef=nan, skip=True, ema=True, d=0.9)
        assert _same(a["e"][i], bufs["e"][i]) and _same(a["p"][i], bufs["p"][i]) and _same(a["m"][i], bufs["m"][i])
    # without the skip the NaN reaches the average like the parameters
    _launch(K, a, 3, _odd(3, bufs["g"][0][3]), 1, coef=nan, skip=False, ema=True, d=0.9)
    assert bool(torch.isnan(a["e"][3]).all()) and bool(torch.isnan(a["p"][3]).all())
    with pytest.raises(ValueError):
        K.adamw(a["p"][1], bufs["g"][0][1], a["m"][1], a["v"][1], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, ema=a["e"][1], ema_decay=1.5)
    with pytest.raises(TypeError):
        K.adamw(a["p"][1], bufs["g"][0][1], a["m"][1], a["v"][1], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, ema=a["e"][2], ema_decay=0.5)


def test_swap_params_kernel(K, bufs):
    for i, n in enumerate(LENS):
        a0, b0 = bufs["p"][i], bufs["e"][i]
        a, b = _odd(i, a0), _odd(i + 1, b0)      # the two buffers in different alignment classes
        lp = _odd(i, torch.zeros(n, dtype=torch.bfloat16, device=DEV))
        K.swap_params(a, b, lp)
        assert _same(a, b0) and _same(b, a0) and _same(lp, b0.to(torch.bfloat16)), n
        K.swap_params(a, b, lp)
        assert _same(a, a0) and _same(b, b0) and _same(lp, a0.to(torch.bfloat16)), n
        K.swap_params(a, b)                      # a null mirror pointer
        assert _same(a, b0) and _same(b, a0) and _same(lp, a0.to(torch.bfloat16)), n
    with pytest.raises(TypeError):
        K.swap_params(bufs["p"][1].clone(), bufs["e"][2].clone())


# ----------------------------------------------------------------------------------------------------------------
def _vit(favit, seed=11, **kw):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                       num_heads=4, use_mhla=True, **kw).to(DEV).train()


@pytest.fixture(scope="module")
def batches3():
    g = torch.Generator(device=DEV).manual_seed(2)
    xs = [torch.randn(8, 3, 32, 32, device=DEV, generator=g) for _ in range(3)]
    ys = [torch.randint(0, 10, (8,), device=DEV, generator=g) for _ in range(3)]
    return xs, ys


def _opt(favit, model, **kw):
    T = favit.train
    return T.FusedAdamW(T.param_groups(model, lr=1e-3), lr=1e-3, weight_decay=0.05, distributed=False, **kw)


def test_optimizer_ema_follows_the_recurrence(favit, batches3):
    xs, ys = batches3
    T = favit.train
    favit.set_compute_dtype("bf16")
    try:
        m = _vit(favit)
        opt = _opt(favit, m, ema_decay=0.99, ema_warmup=True)
        assert all(_same(g["ema"], g["flat"].flat_p) for g in opt.groups)
        ref = [g["ema"].double() for g in opt.groups]
        tol = [torch.zeros_like(r) for r in ref]
        f32 = torch.float32
        for k in range(5):
            e_old = [g["ema"].double().abs() for g in opt.groups]
            T.train_step(m, xs[k % 3], ys[k % 3], opt)
            d = torch.tensor(T.ema_decay_at(0.99, k, True), dtype=f32)          # what the launch received, and the
            omd = torch.tensor(1.0, dtype=f32) - d                             # kernel's own fp32 (1 - d)
            for gi, g in enumerate(opt.groups):
                p = g["flat"].flat_p.double()                                   # THIS run's parameters after step k
                ref[gi] = float(d) * ref[gi] + float(omd) * p
                tol[gi] += 2.0 ** -23 * (e_old[gi] + p.abs())                   # the kernel test's bound, summed
        assert opt.ema_updates == 5 and opt.steps == 5
        for gi, g in enumerate(opt.groups):
            err = (g["ema"].double() - ref[gi]).abs()
            print(f"group {gi}: max |ema - float64 recurrence| {float(err.max()):.3e}, bound there "
                  f"{float(tol[gi].flatten()[err.argmax()]):.3e}")
            assert bool((err <= tol[gi]).all())
            assert not _same(g["ema"], g["flat"].flat_p)
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_ema_weights_context(favit, batches3):
    xs, ys = batches3
    T = favit.train
    favit.set_compute_dtype("bf16")
    try:
        m = _vit(favit)
        opt = _opt(favit, m, ema_decay=0.9)
        for x, y in zip(xs, ys):
            T.train_step(m, x, y, opt)
        snap = lambda: [[_bits(g[k]) if k != "p" else _bits(g["flat"].flat_p) for g in opt.groups] for k in ("p", "ema", "lp")]
        p0, e0, lp0 = snap()

        def restored():
            p1, e1, lp1 = snap()
            return all(torch.equal(a, b) for xs_, ys_ in ((p0, p1), (e0, e1), (lp0, lp1)) for a, b in zip(xs_, ys_))

        with opt.ema_weights():
            for gi, g in enumerate(opt.groups):
                assert torch.equal(_bits(g["flat"].flat_p), e0[gi]) and torch.equal(_bits(g["ema"]), p0[gi])
                assert torch.equal(_bits(g["lp"]), _bits(g["flat"].flat_p.to(torch.bfloat16)))
            with torch.no_grad():
                y_in = m.eval()(xs[0])
            inside = opt.ema_state_dict(m)
            with pytest.raises(RuntimeError, match="nest"):
                with opt.ema_weights():
                    pass
            with pytest.raises(RuntimeError, match="step"):
                opt.step()
        m.train()
        assert restored() and opt.steps == 3 and opt.ema_updates == 3
        sd = opt.ema_state_dict(m)
        assert list(sd.keys()) == list(m.state_dict().keys())
        assert all(_same(sd[k], inside[k]) for k in sd), "the same average from inside and outside the context"
        fresh = _vit(favit, seed=5)
        fresh.load_state_dict(sd)
        with torch.no_grad():
            y_ref = fresh.eval()(xs[0])
            y_train_weights = m.eval()(xs[0])
        m.train()
        assert _same(y_in, y_ref)
        assert not _same(y_in, y_train_weights), "the average differs from the training weights"
        with pytest.raises(KeyError):
            with opt.ema_weights():
                raise KeyError("inside")
        assert restored()
        with opt.ema_weights():                  # and the context is usable again
            pass
        assert restored()
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_graphed_step_survives_an_ema_evaluation(favit, batches3):
    xs, ys = batches3
    T = favit.train
    favit.set_compute_dtype("bf16")

    def run(evaluate):
        m = _vit(favit)
        opt = _opt(favit, m, ema_decay=0.9, max_grad_norm=1.0, skip_nonfinite=True)
        step = T.GraphedStep(m, opt, xs[0], ys[0])
        losses = [step(xs[k % 3], ys[k % 3]).item() for k in range(2)]
        if evaluate:
            with opt.ema_weights(), torch.no_grad():
                m.eval()(xs[0])
            m.train()
        losses += [step(xs[k % 3], ys[k % 3]).item() for k in range(2, 4)]
        return losses, torch.cat([g["flat"].flat_p for g in opt.groups]).cpu(), torch.cat([g["ema"] for g in opt.groups]).cpu()
    try:
        la, pa, ea = run(True)
        lb, pb, eb = run(False)
        print(f"losses with the evaluation {la}, without {lb}; parameters rel-L2 {rel_l2(pa, pb):.3e}, ema {rel_l2(ea, eb):.3e}")
        for a, b in zip(la, lb):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a))
        assert rel_l2(pa, pb) < 2e-3 and rel_l2(ea, eb) < 2e-3
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_resume_is_bitwise_for_optimizer_state(favit, tmp_path):
    """Only the norm, AdamW and EMA kernels run (synthetic gradients), none of which uses atomics: bits are asserted.
    The norm's summation order depends on each buffer's alignment; the fresh flat buffers of the second set of objects
    come from the caching allocator, at least 512-byte aligned like the first ones, so the bits agree."""
    T = favit.train

    def build(seed):
        m = _vit(favit, seed)
        opt = _opt(favit, m, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99, ema_warmup=True)
        return m, opt, T.WarmupCosine(opt, 2, 6, min_ratio=0.1)

    def steps(opt, sched, ks):
        for k in ks:
            g_ = torch.Generator(device=DEV).manual_seed(100 + k)
            opt.zero_grad()
            for g in opt.groups:                 # through the .grad views: the padding between two parameters stays
                for p in g["flat"].params:       # zero, as after a backward (a checkpoint holds parameters, not padding)
                    p.grad.copy_(torch.randn(p.shape, device=DEV, generator=g_) * 1e-2)
            opt.step()
            sched.step()
            assert float(opt.grad_norm) > 1.0, "clipping is active"

    def state(opt):
        out = []
        for g in opt.groups:
            assert g["flat"].flat_p.data_ptr() % 512 == 0 and g["flat"].flat_g.data_ptr() % 512 == 0
            out += [_bits(g["flat"].flat_p), _bits(g["m"]), _bits(g["v"]), _bits(g["ema"]), _bits(g["lp"])]
        return out, (opt.steps, opt.ema_updates, int(opt.skipped_steps), [g["lr"] for g in opt.groups])
    try:
        m1, o1, s1 = build(11)
        steps(o1, s1, range(6))
        want_bits, want_host = state(o1)

        m2, o2, s2 = build(11)
        steps(o2, s2, range(3))
        path = str(tmp_path / "resume.pt")
        T.save_checkpoint(path, m2, o2, s2)
        ck = torch.load(path, map_location="cpu", weights_only=True)
        assert ck["optimizer"]["ema_updates"] == 3 and "ema" in ck["optimizer"]["state"]["head.weight"]
        m3, o3, s3 = build(29)
        assert not _same(m3.head.weight, m2.head.weight)
        T.load_checkpoint(path, m3, o3, s3)
        steps(o3, s3, range(3, 6))
        got_bits, got_host = state(o3)
        assert got_host == want_host
        assert all(torch.equal(a, b) for a, b in zip(got_bits, want_bits))
        for g in o3.groups:                      # load_state_dict left a mirror that matches the loaded weights
            assert _same(g["lp"], g["flat"].flat_p.to(torch.bfloat16))

        # the averaged weights alone, into a model without an optimizer
        m4 = _vit(favit, 31)
        T.load_checkpoint(path, m4, use_ema=True)
        ema3 = {k: v for k, v in ck["optimizer"]["state"].items()}
        assert all(torch.equal(p.detach().cpu(), ema3[n]["ema"]) for n, p in m4.named_parameters())
        # a file without an average is refused by an optimizer that keeps one, before anything is written
        for st in ck["optimizer"]["state"].values():
            del st["ema"]
        torch.save(ck, path)
        before, _ = state(o3)
        with pytest.raises(ValueError, match="ema"):
            T.load_checkpoint(path, m3, o3, s3)
        assert all(torch.equal(a, b) for a, b in zip(state(o3)[0], before))
    finally:
        favit.functional.clear_lp_mirrors()


def test_dropout_continues_after_a_resume(favit, tmp_path, batches3):
    xs, _ = batches3
    T, F = favit.train, favit.functional
    favit.set_compute_dtype("fp32")
    word = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    F.set_dropout_epoch(word)
    try:
        m1 = _vit(favit, 11, dropout=0.1)
        with torch.no_grad():
            y0 = m1(xs[0])
            path = str(tmp_path / "drop.pt")
            T.save_checkpoint(path, m1)
            y1 = m1(xs[0])                       # the uninterrupted run's next forward
        assert not _same(y0, y1), "dropout draws new masks per forward"
        m2 = _vit(favit, 23, dropout=0.1)        # (seeds the CPU generator differently on the way)
        word.fill_(1234)
        T.load_checkpoint(path, m2)
        assert int(word) == 5 and F.get_dropout_epoch() is word, "restored in place"
        with torch.no_grad():
            y1b = m2(xs[0])
        assert _same(y1, y1b)
        # no word registered in the resuming process: one is registered with the file's value
        F.set_dropout_epoch(None)
        m3 = _vit(favit, 37, dropout=0.1)
        T.load_checkpoint(path, m3)
        assert F.get_dropout_epoch() is not None and int(F.get_dropout_epoch()) == 5
        with torch.no_grad():
            assert _same(m3(xs[0]), y1)
    finally:
        F.set_dropout_epoch(None)
        favit.functional.clear_lp_mirrors()


# ----------------------------------------------------------------------------------------------------------------
class _Recording:
    """A train loader that notes the labels of every epoch it serves; its state is the wrapped loader's."""

    def __init__(self, inner, log):
        self.inner, self.log = inner, log

    def __iter__(self):
        ep = []
        self.log.append(ep)
        for x, y in self.inner:
            ep.append(y.cpu().tolist())
            yield x, y

    def __len__(self):
        return len(self.inner)

    def state_dict(self):
        return self.inner.state_dict()

    def check_state_dict(self, s):
        self.inner.check_state_dict(s)

    def load_state_dict(self, s):
        self.inner.load_state_dict(s)


def test_fit_resumes_from_a_checkpoint(favit, tmp_path):
    T, D, DS, H = favit.train, favit.data, favit.datasets, favit.harness
    rs = np.random.RandomState(0)
    rec = rs.randint(0, 256, size=(64, 1 + 3 * 32 * 32)).astype(np.uint8)
    rec[:, 0] = np.arange(64) % 10
    rec.tofile(str(tmp_path / "test_batch.bin"))
    ds = DS.Cifar10Binary(str(tmp_path), train=False)
    favit.set_compute_dtype("bf16")

    def build(model_seed, tf_seed):
        m = _vit(favit, model_seed)
        opt = _opt(favit, m, ema_decay=0.9, ema_warmup=True, max_grad_norm=1.0)
        sched = T.WarmupCosine(opt, 4, 32)
        log = []
        tr = _Recording(D.DeviceLoader(DS.batches(ds, 8, True, seed=3),
                                       D.DeviceTransform("cifar10_train", 32, D.CIFAR10_MEAN, D.CIFAR10_STD, seed=tf_seed)), log)
        va = D.DeviceLoader(DS.batches(ds, 16, False, seed=3), D.DeviceTransform("resize", 32, D.CIFAR10_MEAN, D.CIFAR10_STD))
        return m, opt, sched, tr, va, log

    quiet = lambda s: None
    try:
        m, opt, sched, tr, va, log_a = build(11, 1)
        a = H.fit(m, tr, va, opt, 4, log=quiet, schedule=sched, eval_ema=True)
        # eval_ema leaves the training weights in place: one more "epoch" without a batch, validation only
        before = [_bits(g["flat"].flat_p) for g in opt.groups], [_bits(g["ema"]) for g in opt.groups]
        H.fit(m, [], va, opt, 1, log=quiet, eval_ema=True)
        after = [_bits(g["flat"].flat_p) for g in opt.groups], [_bits(g["ema"]) for g in opt.groups]
        assert all(torch.equal(x, y) for xs_, ys_ in zip(before, after) for x, y in zip(xs_, ys_))

        path = str(tmp_path / "fit.pt")
        m, opt, sched, tr, va, log_b = build(11, 1)
        b2 = H.fit(m, tr, va, opt, 2, log=quiet, schedule=sched, eval_ema=True, checkpoint=path, checkpoint_every=2)
        assert len(b2["history"]["val_loss"]) == 2 and os.path.exists(path)
        m, opt, sched, tr, va, log_c = build(29, 77)                 # every object anew, otherwise seeded
        b = H.fit(m, tr, va, opt, 4, log=quiet, schedule=sched, eval_ema=True, checkpoint=path, resume=True)
        for k in ("train_loss", "train_acc", "val_loss", "val_acc", "epoch_time", "grad_norm"):
            assert len(a["history"][k]) == 4 and len(b["history"][k]) == 4, k
        assert b["history"]["val_loss"][:2] == b2["history"]["val_loss"], "the history is extended, not restarted"
        assert len(log_a) == 4 and log_b + log_c == log_a, "the label order of every epoch"
        assert opt.steps == 32 and sched.t == 32
        va_, vb_ = a["final_val_loss"], b["final_val_loss"]
        print(f"final val_loss straight {va_!r}, resumed {vb_!r}, rel {abs(va_ - vb_) / abs(va_):.3e}")
        assert abs(va_ - vb_) <= 2e-3 * abs(va_)
        assert T.load_checkpoint(path, m, opt, sched, [tr])["epoch"] == 4
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
