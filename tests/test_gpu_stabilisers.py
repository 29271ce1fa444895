"""GPU tests of the training stabilisers: the deterministic global gradient norm (favit_grad_norm), AdamW with the
device-side clip coefficient and the non-finite skip (favit_adamw_clip), label-smoothed cross-entropy
(favit_cross_entropy_ls) and their way up through train.FusedAdamW, train.GraphedStep and data parallelism.
The reference is torch on the CPU in float64 (nn.CrossEntropyLoss, clip_grad_norm_, torch.optim.AdamW); the
cross-entropy and AdamW tolerances are those tests/test_gpu_kernels.py uses for the unsmoothed / unclipped kernels."""
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
LENS = [1, 63, 64, 65, 255, 257, 1023, 10007, 300001, 0]
ADAM = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.05)
LRS = (1e-3, 5e-3)                       # group 0 = even buffers, group 1 = odd buffers


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


def _like(src, values=None):
    """A tensor with src's length AND src's alignment class: odd-numbered buffers are views offset by one float."""
    n = src.numel()
    off = (src.data_ptr() % 16) // 4
    t = torch.empty(n + off, device=DEV)[off:]
    t.copy_(src if values is None else values)
    return t


@pytest.fixture(scope="module")
def bufs():
    """The buffers every kernel test shares (never written): every second one starts one float past a 16-byte
    boundary, so its vector body has a scalar head.  With the float64 norm computed once."""
    g = torch.Generator(device=DEV).manual_seed(7)
    out = []
    for i, n in enumerate(LENS):
        off = i % 2
        out.append((torch.randn(n + off, device=DEV, generator=g) * 2)[off:])
    for i, t in enumerate(out):
        assert t.numel() == LENS[i] and (t.numel() == 0 or (t.data_ptr() % 16 != 0) == (i % 2 == 1))
    ref = float(torch.sqrt(sum((t.double().cpu() ** 2).sum() for t in out)))
    return out, ref


def _bits(t):
    return t.detach().cpu().view(torch.int32).clone()


# ----------------------------------------------------------------------------------------------------------------
def test_grad_norm_kernel(K, bufs):
    ts, ref = bufs
    out = K.grad_norm(ts)
    norm = float(out[0])
    print(f"norm {norm!r} float64 {ref!r} rel {abs(norm - ref) / ref:.3e}")
    assert abs(norm - ref) <= 1e-6 * ref
    assert float(out[1]) == 1.0, "no max_norm: the coefficient is 1"
    again = K.grad_norm(ts)
    assert torch.equal(_bits(out), _bits(again)), "two calls must agree bitwise"
    half = K.grad_norm(ts, scale=0.5)
    assert float(half[0]) == 0.5 * norm, "a power-of-two scale only changes the exponent"
    f32 = torch.float32
    for mx, exact_one in ((ref / 4, False), (ref * 4, True)):
        o = K.grad_norm(ts, max_norm=mx)
        assert float(o[0]) == norm
        want = torch.clamp(torch.tensor(mx, dtype=f32) / (o[0].cpu() + torch.tensor(1e-6, dtype=f32)), max=1.0)
        print(f"max_norm {mx!r}: coef {float(o[1])!r} want {float(want)!r}")
        # one correctly rounded fp32 add and divide on either side: at most the last bit may differ
        assert abs(float(o[1]) - float(want)) <= 2.0 ** -23
        if exact_one:
            assert float(o[1]) == 1.0
        else:
            assert abs(float(o[1]) - 0.25) < 1e-6
    ws = torch.full_like(K.grad_norm_workspace(ts[0].device), float("nan"))
    fresh = K.grad_norm(ts, ws=ws)
    assert torch.equal(_bits(fresh), _bits(out)), "every workspace slot is written before it is read"
    # degenerate calls: nothing but empty buffers, and a single element
    z = K.grad_norm([ts[-1]], max_norm=1.0)
    assert float(z[0]) == 0.0 and float(z[1]) == 1.0
    one = K.grad_norm([ts[0]])
    assert float(one[0]) == abs(float(ts[0][0]))


def _state(ts):
    g = torch.Generator(device=DEV).manual_seed(11)
    p = [_like(t, torch.randn(t.numel(), device=DEV, generator=g)) for t in ts]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    lp = [t.to(torch.bfloat16) for t in p]
    return p, m, v, lp


def _adamw_all(K, p, g, m, v, lp, step, coef=None, skip=False):
    for i in range(len(p)):
        kw = {} if coef is None else dict(coef=coef, skip_nonfinite=skip)
        if coef is None and p[i].numel() == 0:
            continue
        K.adamw(p[i], g[i], m[i], v[i], LRS[i % 2], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], step, p_lp=lp[i], **kw)


def test_clipped_adamw_matches_torch(K, bufs):
    ts, ref = bufs
    mx = ref / 4
    p, m, v, lp = _state(ts)
    rp = [torch.nn.Parameter(t.double().cpu()) for t in p]
    opt = torch.optim.AdamW([{"params": rp[0::2], "lr": LRS[0]}, {"params": rp[1::2], "lr": LRS[1]}],
                            betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"], weight_decay=ADAM["wd"])
    out = torch.empty(2, device=DEV)
    for step, s in ((1, 1.0), (2, 0.5), (3, 2.0)):            # three different norms, all above max_norm
        g = [_like(t, t * s) for t in ts]
        for r, t in zip(rp, g):
            r.grad = t.double().cpu()
        total = torch.nn.utils.clip_grad_norm_(rp, mx)
        opt.step()
        K.grad_norm(g, max_norm=mx, out=out)
        _adamw_all(K, p, g, m, v, lp, step, coef=out[1:2])
        assert abs(float(out[0]) - float(total)) <= 1e-6 * float(total) and float(out[1]) < 0.6
    got = torch.cat([t.flatten() for t in p])
    want = torch.cat([r.detach().flatten() for r in rp])
    print(f"clipped AdamW, 3 steps: parameters rel-L2 {rel_l2(got, want):.3e}")
    assert rel_l2(got, want) < 1e-6
    for grp in (0, 1):
        assert rel_l2(torch.cat([t for t in p[grp::2]]), torch.cat([r.detach() for r in rp[grp::2]])) < 1e-6
    for t, l in zip(p, lp):
        assert torch.equal(l, t.to(torch.bfloat16))
    # coefficient exactly 1: the same bits as plain favit_adamw, from the same state
    one = K.grad_norm(ts, max_norm=ref * 4)
    assert float(one[1]) == 1.0
    a, b = _state(ts), _state(ts)
    for step in (1, 2):
        _adamw_all(K, *[a[0], ts, a[1], a[2], a[3]], step, coef=one[1:2])
        _adamw_all(K, *[b[0], ts, b[1], b[2], b[3]], step)
    for xs, ys in zip(a, b):
        for x, y in zip(xs, ys):
            assert torch.equal(_bits(x.float()), _bits(y.float()))


def test_nonfinite_update_is_skipped_or_propagates(favit, K, bufs):
    ts, ref = bufs
    bad = [_like(t) for t in ts]
    bad[7][5000] = float("nan")
    health = favit.train.Health()
    try:
        # skip on: nothing moves, the counter counts
        p, m, v, lp = _state(ts)
        before = [[_bits(x.float()) for x in xs] for xs in (p, m, v, lp)]
        out, cnt = torch.empty(2, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        K.grad_norm(bad, max_norm=ref / 4, out=out, skipped=cnt)
        _adamw_all(K, p, bad, m, v, lp, 1, coef=out[1:2], skip=True)
        after = [[_bits(x.float()) for x in xs] for xs in (p, m, v, lp)]
        assert all(torch.equal(x, y) for xs, ys in zip(before, after) for x, y in zip(xs, ys))
        assert int(cnt) == 1 and not torch.isfinite(out).any()
        rep = health.poll()
        assert rep is not None and "gradient" in rep["non_finite"] and "parameter" not in rep["non_finite"]
        assert rep["adamw_launches"] == sum(1 for t in ts if t.numel()), "a skipped launch still counts itself"
        # the next clean step updates; the counter stays
        K.grad_norm(ts, max_norm=ref / 4, out=out, skipped=cnt)
        _adamw_all(K, p, ts, m, v, lp, 2, coef=out[1:2], skip=True)
        assert int(cnt) == 1
        for i, t in enumerate(p):
            if t.numel():
                assert not torch.equal(_bits(t), before[0][i]) and bool(torch.isfinite(t).all())
                assert torch.equal(lp[i], t.to(torch.bfloat16))
        # skip off: the NaN coefficient reaches every parameter, as clip_grad_norm_ + AdamW do in torch
        health.words.zero_()
        p, m, v, lp = _state(ts)
        K.grad_norm(bad, max_norm=ref / 4, out=out, skipped=cnt)
        _adamw_all(K, p, bad, m, v, lp, 1, coef=out[1:2], skip=False)
        assert int(cnt) == 2
        assert all(bool(torch.isnan(t).all()) for t in p)
        rp = [torch.nn.Parameter(torch.ones(n, dtype=torch.float64)) for n in LENS]
        for r, t in zip(rp, bad):
            r.grad = t.double().cpu()
        torch.nn.utils.clip_grad_norm_(rp, ref / 4)
        torch.optim.AdamW(rp, lr=1e-3).step()
        assert all(bool(torch.isnan(r).all()) for r in rp), "the torch behaviour this mirrors"
        rep = health.poll()
        assert rep is not None and "gradient" in rep["non_finite"] and "parameter" in rep["non_finite"]
    finally:
        health.close()


# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [10, 65, 1000])
def test_label_smoothing(favit, K, Cn):
    B, eps = 37, 0.1
    g = torch.Generator(device=DEV).manual_seed(Cn)
    logits = torch.randn(B, Cn, device=DEV, generator=g) * 3
    logits[5] = 80.0 * (1 - 2 * (torch.arange(Cn, device=DEV) % 2))           # one row of +-80
    labels = torch.randint(0, Cn, (B,), device=DEV, generator=g)
    ref_in = logits.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(ref_in, labels.cpu(), label_smoothing=eps)
    ref.backward()
    rows, dlog = K.cross_entropy(logits, labels, grad_scale=1.0 / B, label_smoothing=eps)
    print(f"C={Cn}: loss {rows.mean().item()!r} ref {ref.item()!r}; dlogits rel-L2 {rel_l2(dlog, ref_in.grad):.3e}")
    assert abs(rows.double().mean().item() - ref.item()) < 1e-5
    assert rel_l2(dlog, ref_in.grad) < 2e-5
    # eps = 0 through the NEW entry point: the bits of favit_cross_entropy
    rows0, dlog0 = K.cross_entropy(logits, labels, grad_scale=1.0 / B)
    rows1, dlog1 = torch.empty_like(rows0), torch.empty_like(dlog0)
    lib, P = favit._abi.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.favit_cross_entropy_ls(P(logits), P(labels), P(rows1), P(dlog1), B, Cn, 1.0 / B, 0.0, st) == 0
    assert torch.equal(_bits(rows0), _bits(rows1)) and torch.equal(_bits(dlog0), _bits(dlog1))
    assert lib.favit_cross_entropy_ls(P(logits), P(labels), P(rows1), P(dlog1), B, Cn, 1.0 / B, 1.0, st) == favit._abi.ERR_INVALID
    # an out-of-range label: a NaN row, the others untouched
    lab2 = labels.clone()
    lab2[3] = -100
    rows2, _ = K.cross_entropy(logits, lab2, grad_scale=1.0 / B, label_smoothing=eps)
    assert bool(torch.isnan(rows2[3])) and torch.equal(_bits(torch.cat([rows2[:3], rows2[4:]])), _bits(torch.cat([rows[:3], rows[4:]])))
    # the autograd wrapper
    x = logits.clone().requires_grad_(True)
    loss = favit.train.cross_entropy(x, labels, label_smoothing=eps)
    loss.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 and rel_l2(x.grad, ref_in.grad) < 2e-5


# ----------------------------------------------------------------------------------------------------------------
def _vit(favit, seed=11):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                       num_heads=4, use_mhla=True).to(DEV).train()


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
    assert n0 > 0
    return xs, ys, n0


def test_clipped_training_steps_match_torch(favit, vit_case):
    xs, ys, n0 = vit_case
    mx = n0 / 4
    T = favit.train
    favit.set_compute_dtype("bf16")
    try:
        m1 = _vit(favit)
        o1 = T.FusedAdamW(T.param_groups(m1, lr=1e-3), lr=1e-3, weight_decay=0.05, distributed=False, max_grad_norm=mx)
        norms = []
        for x, y in zip(xs, ys):
            T.train_step(m1, x, y, o1)
            norms.append(o1.grad_norm.clone())                   # (device side: no sync inside the loop)
        # the same model, gradients copied out, clip_grad_norm_ + torch.optim.AdamW in float64 on the CPU
        m2 = _vit(favit)
        ref = {id(p): torch.nn.Parameter(p.detach().double().cpu()) for p in m2.parameters()}
        o2 = torch.optim.AdamW([{"params": [ref[id(p)] for p in g_["params"]], "lr": g_["lr"]}
                                for g_ in T.param_groups(m2, lr=1e-3)], lr=1e-3, weight_decay=0.05)
        ref_norms = []
        for x, y in zip(xs, ys):
            m2.zero_grad(set_to_none=True)
            T.cross_entropy(m2(x), y).backward()
            for p in m2.parameters():                            # (a parameter without a gradient: zeros, as in flat_g)
                ref[id(p)].grad = p.grad.double().cpu() if p.grad is not None else torch.zeros_like(ref[id(p)])
            ref_norms.append(float(torch.nn.utils.clip_grad_norm_(list(ref.values()), mx)))
            o2.step()
            with torch.no_grad():
                for p in m2.parameters():
                    p.copy_(ref[id(p)].detach().float())
        norms = [float(n) for n in norms]
        print(f"n0 {n0!r} max_grad_norm {mx!r}; opt.grad_norm per step {norms}; reference {ref_norms}")
        assert all(n > mx for n in norms), "clipping was active at every step"
        # (the same gradient from a second run of the same kernels: a few fp32 atomics land in another order)
        assert abs(norms[0] - n0) <= 1e-5 * n0
        assert int(o1.skipped_steps) == 0
        w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
        w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        print(f"weights rel-L2 after three clipped steps: {rel_l2(w1, w2):.3e}")
        assert rel_l2(w1, w2) < 1e-3
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


def test_graphed_step_with_clipping_matches_eager(favit, vit_case):
    xs, ys, n0 = vit_case
    T = favit.train
    favit.set_compute_dtype("bf16")

    def build():
        m = _vit(favit)
        return m, T.FusedAdamW(T.param_groups(m, lr=1e-3), lr=1e-3, weight_decay=0.05, distributed=False,
                               max_grad_norm=n0 / 4, skip_nonfinite=True)
    try:
        m1, o1 = build()
        eager = [T.train_step(m1, x, y, o1).item() for x, y in zip(xs, ys)]
        m2, o2 = build()
        step = T.GraphedStep(m2, o2, xs[0], ys[0])
        graphed = [step(x, y).item() for x, y in zip(xs, ys)]
        for a, b in zip(eager, graphed):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (eager, graphed)
        w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
        w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        assert rel_l2(w2.cpu(), w1.cpu()) < 1e-3
        assert int(o1.skipped_steps) == 0 and int(o2.skipped_steps) == 0
        assert float(o2.grad_norm) > n0 / 4
    finally:
        favit.set_compute_dtype("fp32")
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
    opt = pkg.train.FusedAdamW(pkg.train.param_groups(m, lr=1e-2), lr=1e-2, weight_decay=0.0, bucket_mb=0.05,
                               max_grad_norm=max_norm)
    x, y = _dp_batch()
    lo = rank * 4
    xs, ys = x[lo:lo + 4].cuda(), y[lo:lo + 4].cuda()
    norms = []
    for _ in range(2):
        pkg.train.train_step(m, xs, ys, opt)
        norms.append(opt.grad_norm.clone())
    torch.cuda.synchronize()
    w = torch.cat([p.detach().flatten().cpu() for p in m.parameters()])
    torch.save({"w": w, "norms": [float(n) for n in norms], "skipped": int(opt.skipped_steps)}, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_dp_two_ranks_clip_by_the_whole_batch_norm(favit, tmp_path):
    favit.set_compute_dtype("fp32")
    try:
        m = _dp_model(favit)
        x, y = _dp_batch()
        favit.train.cross_entropy(m(x.cuda()), y.cuda()).backward()
        n_ref = _grad_norm64(m)
    finally:
        favit.functional.clear_lp_mirrors()
    out = str(tmp_path / "dpclip")
    mp.spawn(_dp_worker, args=(2, 38500 + (os.getpid() % 2000), out, n_ref / 4), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=True), torch.load(out + ".1", weights_only=True)
    print(f"whole-batch norm {n_ref!r}; rank norms {r0['norms']} {r1['norms']}")
    for r in (r0, r1):
        assert abs(r["norms"][0] - n_ref) <= 2e-5 * n_ref
        assert r["norms"][0] > n_ref / 4 and r["skipped"] == 0
    assert r0["norms"] == r1["norms"], "both ranks reduce the same all-reduced gradient in the same order"
    assert torch.equal(r0["w"], r1["w"]), "the two ranks diverged"
