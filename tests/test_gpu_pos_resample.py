"""Position-embedding resampling on the GPU: favit_pos_resample and its adjoint against the float64 matrix product
under a running error bound, whole models at input resolutions other than their own against the float64 oracle with an
autograd-resampled pos_embed, the bf16 / CLS-only path at a resampled token count, and checkpoint import with a
device-resampled pos_embed followed by graphed training steps.

The MHLA models here are 64 wide with 4 heads: the windowed-attention kernels take head widths of 16, 32, 64 and 128
(include/favit.h), so a width of 32 with 4 heads (head width 8) cannot run; the dense model keeps 32 x 4."""
import pytest
import torch
import torch.nn.functional as TF

import _pretrained_ref as S
from conftest import rel_l2
from oracle import favit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL, GRAD_TOL = 1e-4, 5e-4            # tests/test_gpu_modules.py, fp32 mode
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _fp32_mode(favit):
    favit.set_compute_dtype("fp32")
    yield
    favit.set_compute_dtype("fp32")


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


# ------------------------------------------------------------------ the kernel, both directions
def _apply64(M, x, n_prefix, g_src):
    """float64 [n_prefix + g_src^2, D] -> [n_prefix + g_dst^2, D] with the dense matrix M [g_dst, g_src] on both axes."""
    D = x.shape[1]
    grid = torch.einsum("ai,bj,ijd->abd", M, M, x[n_prefix:].reshape(g_src, g_src, D))
    return torch.cat((x[:n_prefix], grid.reshape(-1, D)), dim=0)


def _bound(M, x, n_prefix, g_src):
    """2 (t^2 + 4) 2^-24 (|M| (x) |M|) |x| per element, t the largest tap count of M; 0 on the prefix rows.  t^2
    products and additions, four roundings for the two fp32 weights and their product, a factor 2 of slack."""
    t = int((M != 0).sum(dim=1).max())
    b = 2.0 * (t * t + 4) * U * _apply64(M.abs(), x.abs(), n_prefix, g_src)
    b[:n_prefix] = 0.0
    return b


def _randn_with_spikes(shape, gen):
    x = torch.randn(shape, generator=gen)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // 97)]
    flat[idx] = torch.where(torch.arange(len(idx)) % 2 == 0, 1e3, -1e3)
    return x


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("g_in,g_out", [(1, 4), (4, 1), (2, 3), (3, 2), (5, 3), (14, 24), (24, 14), (7, 7)])
def test_forward_and_adjoint_against_the_float64_matrix(favit, K, g_in, g_out, antialias):
    M = favit.functional.pos_resample_matrix(g_in, g_out, antialias)
    for D in (4, 36, 192):
        for n_prefix in (0, 1):
            gen = torch.Generator().manual_seed(1000 * g_in + 10 * g_out + D + n_prefix)
            x = _randn_with_spikes((n_prefix + g_in * g_in, D), gen)
            g = _randn_with_spikes((n_prefix + g_out * g_out, D), gen)
            tag = (g_in, g_out, antialias, D, n_prefix)
            y = K.pos_resample(x.to(DEV), g_in, g_out, antialias, n_prefix).cpu()
            dx = K.pos_resample(g.to(DEV), g_in, g_out, antialias, n_prefix, adjoint=True)
            dx2 = K.pos_resample(g.to(DEV), g_in, g_out, antialias, n_prefix, adjoint=True)
            assert torch.equal(dx, dx2), tag                              # a gather in table order: the same bits
            dx = dx.cpu()
            assert tuple(y.shape) == (n_prefix + g_out * g_out, D) and tuple(dx.shape) == tuple(x.shape)
            by, bx = _bound(M, x.double(), n_prefix, g_in), _bound(M.t().contiguous(), g.double(), n_prefix, g_out)
            ey = (y.double() - _apply64(M, x.double(), n_prefix, g_in)).abs()
            ex = (dx.double() - _apply64(M.t().contiguous(), g.double(), n_prefix, g_out)).abs()
            assert bool((ey <= by).all()), (tag, "forward", float((ey - by).max()))
            assert bool((ex <= bx).all()), (tag, "adjoint", float((ex - bx).max()))
            if n_prefix:
                assert torch.equal(y[:1], x[:1]) and torch.equal(dx[:1], g[:1]), tag
            if g_in == g_out:
                assert torch.equal(y, x) and torch.equal(dx, g), tag      # the identity, bit for bit
            lhs, rhs = (y.double() * g.double()).sum(), (x.double() * dx.double()).sum()
            slack = (by * g.double().abs()).sum() + (x.double().abs() * bx).sum()
            assert abs(float(lhs - rhs)) <= float(slack), (tag, float(lhs - rhs), float(slack))


def test_autograd_wrapper_and_refusals(favit, K):
    F = favit.functional
    pos = torch.randn(1, 1 + 9, 8, device=DEV, requires_grad=True)
    out = F.pos_resample(pos, 5, antialias=False)
    assert tuple(out.shape) == (1, 26, 8)
    g = torch.randn_like(out)
    out.backward(g)
    assert tuple(pos.grad.shape) == (1, 10, 8)
    assert torch.equal(pos.grad[0], K.pos_resample(g[0].contiguous(), 3, 5, False, 1, adjoint=True))
    with pytest.raises(ValueError, match="multiple of 4"):
        K.pos_resample(torch.zeros(10, 6, device=DEV), 3, 5)
    with pytest.raises(ValueError, match="contiguous fp32"):
        K.pos_resample(torch.zeros(11, 8, device=DEV), 3, 5)
    with pytest.raises(ValueError, match="token rows"):
        K.pos_resample(torch.zeros(10, 8, device=DEV), 3, 128)
    lib, A = favit._abi.lib(), favit._abi
    x, y = torch.zeros(17, 8, device=DEV), torch.zeros(17, 8, device=DEV)
    rp, co, va = K.pos_resample_tables(4, 4, True, x.device)[0]
    p = lambda t: t.data_ptr()
    assert lib.favit_pos_resample(p(x), p(x), p(rp), p(co), p(va), 4, 4, 1, 8, None) == A.ERR_INVALID
    assert lib.favit_pos_resample(p(x), p(y), p(rp), p(co), p(va), 4, 4, 2, 8, None) == A.ERR_INVALID
    assert lib.favit_pos_resample(p(x), p(y), p(rp), p(co), p(va), 4, 4, 1, 6, None) == A.ERR_INVALID
    assert lib.favit_pos_resample(p(x), p(y), p(rp), p(co), p(va), 128, 4, 1, 8, None) == A.ERR_UNSUPPORTED
    assert lib.favit_pos_resample(p(x) + 4, p(y), p(rp), p(co), p(va), 4, 4, 0, 8, None) == A.ERR_ALIGN


# ------------------------------------------------------------------ whole models at another resolution, fp32 mode
def _resampled64(pos, g_out, antialias):
    """cat(cls_row, F.interpolate(grid)): the autograd reference of the resampling, float64."""
    g_in = int(round((pos.shape[1] - 1) ** 0.5))
    grid = pos[:, 1:].reshape(1, g_in, g_in, -1).permute(0, 3, 1, 2)
    grid = TF.interpolate(grid, size=(g_out, g_out), mode="bicubic", align_corners=False, antialias=antialias)
    return torch.cat((pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, g_out * g_out, -1)), dim=1)


def _build(favit, kind, depth=2, seed=21, width=64, heads=4):
    torch.manual_seed(seed)
    M = favit.models
    if kind == "vit":
        m = M.vit.VisionTransformer(img_size=16, patch_size=4, num_classes=5, embed_dim=32, depth=depth, num_heads=4)
        fwd = lambda x, sd: O.vit_forward(x, sd, 4, 4)
    elif kind == "vit_mhla":
        m = M.vit_mhla.VisionTransformerMHLA(img_size=16, patch_size=4, num_classes=5, embed_dim=width, depth=depth,
                                             num_heads=heads, window_size=7, use_mhla=True)
        fwd = lambda x, sd: O.vit_mhla_forward(x, sd, 4, heads, 7, True)
    else:
        m = M.mhla_models.PretrainedViTWithMHLA(img_size=16, patch_size=4, num_classes=5, embed_dim=64, depth=depth,
                                                num_heads=4, window_size=5)
        fwd = lambda x, sd: O.pretrained_vit_mhla_forward(x, sd, 4, 4, 5)
    return m, fwd


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("size", [24, 8])
@pytest.mark.parametrize("kind", ["vit_mhla", "vit", "pretrained_mhla"])
def test_model_at_another_resolution_against_the_oracle(favit, kind, size, antialias):
    m, fwd = _build(favit, kind)
    m.set_pos_antialias(antialias)
    gen = torch.Generator().manual_seed(size)
    x = torch.randn(3, 3, size, size, generator=gen)
    gout = torch.randn(3, 5, generator=gen)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    run = dict(sd)
    run["pos_embed"] = _resampled64(sd["pos_embed"], size // 4, antialias)
    ref = fwd(x.double(), run)
    (ref * gout.double()).sum().backward()
    m.to(DEV).eval()
    y = m(x.to(DEV))
    assert rel_l2(y, ref) < FWD_TOL, rel_l2(y, ref)
    (y * gout.to(DEV)).sum().backward()
    assert tuple(m.pos_embed.grad.shape) == (1, 17, m.embed_dim)
    for k, p in m.named_parameters():
        r = sd[k].grad
        if r.abs().max() < 1e-5:                    # (the rule of tests/test_gpu_modules.py for vanishing gradients)
            assert p.grad.abs().max().item() < 1e-4, k
        else:
            assert rel_l2(p.grad, r) < GRAD_TOL, (k, rel_l2(p.grad, r))


@pytest.mark.parametrize("kind", ["vit_mhla", "vit", "pretrained_mhla"])
def test_native_resolution_never_reaches_the_resampling(favit, K, monkeypatch, kind):
    m1, _ = _build(favit, kind)
    m2, _ = _build(favit, kind)
    x = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    y2 = m2.to(DEV).eval()(x)

    def boom(*a, **k):
        raise AssertionError("pos_resample called at the model's own resolution")
    monkeypatch.setattr(K, "pos_resample", boom)
    y1 = m1.to(DEV).eval()(x)
    y1.sum().backward()
    assert torch.equal(y1, y2) and tuple(m1.pos_embed.grad.shape) == (1, 17, m1.embed_dim)


def test_token_counts_that_are_no_square_grid_are_refused(favit):
    F = favit.functional
    cls = torch.zeros(1, 1, 32, device=DEV)
    with pytest.raises(ValueError, match=r"15 patch tokens.*16 grid rows"):
        F.run(F.PrologueOp(True), [torch.zeros(2, 15, 32, device=DEV)], [cls, torch.zeros(1, 17, 32, device=DEV)])
    with pytest.raises(ValueError, match=r"16 patch tokens.*15 grid rows"):
        F.run(F.PrologueOp(True), [torch.zeros(2, 16, 32, device=DEV)], [cls, torch.zeros(1, 16, 32, device=DEV)])


# ------------------------------------------------------------------ bf16 mode, CLS-only pruned path
def _step(favit, m, x, y):
    for p in m.parameters():
        p.grad = None
    logits = m(x)
    favit.train.cross_entropy(logits, y).backward()
    torch.cuda.synchronize()
    return logits.detach().float().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("width,heads", [(64, 4), (128, 2)])
def test_bf16_pruned_path_at_a_resampled_token_count(favit, K, monkeypatch, width, heads):
    """Depth 4 on 32 x 32 input: the 4 x 4 pos_embed becomes 8 x 8, L = 65, and every block runs on fewer rows than
    the one below; at 128 x 2 (head width 64) the bf16 blocks are the native chains with narrowed MLP halves.  bf16 against the fp32-mode run at the bounds of the existing bf16 comparisons (2e-2 logits, 5e-2
    gradients, rel-L2), pruned against FAVIT_NO_PRUNE=1 (read at every call) at tests/test_gpu_cls_only.py's 1.5e-2."""
    gen = torch.Generator().manual_seed(6)
    x, y = torch.randn(3, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 5, (3,), generator=gen).to(DEV)
    monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
    cuts = [0]
    orig = K.rows_cut_fwd

    def counted(*a, **k):
        cuts[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(K, "rows_cut_fwd", counted)
    out = {}
    try:
        for mode in ("fp32", "bf16"):
            favit.set_compute_dtype(mode)
            m = _build(favit, "vit_mhla", depth=4, width=width, heads=heads)[0].to(DEV)
            cuts[0] = 0
            out[mode, "train"] = _step(favit, m.train(), x, y)
            assert cuts[0] == 4, "the pruned plan runs at the resampled token count"
            with torch.no_grad():
                out[mode, "eval"] = m.eval()(x).float().clone()
            assert cuts[0] == 8
            if mode == "bf16":
                monkeypatch.setenv("FAVIT_NO_PRUNE", "1")
                out["full"] = _step(favit, m.train(), x, y)
                assert cuts[0] == 8, "FAVIT_NO_PRUNE=1 takes the full path"
                monkeypatch.delenv("FAVIT_NO_PRUNE")
    finally:
        favit.set_compute_dtype("fp32")
    (l32, g32), (l16, g16), (lf, gf) = out["fp32", "train"], out["bf16", "train"], out["full"]
    assert rel_l2(l16, l32) < 2e-2 and rel_l2(out["bf16", "eval"], out["fp32", "eval"]) < 2e-2
    worst = max((rel_l2(g16[k], g32[k]), k) for k in g32)
    print(f"\nbf16 vs fp32: logits {rel_l2(l16, l32):.2e}, worst gradient {worst[0]:.2e} ({worst[1]})", end="")
    assert worst[0] < 5e-2, worst
    worst = max((rel_l2(g16[k], gf[k]), k) for k in gf)
    print(f"; pruned vs full: logits {rel_l2(l16, lf):.2e}, worst gradient {worst[0]:.2e} ({worst[1]})", end="")
    assert rel_l2(l16, lf) < 1.5e-2 and worst[0] < 1.5e-2, worst
    assert tuple(g16["pos_embed"].shape) == (1, 17, width)


def test_fp8_mode_at_another_resolution(favit):
    """The prologue is fp32 in every compute mode, so fp8 mode simply works: the resampled prologue and its gradients are
    bit for bit those of fp32 mode, and the whole fp8 step at 24 x 24 stays within the logits bound the existing fp8
    comparison uses against its reference (tests/test_gpu_cfg4_shapes.py: 0.15 rel-L2), with finite gradients."""
    F = favit.functional
    gen = torch.Generator().manual_seed(9)
    tok = torch.randn(2, 36, 64, generator=gen).to(DEV)
    gout = torch.randn(2, 37, 64, generator=gen).to(DEV)
    x = torch.randn(3, 3, 24, 24, generator=gen).to(DEV)
    y = torch.randint(0, 5, (3,), generator=gen).to(DEV)
    got = {}
    try:
        for mode in ("fp32", "fp8"):
            favit.set_compute_dtype(mode)
            cls = torch.randn(1, 1, 64, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
            pos = torch.randn(1, 17, 64, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
            out = F.run(F.PrologueOp(True), [tok], [cls, pos])
            out.backward(gout)
            m = _build(favit, "vit_mhla")[0].to(DEV).train()
            got[mode] = (out.detach().clone(), cls.grad.clone(), pos.grad.clone()) + _step(favit, m, x, y)
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
    for a, b in zip(got["fp32"][:3], got["fp8"][:3]):
        assert torch.equal(a, b)
    assert tuple(got["fp8"][2].shape) == (1, 17, 64)
    assert rel_l2(got["fp8"][3], got["fp32"][3]) < 0.15, rel_l2(got["fp8"][3], got["fp32"][3])
    for k, g in got["fp8"][4].items():
        assert bool(torch.isfinite(g).all()), k
    assert tuple(got["fp8"][4]["pos_embed"].shape) == (1, 17, 64) and float(got["fp8"][4]["pos_embed"].abs().max()) > 0


# ------------------------------------------------------------------ load, then run
def test_load_resamples_on_the_device_then_graphed_steps_and_maps(favit):
    src = S.source_model(seed=12, img=32, d=64)                    # an 8 x 8 source grid, torchvision layout
    sd = src.state_dict()

    def build():
        torch.manual_seed(13)
        m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=16, patch_size=4, num_classes=5, embed_dim=64, depth=2,
                                                        num_heads=4, window_size=7, use_mhla=True).to(DEV)
        rep = favit.pretrained.load_pretrained(m, sd)
        return m, rep
    m1, rep = build()
    assert (rep["layout"], rep["source_grid"], rep["model_grid"], rep["pos_embed"]) == ("torchvision", 8, 4, "resampled")
    assert "8x8 -> 4x4" in rep.summary() and sorted(rep["missing"]) == sorted(k for k in m1.state_dict() if "latent_proj" in k)
    M = favit.functional.pos_resample_matrix(8, 4, True)
    p64 = sd["encoder.pos_embedding"][0].double()
    err = (m1.pos_embed.detach().cpu()[0].double() - _apply64(M, p64.float().double(), 1, 8)).abs()
    assert bool((err <= _bound(M, p64.float().double(), 1, 8)).all())
    assert torch.equal(m1.pos_embed.detach().cpu()[0, 0], p64[0].float())
    assert torch.equal(m1.norm.weight.detach().cpu(), sd["encoder.ln.weight"].float())
    before = {k: v.clone() for k, v in m1.state_dict().items()}
    with pytest.raises(ValueError, match="strict"):
        favit.pretrained.load_pretrained(m1, sd, pos_embed="strict")
    assert all(torch.equal(v, before[k]) for k, v in m1.state_dict().items())

    maps = favit.harness.attention_maps(m1, torch.randn(2, 3, 24, 24, device=DEV))
    assert tuple(maps["grid"].shape) == (2, 6, 6) and tuple(maps["rollout"].shape) == (2, 37)

    # two FusedAdamW steps at 24 x 24 (a 6 x 6 grid from the 4 x 4 parameter): graph replays against eager steps, at the
    # tolerances of tests/test_gpu_modules.py::test_graphed_step_matches_eager_steps
    favit.set_compute_dtype("bf16")
    try:
        g = torch.Generator(device=DEV).manual_seed(14)
        xs = [torch.randn(8, 3, 24, 24, device=DEV, generator=g) for _ in range(2)]
        ys = [torch.randint(0, 5, (8,), device=DEV, generator=g) for _ in range(2)]

        def opt_of(m):
            return favit.train.FusedAdamW(favit.train.param_groups(m.train(), lr=1e-3), lr=1e-3, weight_decay=0.05,
                                          distributed=False)
        o1 = opt_of(m1)
        eager = [favit.train.train_step(m1, x, y, o1).item() for x, y in zip(xs, ys)]
        m2, _ = build()
        o2 = opt_of(m2)
        step = favit.train.GraphedStep(m2, o2, xs[0], ys[0])
        graphed = [step(x, y).item() for x, y in zip(xs, ys)]
        for a, b in zip(eager, graphed):
            assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (eager, graphed)
        w1 = torch.cat([p.detach().flatten() for p in m1.parameters()])
        w2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        assert rel_l2(w2.cpu(), w1.cpu()) < 1e-3
        assert rel_l2(m2.pos_embed, m1.pos_embed) < 1e-3 and not torch.equal(m2.pos_embed.detach(), before["pos_embed"])
    finally:
        favit.set_compute_dtype("fp32")
