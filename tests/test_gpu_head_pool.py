"""The mean-pooled head on the GPU: csrc/head_pool.hip in both orders against the float64
reference of tests/_head_pool_ref.py, and set_global_pool('avg') on the models.

Tolerance.  No fixed number: in every comparison the composition the library offered before this head -- the full-row
LayerNorm kernels around a torch mean (norm-first), or a torch mean around the LayerNorm of the B pooled rows
(pool-first) -- is run on the same inputs against the same float64 reference, and the fused result's max-abs error may
be at most twice the composition's, per output: both sum the same n fp32 terms and differ in order (and, in the fused
kernels, in the fp64 accumulator) only.  Every test prints both errors before it asserts; DESIGN.md section 19 holds
the table measured on an MI355X.  Where a bound is not this rule, the test says where it comes from."""
import pytest
import torch

import _head_pool_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 65, 128), (2, 197, 384), (2, 50, 768), (4, 2, 128), (1, 1030, 128)]
NAMES = ("y", "dx", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


@pytest.fixture(autouse=True)
def _fp32_after(favit):
    yield
    favit.set_compute_dtype("fp32")
    favit.functional.clear_lp_mirrors()


def _inputs(B, L, D, seed=None):
    g = torch.Generator().manual_seed(B * 10000 + L * 10 + D if seed is None else seed)
    x = torch.randn(B, L, D, generator=g) * 1.7 + 0.3
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.3 * torch.randn(D, generator=g)
    dy = torch.randn(B, D, generator=g)
    return x, gamma, beta, dy


@pytest.fixture(scope="module")
def cases():
    """shape -> (host inputs, {norm_first: float64 (y, dx, dgamma, dbeta)}): computed once, never modified."""
    out = {}
    for shape in SHAPES:
        inp = _inputs(*shape)
        out[shape] = (inp, {nf: R.head_pool_grads(*inp, nf) for nf in (True, False)})
    return out


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _fused(favit, K, x, gamma, beta, dy, norm_first, first=1):
    """(y, dx, dgamma, dbeta) of the new entry points, called with NaN-filled outputs and workspace: an element the
    kernels leave unwritten (the CLS rows of dx included) stays NaN and fails the comparison."""
    lib, p, chk = favit._abi.lib(), K._p, favit._abi.check
    B, L, D = x.shape
    n = L - first
    ws = torch.full((lib.favit_head_pool_workspace(B, L, first, D) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    dx = _nan(B, L, D)
    if norm_first:
        y, s, mu, rs, dg, db = _nan(B, D), _nan(B, D), _nan(B, n), _nan(B, n), _nan(D), _nan(D)
        chk(lib.favit_ln_meanpool_fwd(p(x), p(gamma), p(beta), p(y), p(s), p(mu), p(rs), p(ws), B, L, first, D, 1e-5,
                                      K._st()), "favit_ln_meanpool_fwd")
        chk(lib.favit_ln_meanpool_bwd(p(dy), p(x), p(gamma), p(s), p(mu), p(rs), p(dx), p(dg), p(db), 0, B, L, first, D,
                                      K._st()), "favit_ln_meanpool_bwd")
        return y, dx, dg, db
    pm = _nan(B, D)
    chk(lib.favit_meanpool_fwd(p(x), p(pm), p(ws), B, L, first, D, K._st()), "favit_meanpool_fwd")
    y, mu, rs = K.layernorm_fwd(pm, D, gamma, beta, B, D, torch.float32)
    dp, _, dg, db = K.layernorm_bwd(dy, pm, D, gamma, mu, rs, B, D)
    chk(lib.favit_meanpool_bwd(p(dp), p(dx), B, L, first, D, K._st()), "favit_meanpool_bwd")
    return y, dx, dg, db


def _composition(K, x, gamma, beta, dy, norm_first, first=1):
    """The same head from the kernels the library had before: LayerNorm of ALL rows, a torch mean in fp32 and the
    matching backward (norm-first); a torch mean, the LayerNorm of the B pooled rows and an expand (pool-first)."""
    B, L, D = x.shape
    n = L - first
    dx = torch.zeros((B, L, D), device=DEV)
    if norm_first:
        x2 = x.view(B * L, D)
        rows, mu, rs = K.layernorm_fwd(x2, D, gamma, beta, B * L, D, torch.float32)
        y = rows.view(B, L, D)[:, first:].mean(1)
        up = torch.zeros((B, L, D), device=DEV)
        up[:, first:] = (dy / n)[:, None, :]
        dx, _, dg, db = K.layernorm_bwd(up.view(B * L, D), x2, D, gamma, mu, rs, B * L, D)
        return y, dx.view(B, L, D), dg, db
    pm = x[:, first:].mean(1).contiguous()
    y, mu, rs = K.layernorm_fwd(pm, D, gamma, beta, B, D, torch.float32)
    dp, _, dg, db = K.layernorm_bwd(dy, pm, D, gamma, mu, rs, B, D)
    dx[:, first:] = (dp / n)[:, None, :]
    return y, dx, dg, db


def _assert_within_twice(what, fused, comp, ref):
    """max-abs error of every fused output against float64 <= 2 x the composition's; both printed first."""
    bad = []
    for name, f, c, r in zip(NAMES, fused, comp, ref):
        assert f.shape == r.shape, (what, name, f.shape, r.shape)
        ef = (f.detach().double().cpu() - r).abs().max().item()
        ec = (c.detach().double().cpu() - r).abs().max().item()
        print(f"{what} {name}: fused {ef:.3e}  composition {ec:.3e}")
        if not ef <= 2 * ec:                                  # a NaN in the fused output fails here
            bad.append((name, ef, ec))
    assert not bad, (what, bad)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("norm_first", [True, False], ids=["norm_first", "pool_first"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_float64_as_well_as_the_composition(favit, K, cases, shape, norm_first):
    inp, refs = cases[shape]
    x, gamma, beta, dy = (t.to(DEV) for t in inp)
    fused = _fused(favit, K, x, gamma, beta, dy, norm_first)
    comp = _composition(K, x, gamma, beta, dy, norm_first)
    torch.cuda.synchronize()
    assert torch.equal(fused[1][:, :1], torch.zeros((shape[0], 1, shape[2]), device=DEV)), "the CLS rows of dx are zeros"
    _assert_within_twice(f"{shape} {'norm-first' if norm_first else 'pool-first'}", fused, comp, refs[norm_first])


@pytest.mark.parametrize("first", [0, 3])
def test_other_first_rows(favit, K, first):
    inp = _inputs(2, 70, 256, seed=first)
    x, gamma, beta, dy = (t.to(DEV) for t in inp)
    for nf in (True, False):
        ref = R.head_pool_grads(*inp, nf, first)
        fused = _fused(favit, K, x, gamma, beta, dy, nf, first)
        _assert_within_twice(f"first={first} nf={nf}", fused, _composition(K, x, gamma, beta, dy, nf, first), ref)
        assert torch.equal(fused[1][:, :first], torch.zeros((2, first, 256), device=DEV))


def test_wrappers_and_op_give_the_kernels_bits_and_accumulate(favit, K):
    F = favit.functional
    inp = _inputs(2, 197, 384, seed=5)
    x, gamma, beta, dy = (t.to(DEV) for t in inp)
    for nf in (True, False):
        y0, dx0, dg0, db0 = _fused(favit, K, x, gamma, beta, dy, nf)
        xr = x.clone().requires_grad_(True)
        g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.run(F.HeadPoolOp(nf), [xr], [g, b])
        y.backward(dy)
        assert torch.equal(y, y0) and torch.equal(xr.grad, dx0) and torch.equal(g.grad, dg0) and torch.equal(b.grad, db0)
        # existing fp32 gradient buffers are accumulated into
        prior_g, prior_b = g.grad.clone(), b.grad.clone()
        F.run(F.HeadPoolOp(nf), [xr], [g, b]).backward(dy)
        assert torch.allclose(g.grad, prior_g + dg0, rtol=1e-6, atol=1e-6)
        assert torch.allclose(b.grad, prior_b + db0, rtol=1e-6, atol=1e-6)
    y, s, mu, rs = K.ln_meanpool_fwd(x, gamma, beta)
    dx, dg, db = K.ln_meanpool_bwd(dy, x, gamma, s, mu, rs, frozen=True)
    assert dg is None and db is None and torch.equal(dx, _fused(favit, K, x, gamma, beta, dy, True)[1])


@pytest.mark.parametrize("shape", [(2, 197, 384), (1, 1030, 128), (2, 50, 768)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_identical(favit, K, shape):
    x, gamma, beta, dy = (t.to(DEV) for t in _inputs(*shape))
    for nf in (True, False):
        a = _fused(favit, K, x, gamma, beta, dy, nf)
        b = _fused(favit, K, x, gamma, beta, dy, nf)
        for name, u, v in zip(NAMES, a, b):
            assert torch.equal(u, v), (nf, name)


def test_unsupported_width_raises_before_any_launch(favit, K):
    x = torch.zeros((2, 9, 130), device=DEV)
    row, vec = torch.zeros((2, 130), device=DEV), torch.zeros(130, device=DEV)
    assert favit._abi.lib().favit_head_pool_workspace(2, 9, 1, 130) == favit._abi.ERR_UNSUPPORTED
    for call in (lambda: K.ln_meanpool_fwd(x, vec, vec),
                 lambda: K.ln_meanpool_bwd(row, x, vec, row, torch.zeros((2, 8), device=DEV), torch.zeros((2, 8), device=DEV)),
                 lambda: K.meanpool_fwd(x),
                 lambda: K.meanpool_bwd(row, 9)):
        with pytest.raises(RuntimeError, match=r"code -2"):
            call()
    wide = torch.zeros((1, 3, 2052), device=DEV)
    with pytest.raises(RuntimeError, match=r"code -2"):
        K.meanpool_fwd(wide)
    # the entry points themselves refuse it too, with the outputs untouched
    lib, p = favit._abi.lib(), K._p
    y = _nan(2, 130)
    assert lib.favit_meanpool_fwd(p(x), p(y), p(_nan(4096)), 2, 9, 1, 130, K._st()) == favit._abi.ERR_UNSUPPORTED
    dx = _nan(2, 9, 130)
    assert lib.favit_meanpool_bwd(p(row), p(dx), 2, 9, 1, 130, K._st()) == favit._abi.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(dx).all()


# ------------------------------------------------------------------ models
class _HeadTap:
    """Records what functional.HeadPoolOp saw in the model's own run: the encoder output it pooled, the upstream
    gradient and the gradient it handed back to the encoder."""

    def __init__(self, F, monkeypatch):
        self.x = self.dy = self.dx = None
        self.shapes = []
        fwd, bwd = F.HeadPoolOp.fwd, F.HeadPoolOp.bwd
        tap = self

        def rec_fwd(op, ins, prm):
            assert ins[0].dtype == torch.float32, "the encoder's output stream is fp32 in every compute mode"
            tap.x = ins[0].detach().clone()
            tap.shapes.append(tuple(ins[0].shape))
            return fwd(op, ins, prm)

        def rec_bwd(op, saved, dy, needs):
            out = bwd(op, saved, dy, needs)
            tap.dy, tap.dx = dy.detach().clone(), out[0][0].detach().clone()
            return out
        monkeypatch.setattr(F.HeadPoolOp, "fwd", rec_fwd)
        monkeypatch.setattr(F.HeadPoolOp, "bwd", rec_bwd)


def _mhla(favit, seed=7):
    torch.manual_seed(seed)
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, embed_dim=128, depth=2, num_heads=2,
                                                    window_size=7, use_mhla=True)
    with torch.no_grad():                                    # a norm that is not the identity
        m.norm.weight.add_(0.2 * torch.randn(128))
        m.norm.bias.add_(0.3 * torch.randn(128))
    return m.to(DEV)


def _head_logits(favit, m, pooled):
    F = favit.functional
    return F.run(F.LinearOp(), [pooled], [m.head.weight, m.head.bias])


def test_the_centre_of_the_image_reaches_the_avg_head_only(favit, K, monkeypatch):
    """L = 65, window 7, depth 2: the CLS row's logits depend on the token rows [0, 7) and [61, 65) only
    (functional.cls_plan).  Patch 30 is token row 31."""
    favit.set_compute_dtype("bf16")
    m = _mhla(favit).eval()
    assert favit.functional.cls_plan(65, 7, 2)[0] == (7, 4)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    x2 = x.clone()
    x2[:, :, 12:16, 24:28] += 1.5                             # patch 30 = grid row 3, column 6
    tap = _HeadTap(favit.functional, monkeypatch)
    with torch.no_grad():
        tok = m(x)
        assert torch.equal(tok, m(x2)), "the CLS head cannot see patch 30"
        assert tap.x is None
        for norm in ("before", "after"):
            m.set_global_pool("avg", norm)
            a, enc = m(x), tap.x
            assert enc.shape == (3, 65, 128), "the avg head pools the dense encoder output"
            assert not torch.equal(a, m(x2)), norm
            assert (a - m(x2)).abs().max().item() > 1e-4
            # the logits are the float64 head of the model's own encoder output, as well as the composition's are
            g, b = m.norm.weight.detach(), m.norm.bias.detach()
            dy0 = torch.zeros((3, 128), device=DEV)
            ref = (R.head_pool(enc.cpu(), g.cpu(), b.cpu(), norm == "before") @ m.head.weight.detach().double().cpu().T
                   + m.head.bias.detach().double().cpu())
            comp = _head_logits(favit, m, _composition(K, enc, g, b, dy0, norm == "before")[0])
            ef = (a.double().cpu() - ref).abs().max().item()
            ec = (comp.double().cpu() - ref).abs().max().item()
            print(f"avg/{norm} logits: fused {ef:.3e}  composition {ec:.3e}")
            assert ef <= 2 * ec
        m.set_global_pool("token")
        assert torch.equal(m(x), tok), "set_global_pool('avg') and back leaves the token path as it was"


@pytest.mark.parametrize("norm", ["before", "after"])
def test_avg_training_step_gradients_match_float64(favit, K, monkeypatch, norm):
    favit.set_compute_dtype("fp32")
    m = _mhla(favit).train().set_global_pool("avg", norm)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    y = torch.randint(0, 1000, (4,), generator=torch.Generator().manual_seed(3)).to(DEV)
    tap = _HeadTap(favit.functional, monkeypatch)
    loss = favit.train.cross_entropy(m(x), y)
    loss.backward()
    torch.cuda.synchronize()
    g, b = m.norm.weight.detach(), m.norm.bias.detach()
    ref = R.head_pool_grads(tap.x.cpu(), g.cpu(), b.cpu(), tap.dy.cpu(), norm == "before")
    comp = _composition(K, tap.x, g, b, tap.dy, norm == "before")
    pooled = _fused(favit, K, tap.x, g, b, tap.dy, norm == "before")[0]
    _assert_within_twice(f"train avg/{norm}", (pooled, tap.dx, m.norm.weight.grad, m.norm.bias.grad), comp, ref)
    for p in m.parameters():                                  # and the gradient went on into the whole encoder
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert m.blocks[0].norm1.weight.grad.abs().max().item() > 0 and m.pos_embed.grad[0, 31].abs().max().item() > 0


def test_graphed_avg_step_replays_match_eager_and_feed_fused_adamw(favit):
    """1e-5: what tests/test_gpu_cls_only.py allows between a replayed and an eager step of the same kernels."""
    T = favit.train
    favit.set_compute_dtype("fp32")
    rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    m, other = (_mhla(favit).train().set_global_pool("avg") for _ in range(2))
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    y = torch.randint(0, 1000, (4,), generator=torch.Generator().manual_seed(3)).to(DEV)
    mk = lambda mod: T.FusedAdamW(T.param_groups(mod, lr=0.0), lr=0.0, weight_decay=0.0, distributed=False,
                                  fuse_groups=True)
    opt, oo = mk(m), mk(other)
    want = [T.train_step(other, x, y, oo).item() for _ in range(2)]
    torch.cuda.synchronize()
    want_g = {k: p.grad.detach().clone() for k, p in other.named_parameters()}
    for k in ("norm.weight", "norm.bias"):                    # the fused optimizer's flat buffers received them
        assert torch.isfinite(want_g[k]).all() and want_g[k].abs().max().item() > 0, k
    step = T.GraphedStep(m, opt, x, y)
    for i in range(2):
        got = step(x, y).item()
        torch.cuda.synchronize()
        assert abs(got - want[i]) < 1e-5 * abs(want[i])
        worst = max((rel(p.grad, want_g[k]), k) for k, p in m.named_parameters())
        assert worst[0] < 1e-5, worst
    assert m.norm.weight.grad.abs().max().item() > 0 and torch.isfinite(m.norm.bias.grad).all()


def _sppp(favit):
    torch.manual_seed(5)
    S = 64
    m = favit.models.sppp.SPPPViT(img_size=S, patch_size=8, num_classes=10, embed_dim=64, depth=2, num_heads=4,
                                  num_superpixels=4, pooling_type="mean").to(DEV).train()
    ar = torch.arange(S)
    quad = (ar[:, None] >= S // 2).long() * 2 + (ar[None, :] >= S // 2).long()
    m.segmentation.set_label_maps(torch.stack([quad, quad, quad]).contiguous().to(DEV))
    return m, torch.randn(3, 3, S, S, generator=torch.Generator().manual_seed(6)).to(DEV)


def _dense(favit):
    torch.manual_seed(8)
    m = favit.models.vit.VisionTransformer(img_size=32, patch_size=8, num_classes=10, embed_dim=64, depth=2,
                                           num_heads=4).to(DEV).train()
    return m, torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(9)).to(DEV)


@pytest.mark.parametrize("norm", ["before", "after"])
@pytest.mark.parametrize("build", [_sppp, _dense], ids=["sppp", "dense_vit"])
def test_other_models_pool_their_tokens(favit, K, monkeypatch, build, norm):
    favit.set_compute_dtype("fp32")
    m, x = build(favit)
    m.set_global_pool("avg", norm)
    tap = _HeadTap(favit.functional, monkeypatch)
    logits = m(x)
    favit.train.cross_entropy(logits, torch.tensor([1, 4, 7], device=DEV)).backward()
    torch.cuda.synchronize()
    assert tap.x.shape[0] == 3 and tap.x.shape[2] == 64 and tap.x.shape[1] in (5, 17)
    g, b = m.norm.weight.detach(), m.norm.bias.detach()
    ref = R.head_pool_grads(tap.x.cpu(), g.cpu(), b.cpu(), tap.dy.cpu(), norm == "before")
    comp = _composition(K, tap.x, g, b, tap.dy, norm == "before")
    pooled = _fused(favit, K, tap.x, g, b, tap.dy, norm == "before")[0]
    _assert_within_twice(f"{type(m).__name__} avg/{norm}", (pooled, tap.dx, m.norm.weight.grad, m.norm.bias.grad), comp, ref)
    want = (R.head_pool(tap.x.cpu(), g.cpu(), b.cpu(), norm == "before") @ m.head.weight.detach().double().cpu().T
            + m.head.bias.detach().double().cpu())
    # the 10-class head is favit_small_linear_fwd, exact fp32 dot products of 64 terms: 64 * 2^-24 = 4e-6 bounds the
    # rounding of a dot product of terms of size one, on top of the pooled row's own error (printed above, below 1e-6)
    assert (logits.detach().double().cpu() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())


def test_avg_follows_the_token_count_at_another_resolution_and_in_fp8(favit, K, monkeypatch):
    x24 = torch.randn(3, 3, 24, 24, generator=torch.Generator().manual_seed(12)).to(DEV)
    y = torch.tensor([5, 900, 31], device=DEV)
    for mode, norm in (("fp32", "before"), ("fp32", "after"), ("fp8", "before")):
        favit.set_compute_dtype(mode)
        m = _mhla(favit).train().set_global_pool("avg", norm)
        tap = _HeadTap(favit.functional, monkeypatch)
        favit.train.cross_entropy(m(x24), y).backward()
        torch.cuda.synchronize()
        assert tap.shapes == [(3, 37, 128)], "6 x 6 patches and the CLS row: n follows the input"
        g, b = m.norm.weight.detach(), m.norm.bias.detach()
        ref = R.head_pool_grads(tap.x.cpu(), g.cpu(), b.cpu(), tap.dy.cpu(), norm == "before")
        comp = _composition(K, tap.x, g, b, tap.dy, norm == "before")
        pooled = _fused(favit, K, tap.x, g, b, tap.dy, norm == "before")[0]
        _assert_within_twice(f"24x24 {mode} avg/{norm}", (pooled, tap.dx, m.norm.weight.grad, m.norm.bias.grad), comp, ref)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        monkeypatch.undo()
        favit.functional.clear_lp_mirrors()


def test_token_bucketed_and_graphed_eval_run_the_avg_head(favit, monkeypatch):
    """TokenBucketed: groups of 5 and 4 token rows pool 4 and 3 of them; per image the logits are those of the image run
    alone (1e-5 rel-L2, the bound tests/test_gpu_modules.py sets for the same comparison with the CLS head).
    GraphedEval: the captured eval forward feeds EvalMetrics what the eager forward gives."""
    from conftest import rel_l2
    favit.set_compute_dtype("fp32")
    torch.manual_seed(21)
    S = 64
    m = favit.models.sppp_mhla.SPPPViTMHLA(img_size=S, patch_size=8, num_classes=10, embed_dim=64, depth=2, num_heads=4,
                                          num_superpixels=4, pooling_type="mean", window_size=3,
                                          use_mhla=True).to(DEV).eval().set_global_pool("avg", "after")
    ar = torch.arange(S)
    quad = (ar[:, None] >= S // 2).long() * 2 + (ar[None, :] >= S // 2).long()
    tri = torch.where(quad == 1, torch.zeros_like(quad), quad)
    maps = torch.stack([quad, tri, tri, quad]).contiguous().to(DEV)
    x = torch.randn(4, 3, S, S, device=DEV)
    m.segmentation.set_label_maps(maps)
    tap = _HeadTap(favit.functional, monkeypatch)
    with torch.no_grad():
        logits = favit.models.sppp.TokenBucketed(m)(x)
        assert sorted(tap.shapes) == [(2, 4, 64), (2, 5, 64)]
        rows = []
        for i in range(4):
            m.segmentation.set_label_maps(maps[i:i + 1].contiguous())
            rows.append(m(x[i:i + 1]))
    assert rel_l2(logits, torch.cat(rows)) < 1e-5
    m.segmentation.set_label_maps(None)
    monkeypatch.undo()

    H = favit.harness
    v = _mhla(favit).eval().set_global_pool("avg")
    xb = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(14)).to(DEV)
    yb = torch.randint(0, 1000, (4,), generator=torch.Generator().manual_seed(15)).to(DEV)
    eager, graphed = H.EvalMetrics(1000), H.EvalMetrics(1000)
    with torch.no_grad():
        eager.update(v(xb), yb)
    ge = H.GraphedEval(v, xb, yb, graphed)
    ge(xb, yb)
    a, b = eager.compute(), graphed.compute()
    assert a["n"] == b["n"] == 4 and abs(a["loss"] - b["loss"]) < 1e-5 * abs(a["loss"]) and a["top1"] == b["top1"]


def test_attention_maps_refuse_a_pooled_head(favit):
    favit.set_compute_dtype("fp32")
    m = _mhla(favit).eval()
    x = torch.randn(2, 3, 32, 32, device=DEV)
    assert favit.harness.attention_maps(m, x)["rollout"].shape == (2, 65)
    m.set_global_pool("avg")
    with pytest.raises(ValueError, match="CLS row"):
        favit.harness.attention_maps(m, x)
