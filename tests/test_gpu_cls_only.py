"""CLS-only encoders on the GPU: the row-cut kernels against torch indexing, and the pruned step
against the full path (FAVIT_NO_PRUNE=1) and the CPU oracle on one small model.

Tolerances are the project's full-size consistency bounds (tests/test_gpu_fullsize.py), because the pruned and the full
run pick different GEMM kernels by M: 2e-4 rel-L2 per tensor in fp32 mode, 1.5e-2 in bf16.  Where two runs launch the
same kernels on the same inputs (graph replay against eager, the dropout case) gradients may still differ in the order of
fp32 atomic adds (split-K weight gradients at token counts the grouped launch declines): 1e-5 rel-L2 bounds a reordered
fp32 sum of a few hundred terms (sqrt(n) * 2^-24 is about 1e-6) with room to spare."""
import pytest
import torch

from conftest import rel_l2
from oracle import favit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("D", [384, 100])
@pytest.mark.parametrize("n_in,a,b", [(11, 4, 1), (71, 37, 28)])
def test_rows_cut_fwd_bwd_bit_exact(K, n_in, a, b, D):
    B = 3
    g = torch.Generator(device=DEV).manual_seed(n_in * 1000 + D)
    x = torch.randn((B, n_in, D), generator=g, device=DEV)
    keep = list(range(a)) + list(range(n_in - b, n_in))
    y = K.rows_cut_fwd(x, B, n_in, a, b, D)
    assert y.shape == (B, a + b, D) and torch.equal(y, x[:, keep])
    dy = torch.randn((B, a + b, D), generator=g, device=DEV)
    ref = torch.zeros((B, n_in, D), device=DEV)
    ref[:, keep] = dy
    for lp in (torch.bfloat16, torch.float32, None):
        dx, dx_lp = K.rows_cut_bwd(dy, B, n_in, a, b, D, lp_dtype=lp)
        assert torch.equal(dx, ref)
        if lp is None:
            assert dx_lp is None
        else:
            assert dx_lp.dtype == lp and torch.equal(dx_lp, ref.to(lp))


def test_rows_cut_rejects_bad_ranges(K):
    x = torch.zeros((2, 5, 8), device=DEV)
    with pytest.raises(RuntimeError):
        K.rows_cut_fwd(x, 2, 5, 4, 2, 8)           # a + b > n_in
    with pytest.raises(RuntimeError):
        K.rows_cut_fwd(x, 2, 5, 0, 0, 8)


# ------------------------------------------------------------------ the small model, pruned against the full path
L, W, DEPTH, D, H, B = 50, 7, 4, 128, 2, 3


def _model(favit, seed=11, **kw):
    torch.manual_seed(seed)
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=112, patch_size=16, num_classes=10, embed_dim=D, depth=DEPTH,
                                                    num_heads=H, window_size=W, use_mhla=True, **kw)
    x = torch.randn(B, 3, 112, 112)
    y = torch.randint(0, 10, (B,))
    return m, x, y


class _CutCounter:
    def __init__(self, K, monkeypatch):
        self.n = 0
        orig = K.rows_cut_fwd

        def counted(*a, **k):
            self.n += 1
            return orig(*a, **k)
        monkeypatch.setattr(K, "rows_cut_fwd", counted)


def _run(favit, m, x, y):
    for p in m.parameters():
        p.grad = None
    logits = m(x)
    favit.train.cross_entropy(logits, y).backward()
    torch.cuda.synchronize()
    return logits.detach().float().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("mode,tol", [("fp32", 2e-4), ("bf16", 1.5e-2)])
def test_pruned_step_matches_full_path_and_oracle(favit, K, monkeypatch, mode, tol):
    favit.set_compute_dtype(mode)
    try:
        m, x, y = _model(favit)
        sd = {k: v.clone().requires_grad_(True) for k, v in m.state_dict().items()}
        m.to(DEV).train()                                    # dropout = 0: train == eval math, lse-saving attention
        xd, yd = x.to(DEV), y.to(DEV)
        cnt = _CutCounter(K, monkeypatch)
        monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
        lg_p, g_p = _run(favit, m, xd, yd)
        assert cnt.n == DEPTH, "every block of this model runs on fewer rows than the one below"
        monkeypatch.setenv("FAVIT_NO_PRUNE", "1")
        lg_f, g_f = _run(favit, m, xd, yd)
        assert cnt.n == DEPTH, "FAVIT_NO_PRUNE=1 takes the full path"
        e = rel_l2(lg_p, lg_f)
        print(f"\n[{mode}] logits pruned vs full rel-L2 {e:.2e}", end="")
        worst = (0.0, "")
        for k in g_f:
            worst = max(worst, (rel_l2(g_p[k], g_f[k]), k))
        print(f"; worst gradient {worst[0]:.2e} ({worst[1]})", end="")
        assert e < tol
        assert worst[0] < tol, worst
        a1, b1 = favit.functional.cls_plan(L, W, DEPTH)[0]
        for g in (g_p, g_f):
            assert torch.count_nonzero(g["pos_embed"][0, a1:L - b1]).item() == 0
            assert torch.count_nonzero(g["pos_embed"][0, :a1]).item() > 0
        if mode == "fp32":
            ref = O.vit_mhla_forward(x, sd, 16, H, W, True)
            O.cross_entropy(ref, y).backward()
            eo = rel_l2(lg_p.cpu(), ref.detach())
            wo = max((rel_l2(g_p[k].cpu(), sd[k].grad), k) for k in g_p)
            print(f"; vs oracle: logits {eo:.2e}, worst gradient {wo[0]:.2e} ({wo[1]})", end="")
            assert eo < tol
            assert wo[0] < tol, wo
    finally:
        favit.set_compute_dtype("fp32")


def test_lower_blocks_fall_back_to_all_rows(favit, K, monkeypatch):
    """depth 7 at L = 30: blocks 1 and 2 need every row, blocks 3 .. 7 run on 29, 23, 17, 11 and 5."""
    F = favit.functional
    Ls, depth = 30, 7
    plan = F.cls_plan(Ls, W, depth)
    assert plan[:2] == [None, None] and [sum(c) for c in plan[2:]] == [29, 23, 17, 11, 5]
    vit = favit.models.vit
    torch.manual_seed(5)
    blocks = torch.nn.ModuleList([favit.models.mhla.MHLATransformerBlock(64, 2, window_size=W) for _ in range(depth)]).to(DEV)
    norm = torch.nn.LayerNorm(64).to(DEV)
    x0 = torch.randn(2, Ls, 64, device=DEV)
    cnt = _CutCounter(K, monkeypatch)
    res = []
    for cls_only in (True, False):
        for p in blocks.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        t = vit.run_encoder(blocks, x, None, False, cls_only=cls_only)
        assert t.shape[1] == (5 if cls_only else Ls)
        out = F.run(F.FinalNormOp(), [t], [norm.weight, norm.bias])
        (out * torch.linspace(-1, 1, 64, device=DEV)).sum().backward()
        res.append((out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in blocks.parameters()]))
    assert cnt.n == 5
    (o1, gx1, gp1), (o2, gx2, gp2) = res
    assert rel_l2(o1, o2) < 2e-4 and rel_l2(gx1, gx2) < 2e-4
    assert max(rel_l2(a, b) for a, b in zip(gp1, gp2)) < 2e-4
    assert gx1.shape == (2, Ls, 64)


def test_active_dropout_takes_the_full_path(favit, K, monkeypatch):
    m, x, y = _model(favit, dropout=0.1)
    m.to(DEV).train()
    xd, yd = x.to(DEV), y.to(DEV)
    cnt = _CutCounter(K, monkeypatch)
    monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
    torch.manual_seed(99)
    lg_a, g_a = _run(favit, m, xd, yd)
    monkeypatch.setenv("FAVIT_NO_PRUNE", "1")
    torch.manual_seed(99)
    lg_b, g_b = _run(favit, m, xd, yd)
    assert cnt.n == 0
    assert torch.equal(lg_a, lg_b)
    assert max(rel_l2(g_a[k], g_b[k]) for k in g_a) < 1e-5
    m.eval()                                                  # the same model in eval mode: no dropout is active
    monkeypatch.delenv("FAVIT_NO_PRUNE")
    with torch.no_grad():
        m(xd)
    assert cnt.n == DEPTH


@pytest.mark.parametrize("segments", [1, 2])
def test_graphed_pruned_step_replays_match_eager(favit, K, monkeypatch, segments):
    """The captured step re-uses its buffers at every replay: the zeros of the cut rows have to be written by the
    replayed kernels themselves.  segments = 2: the backward is captured in two pieces, and the second encoder node
    starts from the rows the first one left (run_encoder slices the plan per node)."""
    favit.set_compute_dtype("bf16")
    try:
        m, x, y = _model(favit)
        other, _, _ = _model(favit)
        m.to(DEV).train(), other.to(DEV).train()
        xd, yd = x.to(DEV), y.to(DEV)
        mk = lambda mod: favit.train.FusedAdamW(favit.train.param_groups(mod, lr=0.0), lr=0.0, weight_decay=0.0, distributed=False)
        opt, oo = mk(m), mk(other)
        want = favit.train.train_step(other, xd, yd, oo).item()
        torch.cuda.synchronize()
        want_g = {k: p.grad.detach().clone() for k, p in other.named_parameters()}
        calls = {"fwd": [], "bwd": []}
        of, ob = K.rows_cut_fwd, K.rows_cut_bwd
        monkeypatch.setattr(K, "rows_cut_fwd", lambda *a, **k: (calls["fwd"].append(torch.cuda.is_current_stream_capturing()), of(*a, **k))[1])
        monkeypatch.setattr(K, "rows_cut_bwd", lambda *a, **k: (calls["bwd"].append(torch.cuda.is_current_stream_capturing()), ob(*a, **k))[1])
        step = favit.train.GraphedStep(m, opt, xd, yd, segments=segments)
        assert sum(calls["fwd"]) == DEPTH and sum(calls["bwd"]) == DEPTH, "the captured step runs the row cuts"
        n_host = (len(calls["fwd"]), len(calls["bwd"]))
        for _ in range(3):
            got = step(xd, yd).item()
            torch.cuda.synchronize()
            assert abs(got - want) < 1e-5 * abs(want)
            worst = max((rel_l2(p.grad, want_g[k]), k) for k, p in m.named_parameters())
            assert worst[0] < 1e-5, worst
        assert (len(calls["fwd"]), len(calls["bwd"])) == n_host, "replays launch nothing from the host"
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
