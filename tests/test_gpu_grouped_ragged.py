"""The ragged grouped weight-gradient launch (favit_gemm_grouped_tn_ragged: problems whose token counts differ, K-splits
planned per chunk) and the ragged LayerNorm partial-sum fold (favit_reduce_rows_multi_ragged) on the GPU, then both at
model level: a pruned encoder whose blocks share launches.

A "block" is four problems dY [T, 3D | D | 4D | D] against X [T, D | D | D | 4D] at D = 128 (9 tiles).  Bounds:
2e-5 rel-L2 against fp64 for dW / db, the bound of the grouped tests in test_gpu_fullsize.py (bf16 products are exact in
fp32; what is left is the rounding of an fp32 sum of T terms).  Run to run, dW is bitwise equal (slabs added in split
order, or one accumulation chain), and so is db: through slabs where the chunk is split, and as ONE fp32 atomic addend
per row onto the same start value where it is not -- a single addend is exact, the rule test_gpu_fullsize.py states."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


def _rand(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, generator=gen, device=DEV, dtype=torch.float32) * scale).to(dtype)


def _block(T, gen, accumulate, want_db=True, pad=0):
    """(problems, fp64 references, start values) of one block; pad: extra columns in dW's row stride."""
    probs, refs, start = [], [], []
    for N, Kd in [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]:
        dy = _rand((T, N), torch.bfloat16, gen, 0.5)
        x = _rand((T, Kd), torch.bfloat16, gen)
        full = _rand((N, Kd + pad), torch.float32, gen) if accumulate else torch.full((N, Kd + pad), float("nan"), device=DEV)
        db0 = _rand((N,), torch.float32, gen) if accumulate else torch.zeros(N, device=DEV)
        start.append((full.clone(), db0.clone()))
        dw = full[:, :Kd]
        db = db0 if want_db else None
        probs.append((dy, x, dw, db, accumulate))
        ref_w = dy.double().t() @ x.double()
        if accumulate:
            ref_w = ref_w + start[-1][0][:, :Kd].double()
        refs.append((ref_w, dy.double().sum(0) + start[-1][1].double()))
    return probs, refs, start


def _group(Ts, seed, accumulate, want_db=True, pad=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    probs, refs, start = [], [], []
    for T in Ts:
        p, r, s = _block(T, gen, accumulate, want_db, pad)
        probs += p
        refs += r
        start += s
    return probs, refs, start


def _restore(probs, start):
    for (dy, x, dw, db, _), (w0, b0) in zip(probs, start):
        dw.copy_(w0[:, :dw.shape[1]])
        if db is not None:
            db.copy_(b0)


def _splits(favit):
    return int(favit._abi.lib().favit_gemm_grouped_last_splits())


@pytest.mark.parametrize("want_db", [True, False])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("Ts,split", [((160, 352, 2048), None), ((12800, 160), True)])
def test_ragged_group_against_fp64_and_run_to_run(K, favit, Ts, split, accumulate, want_db):
    """Three blocks of different token counts in one launch; and 12,800 tokens (over the planner's 6,400-token cap: that
    chunk is split, through slabs) beside 160 (one direct-writing unit)."""
    probs, refs, start = _group(Ts, sum(Ts) + 2 * accumulate + want_db, accumulate, want_db)
    assert K.gemm_grouped_tn_ragged(probs)
    if split:
        assert _splits(favit) > 1
    torch.cuda.synchronize()
    for (dy, x, dw, db, _), (ref_w, ref_b) in zip(probs, refs):
        assert torch.isfinite(dw).all()
        e = rel_l2(dw, ref_w)
        assert e < 2e-5, (dy.shape[0], tuple(dw.shape), e)
        if db is not None:
            e = rel_l2(db, ref_b)
            assert e < 2e-5, (dy.shape[0], tuple(dw.shape), e)
    first = [(p[2].clone(), p[3].clone() if p[3] is not None else None) for p in probs]
    _restore(probs, start)
    assert K.gemm_grouped_tn_ragged(probs)
    torch.cuda.synchronize()
    for p, (w1, b1) in zip(probs, first):
        assert torch.equal(p[2], w1), "weight gradients must be bitwise reproducible"
        if b1 is not None:
            assert torch.equal(p[3], b1)      # split chunk: slabs in split order; one split: a single addend per row, exact


@pytest.mark.parametrize("Ts", [(2048,) * 3, (12800,) * 2])
def test_uniform_group_equals_the_uniform_entry_point(K, favit, Ts):
    """One token count: the ragged entry point plans what favit_gemm_grouped_tn plans -- same split count, same bits."""
    probs, _, start = _group(Ts, 7, True)
    assert K.gemm_grouped_tn(probs)
    s_old = _splits(favit)
    old = [(p[2].clone(), p[3].clone()) for p in probs]
    _restore(probs, start)
    assert K.gemm_grouped_tn_ragged(probs)
    assert _splits(favit) == s_old
    torch.cuda.synchronize()
    for p, (w, b) in zip(probs, old):
        assert torch.equal(p[2], w) and torch.equal(p[3], b)


def test_no_cross_talk_between_chunks(K, favit):
    """Padded ldc; the destination of one problem holds a sentinel.  A non-accumulating launch leaves no sentinel, and
    nothing outside any problem's [M, N] window changes (the pad columns keep their start values)."""
    pad, sentinel = 8, 12345.0
    probs, refs, start = _group((12800, 160, 352), 9, False, True, pad)
    assert K.gemm_grouped_tn_ragged(probs)
    assert _splits(favit) > 1
    torch.cuda.synchronize()
    clean = [p[2].clone() for p in probs]
    fulls = []
    for i, ((dy, x, dw, db, _), (w0, b0)) in enumerate(zip(probs, start)):
        full = dw._base if dw._base is not None else dw
        full.copy_(w0)                                    # NaN window and NaN pad again
        full[:, dw.shape[1]:] = float(i + 1)             # the pad columns: a known value per problem
        db.copy_(b0)
        fulls.append(full)
    victim = 5                                            # (the second problem of the 160-token block)
    probs[victim][2].fill_(sentinel)
    assert K.gemm_grouped_tn_ragged(probs)
    torch.cuda.synchronize()
    for i, ((dy, x, dw, db, _), full) in enumerate(zip(probs, fulls)):
        assert not (dw == sentinel).any()
        assert torch.equal(dw, clean[i]), i
        assert (full[:, dw.shape[1]:] == float(i + 1)).all(), f"problem {i}: a store left its [M, N] window"


def test_refusals_leave_destinations_untouched(K, favit):
    probs, _, _ = _group((160, 352), 3, True)
    bad, _, _ = _block(176, torch.Generator(device=DEV).manual_seed(4), True)       # 176 % 32 != 0
    mixed = probs[:5] + [bad[1]] + probs[6:]
    before = [(p[2].clone(), p[3].clone()) for p in mixed]
    assert K.gemm_grouped_tn_ragged(mixed) is False
    many = (probs * 7)[:K.GROUP_MAX + 1]
    assert K.gemm_grouped_tn_ragged(many) is False
    # the library itself: more than GROUP_MAX problems is an invalid call
    abi = favit._abi
    arr = (abi.GemmDesc * (K.GROUP_MAX + 1))()
    assert abi.lib().favit_gemm_grouped_tn_ragged(arr, K.GROUP_MAX + 1, None) == abi.ERR_INVALID
    torch.cuda.synchronize()
    for p, (w, b) in zip(mixed, before):
        assert torch.equal(p[2], w) and torch.equal(p[3], b)


def test_reduce_rows_multi_ragged(K):
    """3, 40, 511, 512 and 1,030 rows x 128 columns in one launch.  Below 512 rows an entry is one deterministic sum,
    identical to a launch of its own; from 512 rows eight partial sums are added atomically (order-dependent): 2e-5
    against fp64, the bound of test_reduce_rows_multi."""
    gen = torch.Generator(device=DEV).manual_seed(17)
    rows, cols = [3, 40, 511, 512, 1030], 128
    parts = [torch.randn((2, r, cols), generator=gen, device=DEV) + 0.5 for r in rows]
    s0 = [torch.randn(cols, generator=gen, device=DEV) for _ in rows]
    s1 = [torch.randn(cols, generator=gen, device=DEV) for _ in rows]
    refs = [(a.double() + p[0].double().sum(0), b.double() + p[1].double().sum(0)) for p, a, b in zip(parts, s0, s1)]
    alone = [(a.clone(), b.clone()) for a, b in zip(s0, s1)]
    for p, (a, b) in zip(parts, alone):
        K.reduce_rows_multi([(p, a, b)])
    for fn in (K.reduce_rows_multi_ragged, K.reduce_rows_multi):       # (the one-shape form hands mixed row counts on)
        outs = [(a.clone(), b.clone()) for a, b in zip(s0, s1)]
        fn([(p, a, b) for p, (a, b) in zip(parts, outs)])
        torch.cuda.synchronize()
        for r, got, one, ref in zip(rows, outs, alone, refs):
            if r < 512:
                assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]), r
            assert rel_l2(got[0], ref[0]) < 2e-5 and rel_l2(got[1], ref[1]) < 2e-5, r


# ------------------------------------------------------------------ model level (the small model of test_gpu_cls_only.py)
L, W, DEPTH, H, B = 50, 7, 4, 2, 32       # B = 32: every block's token count (32 x 23, 17, 11, 5) is a multiple of 32


def _model(favit, seed=11):
    torch.manual_seed(seed)
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=112, patch_size=16, num_classes=10, embed_dim=D, depth=DEPTH,
                                                    num_heads=H, window_size=W, use_mhla=True)
    return m, torch.randn(B, 3, 112, 112), torch.randint(0, 10, (B,))


class _Counter:
    def __init__(self, K, monkeypatch, name):
        self.n, self.capturing, self.sizes = 0, 0, []
        orig = getattr(K, name)

        def counted(problems, *a, **k):
            ok = orig(problems, *a, **k)
            self.n += 1
            self.capturing += torch.cuda.is_current_stream_capturing()
            self.sizes.append((len(problems), ok))
            return ok
        monkeypatch.setattr(K, name, counted)


def _fused_step_grads(favit, m, xd, yd):
    """One step of the fused-optimizer flow (parameters own gradient buffers, so the latent_proj fold is deferred and
    the weight gradients may wait for further blocks); lr = 0: the gradients are the result."""
    opt = favit.train.FusedAdamW(favit.train.param_groups(m, lr=0.0), lr=0.0, weight_decay=0.0, distributed=False)
    favit.train.train_step(m, xd, yd, opt)
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def test_pruned_backward_groups_across_blocks(favit, K, monkeypatch):
    favit.set_compute_dtype("bf16")
    try:
        m, x, y = _model(favit)
        other, _, _ = _model(favit)
        m.to(DEV).train(), other.to(DEV).train()
        xd, yd = x.to(DEV), y.to(DEV)
        monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
        monkeypatch.delenv("FAVIT_WGRAD_PER_BLOCK", raising=False)
        cnt = _Counter(K, monkeypatch, "gemm_grouped_tn_ragged")
        g_new = _fused_step_grads(favit, m, xd, yd)
        assert 0 < cnt.n < DEPTH, cnt.sizes
        assert all(ok for _, ok in cnt.sizes), "the library took every ragged list"
        assert sum(n for n, _ in cnt.sizes) == 4 * DEPTH
        monkeypatch.setenv("FAVIT_WGRAD_PER_BLOCK", "1")
        n0 = cnt.n
        g_old = _fused_step_grads(favit, other, xd, yd)
        assert cnt.n == n0, "FAVIT_WGRAD_PER_BLOCK=1 keeps one uniform launch per block"
        worst = max((rel_l2(g_new[k], g_old[k]), k) for k in g_old)
        print(f"\ngrouped across blocks vs per block: worst gradient rel-L2 {worst[0]:.2e} ({worst[1]})", end="")
        assert worst[0] < 1.5e-2, worst
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


@pytest.mark.parametrize("segments", [1, 2])
def test_graphed_pruned_step_with_ragged_launches(favit, K, monkeypatch, segments):
    favit.set_compute_dtype("bf16")
    try:
        m, x, y = _model(favit)
        other, _, _ = _model(favit)
        m.to(DEV).train(), other.to(DEV).train()
        xd, yd = x.to(DEV), y.to(DEV)
        mk = lambda mod: favit.train.FusedAdamW(favit.train.param_groups(mod, lr=0.0), lr=0.0, weight_decay=0.0, distributed=False)
        opt, oo = mk(m), mk(other)
        monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
        monkeypatch.delenv("FAVIT_WGRAD_PER_BLOCK", raising=False)
        want = favit.train.train_step(other, xd, yd, oo).item()
        torch.cuda.synchronize()
        want_g = {k: p.grad.detach().clone() for k, p in other.named_parameters()}
        cnt = _Counter(K, monkeypatch, "gemm_grouped_tn_ragged")
        step = favit.train.GraphedStep(m, opt, xd, yd, segments=segments)
        assert cnt.capturing > 0, "the captured backward issues the ragged launch"
        n_host = cnt.n
        for _ in range(3):
            got = step(xd, yd).item()
            torch.cuda.synchronize()
            assert abs(got - want) < 1e-5 * abs(want)
            worst = max((rel_l2(p.grad, want_g[k]), k) for k, p in m.named_parameters())
            assert worst[0] < 1e-5, worst
        assert cnt.n == n_host, "replays launch nothing from the host"
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
