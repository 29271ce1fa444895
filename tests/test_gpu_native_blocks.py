"""Native block chains against the Python chains, in one process.

favit_mhla_block_fwd / _bwd issue the launches of the Python chains with the same arguments, so everything that does
not pass through fp32 atomics is compared with torch.equal: block outputs, the stream gradient, the LayerNorm partial
sums, and the weight gradients (at the token counts used here, 6 to 69, every weight-gradient GEMM is one direct launch
without K-splits).  Gradients that are summed with fp32 atomics in an order that varies from run to run (the
latent_proj fold into qkv / latent_proj, cls_token, pos_embed, the patch embedding) are held to what the Python path
shows against itself: it runs twice, and the native run may differ from it by ten times the worst relative difference
of those two runs, with a floor of 1e-6.  A gradient outside that list on which the two Python runs themselves
disagree is held to the same bound (it evidently is such a sum); none is known."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOMIC = ("latent_proj", "qkv", "cls_token", "pos_embed", "patch_embed")
FINAL_NORM = ("norm.weight", "norm.bias")       # FinalNormOp adds its dgamma / dbeta with the rows split eight ways: atomics too


def _atomic(name):
    return name in FINAL_NORM or any(a in name for a in ATOMIC)


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


@pytest.fixture()
def bf16(favit, monkeypatch):
    monkeypatch.delenv("FAVIT_NO_NATIVE_BLOCKS", raising=False)
    monkeypatch.delenv("FAVIT_NO_PRUNE", raising=False)
    favit.set_compute_dtype("bf16")
    favit.functional.set_native_blocks(True)
    yield favit.functional
    favit.functional.set_native_blocks(True)
    favit.set_compute_dtype("fp32")
    favit.functional.clear_lp_mirrors()


class _Calls:
    """Counts the calls of K.mhla_block_fwd / _bwd and how many of them the library took (returned 0)."""

    def __init__(self, K, monkeypatch):
        self.fwd, self.bwd, self.fwd_ok, self.bwd_ok, self.capturing = 0, 0, 0, 0, 0
        of, ob = K.mhla_block_fwd, K.mhla_block_bwd

        def fwd(*a, **k):
            rc = of(*a, **k)
            self.fwd += 1
            self.fwd_ok += rc == 0
            self.capturing += torch.cuda.is_current_stream_capturing()
            return rc

        def bwd(*a, **k):
            rc = ob(*a, **k)
            self.bwd += 1
            self.bwd_ok += rc == 0
            return rc
        monkeypatch.setattr(K, "mhla_block_fwd", fwd)
        monkeypatch.setattr(K, "mhla_block_bwd", bwd)

    def reset(self):
        self.fwd = self.bwd = self.fwd_ok = self.bwd_ok = self.capturing = 0


def _check_grads(native, py1, py2):
    """native against the first Python run, by the rule of the module docstring."""
    worst = max(rel_l2(py2[k], py1[k]) for k in py1)
    tol = max(10.0 * worst, 1e-6)
    print(f"\nPython path against itself: worst rel-L2 {worst:.2e}; atomic-sum tolerance {tol:.2e}", end="")
    for k in py1:
        if _atomic(k) or not torch.equal(py1[k], py2[k]):
            e = rel_l2(native[k], py1[k])
            assert e <= tol, (k, e, tol)
        else:
            assert torch.equal(native[k], py1[k]), k


# ------------------------------------------------------------------ EncoderOp through run_encoder
def _encoder(favit, B, L, D, H, W, depth, seed=3):
    torch.manual_seed(seed)
    blocks = torch.nn.ModuleList([favit.models.mhla.MHLATransformerBlock(D, H, window_size=W) for _ in range(depth)]).to(DEV)
    x0 = torch.randn(B, L, D, device=DEV)
    return blocks, x0


def _run_encoder(favit, K, monkeypatch, blocks, x0, between=None, grad_buffers=True):
    """Forward + backward of the CLS-only encoder; returns (output, stream gradient, LayerNorm partial sums, parameter
    gradients by name).  grad_buffers: parameters own zeroed fp32 .grad buffers, as under the fused optimizer (the
    kernels accumulate into them).  between(): called between forward and backward."""
    for p in blocks.parameters():
        p.grad = torch.zeros_like(p) if grad_buffers else None
    parts = []
    orig = K.reduce_rows_multi
    monkeypatch.setattr(K, "reduce_rows_multi", lambda es: (parts.extend(e[0].clone() for e in es), orig(es))[1])
    try:
        x = x0.clone().requires_grad_(True)
        t = favit.models.vit.run_encoder(blocks, x, None, True, cls_only=True)
        w = torch.linspace(-1, 1, t.numel(), device=DEV).reshape(t.shape)
        if between is not None:
            between()
        (t * w).sum().backward()
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(K, "reduce_rows_multi", orig)
    return t.detach().clone(), x.grad.clone(), parts, {k: p.grad.clone() for k, p in blocks.named_parameters()}


ENCODERS = [
    # (B, L, D, H, W, depth), native blocks: every block whose row count the lse attention kernels take (n >= W + 1)
    ((3, 17, 128, 2, 7, 3), 2),        # rows 17 (all), 11, 5: odd row counts, the half-wave LayerNorm's dead half
    ((2, 30, 192, 3, 3, 5), 4),        # rows 11, 9, 7, 5, 3: D = 192 leaves the last LayerNorm vector half filled; h = 1
]


@pytest.mark.parametrize("shape,n_native", ENCODERS)
def test_encoder_on_off_bit_identical(favit, K, bf16, monkeypatch, shape, n_native):
    F = bf16
    blocks, x0 = _encoder(favit, *shape)
    calls = _Calls(K, monkeypatch)
    F.set_native_blocks(False)
    o1, gx1, parts1, g1 = _run_encoder(favit, K, monkeypatch, blocks, x0)
    o2, gx2, parts2, g2 = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert calls.fwd == 0 and calls.bwd == 0
    F.set_native_blocks(True)
    on, gxn, partsn, gn = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert (calls.fwd_ok, calls.bwd_ok) == (n_native, n_native), "the native chains ran for every block they can take"
    assert calls.fwd == n_native and calls.bwd == n_native, "no call was declined: the plan query filters the geometry"
    assert torch.equal(on, o1) and torch.equal(gxn, gx1)
    assert len(partsn) == len(parts1) == 2 * shape[5]
    for a, b in zip(partsn, parts1):
        assert a.shape == b.shape and torch.equal(a, b)
    _check_grads(gn, g1, g2)


def test_mixed_directions(favit, K, bf16, monkeypatch):
    """A native forward followed by the Python backward (its tape hands out views of the one allocation), and a Python
    forward followed by a backward with the switch on, which has no native tape and takes the Python chains."""
    F = bf16
    shape = ENCODERS[0][0]
    blocks, x0 = _encoder(favit, *shape)
    calls = _Calls(K, monkeypatch)
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0)
    ref2 = _run_encoder(favit, K, monkeypatch, blocks, x0)
    for first in (True, False):
        calls.reset()
        F.set_native_blocks(first)
        got = _run_encoder(favit, K, monkeypatch, blocks, x0, between=lambda: F.set_native_blocks(not first))
        assert calls.fwd_ok == (2 if first else 0) and calls.bwd == 0
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        assert all(torch.equal(a, b) for a, b in zip(got[2], ref[2])) and len(got[2]) == len(ref[2])
        _check_grads(got[3], ref[3], ref2[3])


def test_parameters_without_gradient_buffers_take_the_python_backward(favit, K, bf16, monkeypatch):
    F = bf16
    blocks, x0 = _encoder(favit, *ENCODERS[0][0])
    calls = _Calls(K, monkeypatch)
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=False)
    ref2 = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=False)
    F.set_native_blocks(True)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=False)
    assert calls.fwd_ok == 2 and calls.bwd == 0
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    _check_grads(got[3], ref[3], ref2[3])


def test_declined_calls_launch_nothing_and_the_python_path_runs(favit, K, bf16, monkeypatch):
    F, A = bf16, favit._abi
    B, L, D, H, W, depth = ENCODERS[0][0]
    # the library itself: a tape one byte short is refused and not a byte of it is written
    plan = K.mhla_block_plan(B, L, D, H, W, 4 * D, True)
    assert K.mhla_block_plan(B, L, 96, 2, W, 384, True) is None and K.mhla_block_plan(B, 5, D, H, W, 4 * D, True) is None
    g = torch.Generator(device=DEV).manual_seed(1)
    f32 = lambda *s: torch.randn(*s, generator=g, device=DEV)
    bf = lambda *s: f32(*s).to(torch.bfloat16)
    x = f32(B * L, D)
    args = (f32(D), f32(D), f32(D), f32(D), bf(3 * D, D), f32(3 * D), bf(D, D), f32(D), bf(4 * D, D), f32(4 * D), bf(D, 4 * D), f32(D))
    tape = torch.full((plan.tape_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    assert K.mhla_block_fwd(plan, x, tape[:-1], *args) == A.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((tape == 0xA5).all())
    arena = torch.full((plan.bwd_bytes[1],), 0xA5, dtype=torch.uint8, device=DEV)
    gg = f32(B * L, D)
    bwd = lambda t, a: K.mhla_block_bwd(plan, x, t, args[0], args[2], args[4], args[6], args[8], args[10], gg, gg.to(torch.bfloat16), a, True)
    assert bwd(tape[:-1], arena) == A.ERR_INVALID and bwd(tape, arena[:-1]) == A.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((tape == 0xA5).all()) and bool((arena == 0xA5).all())
    # EncoderOp: every call declined (the tape handed over is one byte short) -> the Python chains produce the result
    blocks, x0 = _encoder(favit, B, L, D, H, W, depth)
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0)
    ref2 = _run_encoder(favit, K, monkeypatch, blocks, x0)
    F.set_native_blocks(True)
    real = K.mhla_block_fwd
    monkeypatch.setattr(K, "mhla_block_fwd", lambda plan, x, tape, *a: real(plan, x, tape[:-1], *a))
    calls = _Calls(K, monkeypatch)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert calls.fwd == 2 and calls.fwd_ok == 0 and calls.bwd == 0
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    _check_grads(got[3], ref[3], ref2[3])
    # a width the chains do not take (D = 96): no call at all
    calls.reset()
    blocks, x0 = _encoder(favit, 2, 17, 96, 6, 7, 2)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0)
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert calls.fwd == 0 and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


# ------------------------------------------------------------------ the small model of test_gpu_cls_only.py
L, W, DEPTH, D, H, B = 50, 7, 4, 128, 2, 3
N_NATIVE = 3                                    # rows 23, 17, 11 and 5: the last block is below the lse kernels' W + 1


def _model(favit, seed=11, **kw):
    torch.manual_seed(seed)
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=112, patch_size=16, num_classes=10, embed_dim=D, depth=DEPTH,
                                                    num_heads=H, window_size=W, use_mhla=True, **kw)
    x = torch.randn(B, 3, 112, 112)
    y = torch.randint(0, 10, (B,))
    return m.to(DEV), x.to(DEV), y.to(DEV)


def _opt(favit, m):
    return favit.train.FusedAdamW(favit.train.param_groups(m, lr=0.0), lr=0.0, weight_decay=0.0, distributed=False)


def _step(favit, m, opt, x, y):
    loss = favit.train.train_step(m, x, y, opt).detach().clone()
    torch.cuda.synchronize()
    return loss, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def test_train_step_on_off(favit, K, bf16, monkeypatch):
    F = bf16
    m, x, y = _model(favit)
    m.train()
    opt = _opt(favit, m)                        # lr = 0: the three steps start from the same weights
    calls = _Calls(K, monkeypatch)
    F.set_native_blocks(False)
    l1, g1 = _step(favit, m, opt, x, y)
    l2, g2 = _step(favit, m, opt, x, y)
    assert calls.fwd == 0
    F.set_native_blocks(True)
    ln, gn = _step(favit, m, opt, x, y)
    assert (calls.fwd_ok, calls.bwd_ok) == (N_NATIVE, N_NATIVE)
    assert torch.equal(ln, l1) and torch.equal(l2, l1)
    _check_grads(gn, g1, g2)


def test_eval_no_grad_logits_bit_identical(favit, K, bf16, monkeypatch):
    F = bf16
    m, x, _ = _model(favit)
    m.eval()
    calls = _Calls(K, monkeypatch)
    with torch.no_grad():
        F.set_native_blocks(False)
        ref = m(x).clone()
        F.set_native_blocks(True)
        got = m(x).clone()
    assert calls.fwd_ok == N_NATIVE and calls.bwd == 0
    assert torch.equal(got, ref)
    plans = [p for p in m.blocks[0].norm1.weight._favit_blocks.values() if p is not None]
    assert plans and all(p.off["lse"][1] == 0 for p in plans), "the eval-mode tape has no lse"


@pytest.mark.parametrize("how", ["fp32", "dropout", "gemm_trace", "env"])
def test_fallbacks(favit, K, bf16, monkeypatch, how):
    """Where the native chains do not apply nothing calls them, and the result is the one of the switch turned off."""
    F = bf16
    m, x, y = _model(favit, **({"dropout": 0.1} if how == "dropout" else {}))
    m.train()
    if how == "fp32":
        favit.set_compute_dtype("fp32")
    if how == "env":
        monkeypatch.setenv("FAVIT_NO_NATIVE_BLOCKS", "1")
    calls = _Calls(K, monkeypatch)
    res, traces = [], []
    for on in (True, False):
        F.set_native_blocks(on)
        if how == "gemm_trace":
            monkeypatch.setattr(K, "GEMM_TRACE", [])
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(99)                   # (the dropout seeds are drawn from torch's CPU generator)
        logits = m(x)
        favit.train.cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        res.append((logits.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
        if how == "gemm_trace":
            traces.append([(e[3], e[4]) for e in K.GEMM_TRACE])
            monkeypatch.setattr(K, "GEMM_TRACE", None)
    assert calls.fwd == 0 and calls.bwd == 0
    assert torch.equal(res[0][0], res[1][0])
    assert max(rel_l2(res[0][1][k], res[1][1][k]) for k in res[0][1]) < 1e-5    # (fp32 atomics: test_gpu_cls_only.py)
    if how == "gemm_trace":
        assert traces[0] == traces[1]
        rows = [23, 17, 11, 5]
        for n in rows:                          # every block's four forward and four input-gradient GEMMs are listed
            Mb = B * n
            for shp in ((Mb, 3 * D, D, 1), (Mb, D, D, 1), (Mb, 4 * D, D, 1), (Mb, D, 4 * D, 1), (Mb, D, 3 * D, 1)):
                assert any(s == shp for _, s in traces[0]), shp
            assert sum(s == (Mb, D, D, 1) for _, s in traces[0]) >= 2 and sum(s == (Mb, 4 * D, D, 1) for _, s in traces[0]) >= 2


@pytest.mark.parametrize("segments", [1, 2])
def test_graphed_step_replays_match_the_eager_native_step(favit, K, bf16, monkeypatch, segments):
    m, x, y = _model(favit)
    other, _, _ = _model(favit)
    m.train(), other.train()
    opt, oo = _opt(favit, m), _opt(favit, other)
    calls = _Calls(K, monkeypatch)
    want, want_g = _step(favit, other, oo, x, y)
    assert (calls.fwd_ok, calls.bwd_ok) == (N_NATIVE, N_NATIVE)
    calls.reset()
    step = favit.train.GraphedStep(m, opt, x, y, segments=segments)
    assert calls.capturing == N_NATIVE, "the captured step holds the native chains"
    n_host = (calls.fwd, calls.bwd)
    assert calls.fwd == calls.fwd_ok and calls.bwd == calls.bwd_ok and calls.bwd_ok == calls.fwd_ok
    for _ in range(3):
        got = step(x, y)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        for k, p in m.named_parameters():
            if _atomic(k):
                assert rel_l2(p.grad, want_g[k]) < 1e-5, k     # (a reordered fp32 sum: the bound of test_gpu_cls_only.py)
            else:
                assert torch.equal(p.grad, want_g[k]), k
    assert (calls.fwd, calls.bwd) == n_host, "replays launch nothing from the host"
