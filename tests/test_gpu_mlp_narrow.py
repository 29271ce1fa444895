"""Narrowed MLP halves on the GPU: every block of a CLS-only encoder runs LayerNorm 2, fc1, fc2 and
their backward on the rows the NEXT block reads, with the row cut inside the block instead of in front of the next one.

Bounds.  Narrowed against FAVIT_NO_MLP_NARROW=1 (and against the full path and the oracle): the MLP-half GEMMs run at
another M and the fc1 / fc2 weight gradients sum over another K, so kernels may be chosen differently -- the project's
consistency bounds for that, 2e-4 rel-L2 per tensor in fp32 mode and 1.5e-2 in bf16 (tests/test_gpu_cls_only.py).
Native against Python on the narrowed path: the same launches with the same arguments, torch.equal, and for sums made
with fp32 atomics the rule of tests/test_gpu_native_blocks.py (ten times what the Python path shows against itself,
floor 1e-6).  Graph replay against eager: 1e-5, as in the existing graph tests.

K.GEMM_TRACE holds every block on one row count (functional.mlp_narrow_on: tests/test_gpu_native_blocks.py looks every
GEMM of a block up under the block's own rows in such a trace), so the shapes the narrowed GEMMs ran at are recorded
here by wrapping K.gemm and the grouped weight-gradient launches instead."""
import pytest
import torch

from conftest import rel_l2
from oracle import favit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOMIC = ("latent_proj", "qkv", "cls_token", "pos_embed", "patch_embed", "norm.weight", "norm.bias")


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


@pytest.fixture()
def env(favit, monkeypatch):
    for k in ("FAVIT_NO_NATIVE_BLOCKS", "FAVIT_NO_PRUNE", "FAVIT_NO_MLP_NARROW"):
        monkeypatch.delenv(k, raising=False)
    favit.functional.set_native_blocks(True)
    yield favit.functional
    favit.functional.set_native_blocks(True)
    favit.set_compute_dtype("fp32")
    favit.functional.clear_lp_mirrors()


class _Calls:
    """Calls of the four block entry points, how many the library took, and the row cuts in both directions."""
    NAMES = ("mhla_block_fwd", "mhla_block_mlp_fwd", "mhla_block_mlp_bwd", "mhla_block_bwd")

    def __init__(self, K, monkeypatch):
        self.n, self.ok, self.cut_f, self.cut_b, self.capturing = {}, {}, 0, 0, 0
        self.reset()
        for name in self.NAMES:
            monkeypatch.setattr(K, name, self._wrap(name, getattr(K, name)))
        of, ob = K.rows_cut_fwd, K.rows_cut_bwd

        def cf(*a, **k):
            self.cut_f += 1
            return of(*a, **k)

        def cb(*a, **k):
            self.cut_b += 1
            return ob(*a, **k)
        monkeypatch.setattr(K, "rows_cut_fwd", cf)
        monkeypatch.setattr(K, "rows_cut_bwd", cb)

    def _wrap(self, name, fn):
        def w(*a, **k):
            rc = fn(*a, **k)
            self.n[name] += 1
            self.ok[name] += rc == 0
            self.capturing += torch.cuda.is_current_stream_capturing()
            return rc
        return w

    def reset(self):
        self.n, self.ok = {k: 0 for k in self.NAMES}, {k: 0 for k in self.NAMES}
        self.cut_f = self.cut_b = self.capturing = 0

    def all_ok(self, fwd, mlp, bwd=True):
        want = {"mhla_block_fwd": fwd, "mhla_block_mlp_fwd": mlp, "mhla_block_mlp_bwd": mlp if bwd else 0,
                "mhla_block_bwd": fwd if bwd else 0}
        return self.n == want and self.ok == want


# ------------------------------------------------------------------ encoders through run_encoder
# (B, L, D, H, W, depth), native blocks, of them with a narrowed MLP half
ENCODERS = [
    ((3, 17, 128, 2, 7, 3), 2, 2),        # rows 17 (all) / 11 / 5: MLP halves on 11, 5, 5
    ((2, 30, 192, 3, 3, 5), 4, 4),        # rows 11, 9, 7, 5, 3: MLP halves on 9, 7, 5, 3, 3
]


def _encoder(favit, B, L, D, H, W, depth, seed=3):
    torch.manual_seed(seed)
    blocks = torch.nn.ModuleList([favit.models.mhla.MHLATransformerBlock(D, H, window_size=W) for _ in range(depth)]).to(DEV)
    return blocks, torch.randn(B, L, D, device=DEV)


def _run_encoder(favit, K, monkeypatch, blocks, x0, between=None, grad_buffers=True):
    """(output, stream gradient, LayerNorm partial sums, parameter gradients) of the CLS-only encoder.
    grad_buffers: True / False for all parameters, or a predicate of the parameter's name."""
    has = grad_buffers if callable(grad_buffers) else (lambda name: grad_buffers)
    for k, p in blocks.named_parameters():
        p.grad = torch.zeros_like(p) if has(k) else None
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


def _check_grads(native, py1, py2):
    worst = max(rel_l2(py2[k], py1[k]) for k in py1)
    tol = max(10.0 * worst, 1e-6)
    print(f"\nPython path against itself: worst rel-L2 {worst:.2e}; atomic-sum tolerance {tol:.2e}", end="")
    for k in py1:
        if any(a in k for a in ATOMIC) or not torch.equal(py1[k], py2[k]):
            e = rel_l2(native[k], py1[k])
            assert e <= tol, (k, e, tol)
        else:
            assert torch.equal(native[k], py1[k]), k


def _same(got, ref, ref2):
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert len(got[2]) == len(ref[2])
    for a, b in zip(got[2], ref[2]):
        assert a.shape == b.shape and torch.equal(a, b)
    _check_grads(got[3], ref[3], ref2[3])


@pytest.mark.parametrize("mode,tol", [("fp32", 2e-4), ("bf16", 1.5e-2)])
@pytest.mark.parametrize("shape", [e[0] for e in ENCODERS])
def test_encoder_narrowed_against_switch_off(favit, K, env, monkeypatch, shape, mode, tol):
    favit.set_compute_dtype(mode)
    blocks, x0 = _encoder(favit, *shape)
    calls = _Calls(K, monkeypatch)
    nar = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=False)
    cuts_n = (calls.cut_f, calls.cut_b)
    calls.reset()
    monkeypatch.setenv("FAVIT_NO_MLP_NARROW", "1")
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=False)
    assert calls.ok["mhla_block_mlp_fwd"] == 0 and calls.n["mhla_block_mlp_bwd"] == 0
    assert cuts_n == (calls.cut_f, calls.cut_b) and cuts_n[0] == cuts_n[1] > 0, "the cuts move, their number stays"
    assert nar[0].shape == ref[0].shape and nar[0].shape[1] == (5 if shape[4] == 7 else 3)
    eo, eg = rel_l2(nar[0], ref[0]), rel_l2(nar[1], ref[1])
    worst = max((rel_l2(nar[3][k], ref[3][k]), k) for k in ref[3])
    print(f"\n[{mode} {shape}] narrowed vs switch off: output {eo:.2e} (bit-identical: {torch.equal(nar[0], ref[0])}), "
          f"stream gradient {eg:.2e}, worst parameter gradient {worst[0]:.2e} ({worst[1]})", end="")
    assert eo < tol and eg < tol
    assert worst[0] < tol, worst
    # rows the block above never reads carry no gradient in either run
    assert torch.equal(nar[1] == 0, ref[1] == 0)


@pytest.mark.parametrize("shape,n_native,n_narrow", ENCODERS)
def test_native_against_python_on_the_narrowed_path(favit, K, env, monkeypatch, shape, n_native, n_narrow):
    F = env
    favit.set_compute_dtype("bf16")
    blocks, x0 = _encoder(favit, *shape)
    calls = _Calls(K, monkeypatch)
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0)
    ref2 = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert sum(calls.n.values()) == 0
    n_cuts = calls.cut_f // 2
    calls.reset()
    F.set_native_blocks(True)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert calls.all_ok(n_native, n_narrow), (calls.n, calls.ok)
    assert (calls.cut_f, calls.cut_b) == (n_cuts, n_cuts), "every cut stays a Python-visible call"
    assert len(got[2]) == 2 * shape[5]
    _same(got, ref, ref2)
    # a native forward with the Python backward: the tape hands out views on two row counts
    calls.reset()
    got = _run_encoder(favit, K, monkeypatch, blocks, x0, between=lambda: F.set_native_blocks(False))
    assert calls.all_ok(n_native, n_narrow, bwd=False), (calls.n, calls.ok)
    _same(got, ref, ref2)


def test_declined_mlp_half_calls_launch_nothing_and_the_python_half_runs(favit, K, env, monkeypatch):
    F, A = env, favit._abi
    favit.set_compute_dtype("bf16")
    B, L, D, H, W, depth = ENCODERS[0][0]
    n_mlp = 11
    plan = K.mhla_block_plan(B, L, D, H, W, 4 * D, True, n_mlp=n_mlp)
    g = torch.Generator(device=DEV).manual_seed(1)
    f32 = lambda *s: torch.randn(*s, generator=g, device=DEV)
    bf = lambda *s: f32(*s).to(torch.bfloat16)
    x = f32(B * L, D)
    args = (f32(D), f32(D), f32(D), f32(D), bf(3 * D, D), f32(3 * D), bf(D, D), f32(D), bf(4 * D, D), f32(4 * D), bf(D, 4 * D), f32(D))
    pad = f32(B * n_mlp * D + 4)
    x1c, x1c_odd = pad[:B * n_mlp * D].reshape(B * n_mlp, D), pad[1:1 + B * n_mlp * D].reshape(B * n_mlp, D)
    tape = torch.full((plan.tape_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    # the descriptor of a declined attention-half call (tape one byte short) declines the MLP half too
    assert K.mhla_block_fwd(plan, x, tape[:-1], *args) == A.ERR_INVALID
    assert K.mhla_block_mlp_fwd(plan, x1c) == A.ERR_INVALID
    plan.desc.tape_bytes = tape.numel()
    assert K.mhla_block_mlp_fwd(plan, x1c_odd) == A.ERR_ALIGN
    torch.cuda.synchronize()
    assert bool((tape == 0xA5).all())
    arena = torch.full((plan.bwd_bytes[1],), 0xA5, dtype=torch.uint8, device=DEV)
    gg = f32(B * n_mlp, D)
    bwd = lambda t, a, xc: K.mhla_block_mlp_bwd(plan, x, t, args[0], args[2], args[4], args[6], args[8], args[10], xc, gg,
                                                gg.to(torch.bfloat16), a, True)
    assert bwd(tape[:-1], arena, x1c) == A.ERR_INVALID and bwd(tape, arena[:-1], x1c) == A.ERR_INVALID
    assert bwd(tape, arena, x1c_odd) == A.ERR_ALIGN
    ge = f32(B * L, D)
    assert K.mhla_block_bwd(plan, x, tape, args[0], args[2], args[4], args[6], args[8], args[10], ge, ge.to(torch.bfloat16),
                            arena[:-1], True) == A.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((tape == 0xA5).all()) and bool((arena == 0xA5).all())
    # EncoderOp: every MLP-half call declined (a misaligned x1c) -> the Python chain runs that half, same result
    blocks, x0 = _encoder(favit, B, L, D, H, W, depth)
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0)
    ref2 = _run_encoder(favit, K, monkeypatch, blocks, x0)
    F.set_native_blocks(True)

    def odd(t):
        flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
        flat[1:1 + t.numel()] = t.reshape(-1)
        return flat[1:1 + t.numel()].reshape(t.shape)
    real_f, real_b = K.mhla_block_mlp_fwd, K.mhla_block_mlp_bwd
    monkeypatch.setattr(K, "mhla_block_mlp_fwd", lambda plan, x1c: real_f(plan, odd(x1c)))
    calls = _Calls(K, monkeypatch)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert calls.n["mhla_block_mlp_fwd"] == 2 and calls.ok["mhla_block_mlp_fwd"] == 0 and calls.n["mhla_block_mlp_bwd"] == 0
    assert calls.ok["mhla_block_fwd"] == 2 and calls.ok["mhla_block_bwd"] == 2, "the attention halves stay native"
    _same(got, ref, ref2)
    # the same for the backward half alone
    monkeypatch.setattr(K, "mhla_block_mlp_fwd", real_f)
    monkeypatch.setattr(K, "mhla_block_mlp_bwd", lambda plan, x, tape, g1, g2, we, wp, w1, w2, x1c, *a: real_b(plan, x, tape, g1, g2, we, wp, w1, w2, odd(x1c), *a))
    calls = _Calls(K, monkeypatch)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0)
    assert calls.ok["mhla_block_mlp_fwd"] == 2 and calls.n["mhla_block_mlp_bwd"] == 2 and calls.ok["mhla_block_mlp_bwd"] == 0
    assert calls.ok["mhla_block_bwd"] == 2
    _same(got, ref, ref2)


def test_declined_attention_half_backward_after_an_accepted_mlp_half(favit, K, env, monkeypatch):
    """The MLP half of each narrowed block's backward is taken (its arena holds the gradient of x1), then the library
    declines the attention half (an arena one byte short; a short tape would not do: with ptrs_set the descriptor's
    tape pointer is not rewritten) and the Python chain runs that half on the expanded gradient.
    Blocks 0 and 1 of this encoder are native and narrowed, block 2 (5 rows) runs the Python chains: two calls of each
    entry point, no whole-block backward call."""
    F = env
    favit.set_compute_dtype("bf16")
    blocks, x0 = _encoder(favit, *ENCODERS[0][0])
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0)
    ref2 = _run_encoder(favit, K, monkeypatch, blocks, x0)
    F.set_native_blocks(True)
    real = K.mhla_block_bwd
    seen = []

    def short_arena(plan, *a, **k):
        if plan.rows is not None:
            seen.append(k.get("ptrs_set", False))
            a = a[:10] + (a[10][:-1],) + a[11:]
        return real(plan, *a, **k)
    monkeypatch.setattr(K, "mhla_block_bwd", short_arena)
    calls = _Calls(K, monkeypatch)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0)
    print(f"\ncalls {calls.n}, accepted {calls.ok}, ptrs_set {seen}", end="")
    assert calls.ok["mhla_block_fwd"] == 2 and calls.ok["mhla_block_mlp_fwd"] == 2
    assert calls.n["mhla_block_mlp_bwd"] == 2 and calls.ok["mhla_block_mlp_bwd"] == 2
    assert calls.n["mhla_block_bwd"] == 2 and calls.ok["mhla_block_bwd"] == 0
    assert seen == [True, True], "the attention half follows an accepted MLP half of the same plan"
    _same(got, ref, ref2)


def test_layernorm1_without_gradient_buffers_layernorm2_with(favit, K, env, monkeypatch):
    """The LayerNorm 2 fold of a narrowed block goes to its gradient buffers from the native MLP half; LayerNorm 1 has
    none, so the attention half is never offered to the library and the Python chain returns dgamma / dbeta."""
    F = env
    favit.set_compute_dtype("bf16")
    blocks, x0 = _encoder(favit, *ENCODERS[0][0])
    has = lambda name: "norm1" not in name
    F.set_native_blocks(False)
    ref = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=has)
    ref2 = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=has)
    F.set_native_blocks(True)
    calls = _Calls(K, monkeypatch)
    got = _run_encoder(favit, K, monkeypatch, blocks, x0, grad_buffers=has)
    print(f"\ncalls {calls.n}, accepted {calls.ok}, deferred LayerNorm folds {len(got[2])} (reference {len(ref[2])})", end="")
    assert calls.ok["mhla_block_fwd"] == 2 and calls.ok["mhla_block_mlp_fwd"] == 2
    assert calls.n["mhla_block_mlp_bwd"] == 2 and calls.ok["mhla_block_mlp_bwd"] == 2
    assert calls.ok["mhla_block_bwd"] == 0, "no narrowed attention-half call is accepted"
    assert len(got[2]) == 3, "LayerNorm 2 of every block folds deferred, LayerNorm 1 of none"
    assert all(k in got[3] for k in ref[3])
    _same(got, ref, ref2)


# ------------------------------------------------------------------ the small model of test_gpu_cls_only.py
L, W, DEPTH, D, H, B = 50, 7, 4, 128, 2, 3
ROWS = [23, 17, 11, 5]
MLP_ROWS = [17, 11, 5, 5]
N_NATIVE = 3


def _model(favit, seed=11, **kw):
    torch.manual_seed(seed)
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=112, patch_size=16, num_classes=10, embed_dim=D, depth=DEPTH,
                                                    num_heads=H, window_size=W, use_mhla=True, **kw)
    x = torch.randn(B, 3, 112, 112)
    y = torch.randint(0, 10, (B,))
    return m, x, y


def _run(favit, m, x, y):
    for p in m.parameters():
        p.grad = None
    logits = m(x)
    favit.train.cross_entropy(logits, y).backward()
    torch.cuda.synchronize()
    return logits.detach().float().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("mode,tol", [("fp32", 2e-4), ("bf16", 1.5e-2)])
def test_narrowed_step_against_switch_off_full_path_and_oracle(favit, K, env, monkeypatch, mode, tol):
    favit.set_compute_dtype(mode)
    m, x, y = _model(favit)
    sd = {k: v.clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m.to(DEV).train()
    xd, yd = x.to(DEV), y.to(DEV)
    calls = _Calls(K, monkeypatch)
    lg_n, g_n = _run(favit, m, xd, yd)
    assert (calls.cut_f, calls.cut_b) == (DEPTH, DEPTH), "one cut in front of the first block, one inside each of the next three"
    calls.reset()
    monkeypatch.setenv("FAVIT_NO_MLP_NARROW", "1")
    lg_o, g_o = _run(favit, m, xd, yd)
    assert (calls.cut_f, calls.cut_b) == (DEPTH, DEPTH)
    monkeypatch.delenv("FAVIT_NO_MLP_NARROW")
    monkeypatch.setenv("FAVIT_NO_PRUNE", "1")
    lg_f, g_f = _run(favit, m, xd, yd)
    for name, lg, gr in (("switch off", lg_o, g_o), ("full path", lg_f, g_f)):
        e = rel_l2(lg_n, lg)
        worst = max((rel_l2(g_n[k], gr[k]), k) for k in gr)
        print(f"\n[{mode}] narrowed vs {name}: logits {e:.2e} (bit-identical: {torch.equal(lg_n, lg)}), "
              f"worst gradient {worst[0]:.2e} ({worst[1]})", end="")
        assert e < tol
        assert worst[0] < tol, (name, worst)
    if mode == "fp32":
        ref = O.vit_mhla_forward(x, sd, 16, H, W, True)
        O.cross_entropy(ref, y).backward()
        eo = rel_l2(lg_n.cpu(), ref.detach())
        wo = max((rel_l2(g_n[k].cpu(), sd[k].grad), k) for k in g_n)
        print(f"\n[{mode}] narrowed vs oracle: logits {eo:.2e}, worst gradient {wo[0]:.2e} ({wo[1]})", end="")
        assert eo < tol
        assert wo[0] < tol, wo


def test_gemm_shapes_of_the_narrowed_step(favit, K, env, monkeypatch):
    """fc1 / fc2 / dpre / dxn2 run at M = B * n_{k+1}, qkv / proj / do / dxn1 at M = B * n_k, and the fc1 / fc2 weight
    gradients sum over K = B * n_{k+1} (the Python chains: every GEMM passes K.gemm or a grouped launch)."""
    F = env
    favit.set_compute_dtype("bf16")
    F.set_native_blocks(False)
    m, x, y = _model(favit)
    m.to(DEV).train()
    ran, wg = [], []
    og, ot, orr = K.gemm, K.gemm_grouped_tn, K.gemm_grouped_tn_ragged
    monkeypatch.setattr(K, "gemm", lambda A_, B_, C_, M, N, Kd, *a, **k: (ran.append((M, N, Kd)), og(A_, B_, C_, M, N, Kd, *a, **k))[1])

    def grouped(orig):
        def w(problems, *a, **k):
            ok = orig(problems, *a, **k)
            if ok:
                wg.extend((tuple(p[2].shape), p[0].shape[0]) for p in problems)
            return ok
        return w
    monkeypatch.setattr(K, "gemm_grouped_tn", grouped(ot))
    monkeypatch.setattr(K, "gemm_grouped_tn_ragged", grouped(orr))
    _run(favit, m, x.to(DEV), y.to(DEV))
    wg += [((Mg, Ng), Kg) for Mg, Ng, Kg in ran]         # (a weight gradient launched on its own is a K.gemm with K = tokens)
    Hd = 4 * D
    for n, nm in zip(ROWS, MLP_ROWS):
        Ma, Mm = B * n, B * nm
        for shp in ((Ma, 3 * D, D), (Ma, D, 3 * D)):                      # qkv, dxn1
            assert shp in ran, shp
        for shp in ((Mm, Hd, D), (Mm, D, Hd)):                            # fc1 + dpre, fc2 + dxn2
            assert ran.count(shp) >= 2, (shp, ran.count(shp))
        assert ran.count((Ma, D, D)) >= 2, (Ma, D, D)                     # proj, do
        assert ((Hd, D), Mm) in wg and ((D, Hd), Mm) in wg, (nm, wg)      # dW1, dW2
        assert ((D, D), Ma) in wg and ((3 * D, D), Ma) in wg, (n, wg)     # dWproj, dWeff
    assert (B * 23, Hd, D) not in ran and (B * 23, D, Hd) not in ran, "no MLP-half GEMM on the first block's 23 rows"


def _opt(favit, m):
    return favit.train.FusedAdamW(favit.train.param_groups(m, lr=0.0), lr=0.0, weight_decay=0.0, distributed=False)


@pytest.mark.parametrize("segments", [1, 2])
def test_graphed_narrowed_step_replays_match_eager(favit, K, env, monkeypatch, segments):
    favit.set_compute_dtype("bf16")
    m, x, y = _model(favit)
    other, _, _ = _model(favit)
    m.to(DEV).train(), other.to(DEV).train()
    xd, yd = x.to(DEV), y.to(DEV)
    opt, oo = _opt(favit, m), _opt(favit, other)
    calls = _Calls(K, monkeypatch)
    want = favit.train.train_step(other, xd, yd, oo).item()
    torch.cuda.synchronize()
    assert calls.all_ok(N_NATIVE, N_NATIVE), (calls.n, calls.ok)
    want_g = {k: p.grad.detach().clone() for k, p in other.named_parameters()}
    calls.reset()
    step = favit.train.GraphedStep(m, opt, xd, yd, segments=segments)
    assert calls.capturing == 4 * N_NATIVE, "the captured step holds both halves of every native block, both directions"
    host = (dict(calls.n), calls.cut_f, calls.cut_b)
    assert calls.n == calls.ok
    for _ in range(3):
        got = step(xd, yd).item()
        torch.cuda.synchronize()
        assert abs(got - want) < 1e-5 * abs(want)
        worst = max((rel_l2(p.grad, want_g[k]), k) for k, p in m.named_parameters())
        assert worst[0] < 1e-5, worst
    assert (dict(calls.n), calls.cut_f, calls.cut_b) == host, "replays launch nothing from the host"


def test_eval_no_grad_logits_native_on_off(favit, K, env, monkeypatch):
    F = env
    favit.set_compute_dtype("bf16")
    m, x, _ = _model(favit)
    m.to(DEV).eval()
    xd = x.to(DEV)
    calls = _Calls(K, monkeypatch)
    with torch.no_grad():
        F.set_native_blocks(False)
        ref = m(xd).clone()
        assert calls.cut_f == DEPTH
        F.set_native_blocks(True)
        got = m(xd).clone()
    assert calls.all_ok(N_NATIVE, N_NATIVE, bwd=False), (calls.n, calls.ok)
    assert calls.cut_f == 2 * DEPTH
    assert torch.equal(got, ref)
