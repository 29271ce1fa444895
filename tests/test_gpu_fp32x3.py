"""fp32x3 compute mode on the GPU: the split-bf16 form of the exact-fp32 DMA kernel (FAVIT_F32X3, include/favit.h)
on the case grid of the exact kernel's own tests, its fallbacks, and the whole models / training flows of the fp32
mode at the fp32 mode's tolerances.

GEMM tolerance: rel-L2 against fp64 below 1e-5.  The numerical model (tests/test_fp32x3_host.py) sits at 4.4e-6 at
every K, fp32 accumulation adds ~4e-7; a truncating split (1.3e-5) or a dropped cross term (2e-3) lands above it.
Bias gradients sum the unsplit fp32 values and keep the exact kernel's 2e-6."""
import pytest
import torch

from conftest import rel_l2
import test_configs_golden as TC
import test_gpu_fullsize as TF
import test_gpu_modules as TM

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEMM_TOL = 1e-5
EXACT_TOL = 2e-6
X3_TAGS = ("p4x3", "p4x3_128")


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


@pytest.fixture(autouse=True)
def _fp32_mode(favit):
    favit.set_compute_dtype("fp32")
    yield
    favit.set_compute_dtype("fp32")
    favit.functional.clear_lp_mirrors()
    favit.functional.set_grad_ready_hook(None)


def _rand(shape, gen):
    return torch.randn(shape, generator=gen, device=DEV, dtype=torch.float32)


def _last(favit):
    return favit._abi.lib().favit_gemm_last_kernel().decode()


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("ak,bk", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,Kd", [(50432, 384, 384), (8192 + 40, 1152, 400), (32768 + 4, 200, 64), (36928, 768, 768)])
@pytest.mark.parametrize("epi", ["plain", "gelu", "dgelu", "res"])
def test_gemm_fp32x3_dma_kernel(K, favit, ak, bk, M, N, Kd, epi):
    """The grid of test_gemm_exact_fp32_dma_kernel issued with in_dtype = F32X3: every operand layout, ragged M and N
    tiles, the fused epilogues, against an fp64 product."""
    A = favit._abi
    g = torch.Generator(device=DEV).manual_seed(91)
    a = _rand((M, Kd) if ak else (Kd, M), g)
    b = _rand((N, Kd) if bk else (Kd, N), g)
    bias = _rand((N,), g)
    out = torch.empty((M, N), dtype=torch.float32, device=DEV)
    ref = ((a if ak else a.t()).double() @ (b.t() if bk else b).double())
    lda, ldb = (Kd if ak else M), (Kd if bk else N)
    kw = dict(a_kmajor=ak, b_kmajor=bk, in_dtype=A.F32X3)
    if epi == "plain":
        K.gemm(a, b, out, M, N, Kd, lda, ldb, N, **kw)
    elif epi == "gelu":
        pre = torch.empty_like(out)
        K.gemm(a, b, out, M, N, Kd, lda, ldb, N, bias=bias, act=A.ACT_GELU, aux_out=pre, ld_aux_out=N, **kw)
        ref = ref + bias.double()
        e_pre = rel_l2(pre.double(), ref)
        print(f"saved pre-activation rel-L2 {e_pre:.2e}")
        assert e_pre < GEMM_TOL
        ref = torch.nn.functional.gelu(ref)
    elif epi == "dgelu":
        pre = _rand((M, N), g)
        K.gemm(a, b, out, M, N, Kd, lda, ldb, N, act=A.ACT_DGELU, aux_in=pre, ld_aux_in=N, **kw)
        x = pre.double().requires_grad_(True)
        torch.nn.functional.gelu(x).sum().backward()
        ref = ref * x.grad
    else:
        res = _rand((M, N), g)
        K.gemm(a, b, out, M, N, Kd, lda, ldb, N, bias=bias, residual=res, ld_res=N, alpha=0.5, **kw)
        ref = 0.5 * ref + bias.double() + res.double()
    tag = _last(favit)
    err = rel_l2(out.double(), ref)
    print(f"{tag}: rel-L2 vs fp64 {err:.2e}")
    assert tag in X3_TAGS                                # (256- or 128-row tiles: by balance)
    assert err < GEMM_TOL


@pytest.mark.parametrize("M,N,T", [(1536, 384, 50432), (384, 1536, 50432), (1152, 384, 50432), (768, 3072, 36928), (200, 136, 65536)])
def test_gemm_fp32x3_dma_kernel_weight_gradients(K, favit, M, N, T):
    """The weight-gradient shape (both operands token-major, split over the tokens with fp32 atomics, fused bias
    gradient), from zero and accumulating into an existing gradient."""
    X3 = favit._abi.F32X3
    g = torch.Generator(device=DEV).manual_seed(92)
    dy = _rand((T, M), g)
    x = _rand((T, N), g)
    dw = torch.empty((M, N), dtype=torch.float32, device=DEV)
    db = torch.zeros((M,), dtype=torch.float32, device=DEV)
    K.gemm(dy, x, dw, M, N, T, M, N, N, a_kmajor=False, b_kmajor=False, a_rowsum=db, in_dtype=X3)
    assert _last(favit) in X3_TAGS
    ref = dy.double().t() @ x.double()
    e_w, e_b = rel_l2(dw.double(), ref), rel_l2(db.double(), dy.double().sum(0))
    print(f"{_last(favit)}: dW rel-L2 {e_w:.2e}, bias gradient {e_b:.2e}")
    assert e_w < GEMM_TOL
    assert e_b < EXACT_TOL
    K.gemm(dy, x, dw, M, N, T, M, N, N, a_kmajor=False, b_kmajor=False, a_rowsum=db, accumulate=True, in_dtype=X3)
    assert _last(favit) in X3_TAGS
    assert rel_l2(dw.double(), 2 * ref) < GEMM_TOL
    assert rel_l2(db.double(), 2 * dy.double().sum(0)) < EXACT_TOL


def test_gemm_fp32x3_falls_back_to_the_exact_kernels(K, favit):
    """F32X3 is a request: a batched problem, a K that is not a multiple of the stage depth and a misaligned operand
    run the exact-fp32 kernel they run under F32 -- exact-fp32 accuracy, tagged as the exact kernel."""
    X3 = favit._abi.F32X3
    g = torch.Generator(device=DEV).manual_seed(93)
    # batched
    Bz, M, N, Kd = 6, 8192, 256, 128
    a, b = _rand((Bz, M, Kd), g), _rand((Bz, N, Kd), g)
    out = torch.empty((Bz, M, N), dtype=torch.float32, device=DEV)
    K.gemm(a, b, out, M, N, Kd, Kd, Kd, N, batch=Bz, sA=(M * Kd, 0), sB=(N * Kd, 0), sC=(M * N, 0), in_dtype=X3)
    assert _last(favit) == "t128"
    assert rel_l2(out.double(), a.double() @ b.double().transpose(1, 2)) < EXACT_TOL
    # K = 392 is not a multiple of 16
    M, N, Kd = 50432, 384, 392
    a, b = _rand((M, Kd), g), _rand((N, Kd), g)
    out = torch.empty((M, N), dtype=torch.float32, device=DEV)
    K.gemm(a, b, out, M, N, Kd, Kd, Kd, N, in_dtype=X3)
    assert _last(favit) == "t128"
    assert rel_l2(out.double(), a.double() @ b.double().t()) < EXACT_TOL
    # A starts 4 bytes past a 16-byte boundary
    Kd = 384
    buf = _rand((M * Kd + 1,), g)
    b = _rand((N, Kd), g)
    K.gemm(buf, b, out, M, N, Kd, Kd, Kd, N, a_off=1, in_dtype=X3)
    assert _last(favit) == "t128"
    assert rel_l2(out.double(), buf[1:].view(M, Kd).double() @ b.double().t()) < EXACT_TOL
    # the same, aligned: the split kernel
    K.gemm(buf, b, out, M, N, Kd, Kd, Kd, N, in_dtype=X3)
    assert _last(favit) in X3_TAGS


def test_modes_do_not_leak(K, favit):
    """fp32 -> fp32x3 -> fp32 around one forward GEMM: the fp32 results are bitwise equal and come from the exact
    kernel; the fp32x3 result differs and comes from the split kernel."""
    g = torch.Generator(device=DEV).manual_seed(94)
    M, N, Kd = 50432, 384, 384
    a, w = _rand((M, Kd), g), _rand((N, Kd), g)
    outs, tags = [], []
    try:
        for mode in ("fp32", "fp32x3", "fp32"):
            favit.set_compute_dtype(mode)
            out = torch.empty((M, N), dtype=torch.float32, device=DEV)
            K.gemm(a, w, out, M, N, Kd, Kd, Kd, N)
            outs.append(out)
            tags.append(_last(favit))
    finally:
        favit.set_compute_dtype("fp32")
    assert tags[0] in ("p4f", "p4f128") and tags[2] == tags[0] and tags[1] in X3_TAGS, tags
    assert torch.equal(outs[0], outs[2])
    assert not torch.equal(outs[0], outs[1])
    assert rel_l2(outs[1], outs[0]) < GEMM_TOL


@pytest.mark.parametrize("bk", [True, False])
def test_gemm_fp32x3_single_pass_is_deterministic(K, favit, bk):
    """Forward (k-major weights) and input-gradient (mn-major weights) GEMMs are single-pass: bitwise equal across
    two launches."""
    g = torch.Generator(device=DEV).manual_seed(95)
    M, N, Kd = 50432, 384, 1536
    a = _rand((M, Kd), g)
    w = _rand((N, Kd) if bk else (Kd, N), g)
    o1 = torch.empty((M, N), dtype=torch.float32, device=DEV)
    o2 = torch.empty_like(o1)
    for o in (o1, o2):
        K.gemm(a, w, o, M, N, Kd, Kd, Kd if bk else N, N, b_kmajor=bk, in_dtype=favit._abi.F32X3)
        assert _last(favit) in X3_TAGS
    assert torch.equal(o1, o2)


# ------------------------------------------------------------------ whole models against the reference's golden vectors
def test_cfg1_vit_tiny_fp32x3(favit):
    favit.set_compute_dtype("fp32x3")
    TM.test_cfg1_vit_tiny_logits_loss_gradnorms(favit)
    assert favit.get_compute_mode() == "fp32x3"


def test_cfg2_vit_mhla_small_fp32x3(favit):
    TM.test_cfg2_vit_mhla_small_logits_loss_gradnorms(favit, "fp32x3", 1e-3, 2e-3)


def test_cfg3_sppp_mhla_small_fp32x3(favit):
    TC.test_gpu_cfg3_sppp_mhla_small(favit, "fp32x3", 1e-3, 2e-3)


def test_cfg4_vit_mhla_base_577_tokens_fp32x3(favit):
    TC.test_gpu_cfg4_vit_mhla_base_577_tokens(favit, "fp32x3", 1e-3, 2e-3)


def test_cfg5_identity_latent_mixed_counts_fp32x3(favit):
    TC.test_gpu_cfg5_identity_latent_mixed_counts(favit, "fp32x3", 1e-3, 2e-3)


def test_full_size_cfg2_forward_backward_fp32x3(favit, K):
    """The cfg2 step at B = 256 as test_full_size_cfg2_forward_backward_matches_golden[fp32...] does it, in fp32x3:
    element-wise 2e-4 against the B = 2 gradients, 2e-3 against the golden gradient norms, logits 1e-3 -- and the
    split kernel ran."""
    tol_elem, tol_gn, tol_logits = 2e-4, 2e-3, 1e-3
    MD = TF.MD
    favit.set_compute_dtype("fp32x3")
    try:
        m, x, y = TF._cfg2_model(favit)
        m.to(DEV).train()
        x, y = x.to(DEV), y.to(DEV)
        logits2 = m(x)
        assert rel_l2(logits2.detach().cpu(), MD["cfg2/logits"]) < tol_logits
        favit.train.cross_entropy(logits2, y).backward()
        g2 = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        for p in m.parameters():
            p.grad = None
        opt = favit.train.FusedAdamW(favit.train.param_groups(m, lr=1e-4), distributed=False)
        xb, yb = x.repeat(128, 1, 1, 1).contiguous(), y.repeat(128).contiguous()
        opt.zero_grad()
        K.GEMM_TRACE = []
        try:
            logits = m(xb)
            loss = favit.train.cross_entropy(logits, yb)
            loss.backward()
            torch.cuda.synchronize()
            ran = sorted({(t[3], t[5]) for t in K.GEMM_TRACE})
        finally:
            K.GEMM_TRACE = None
        print("GEMM kernels of the B = 256 step:", ran)
        assert any(fam in X3_TAGS for _, fam in ran), f"the split kernel did not run: {ran}"
        assert not any(fam in ("p4f", "p4f128") for _, fam in ran), f"an exact DMA-kernel launch in fp32x3 mode: {ran}"
        e_l = max(rel_l2(logits[:2].detach().cpu(), MD["cfg2/logits"]), rel_l2(logits[254:].detach().cpu(), MD["cfg2/logits"]))
        assert e_l < tol_logits
        assert abs(loss.item() - float(MD["cfg2/loss"])) < tol_logits * abs(float(MD["cfg2/loss"]))
        worst_e, worst_n = 0.0, 0.0
        for k, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            e = rel_l2(p.grad, g2[k])
            worst_e = max(worst_e, e)
            r = float(MD[f"cfg2/gnorm/{k}"])
            n = abs(p.grad.norm().item() - r) / max(r, 1e-12)
            worst_n = max(worst_n, n)
        print(f"[fp32x3] logits rel-L2 {e_l:.2e}; worst element-wise rel-L2 vs B=2: {worst_e:.2e}; "
              f"worst gradient-norm deviation vs golden: {worst_n:.2e}")
        assert worst_e < tol_elem
        assert worst_n < tol_gn
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()


# ------------------------------------------------------------------ training flows against the oracle
# Bound of both tests: 1e-4, the bound of their fp32 rows.  Measured worst values on the MI355X:
# 1.9e-7 (AdamW steps, loss) and 1.18e-6 (frozen layers, gradients; loss 1.0e-7); three times either is below 1e-4, so
# 1e-4 -- the larger of the two -- is the bound.
TRAIN_TOL = 1e-4


def test_torch_optim_adamw_training_steps_fp32x3(favit):
    """test_torch_optim_adamw_training_steps restated for fp32x3: three torch.optim.AdamW steps against the oracle."""
    from oracle import favit_oracle as O
    favit.set_compute_dtype("fp32x3")
    torch.manual_seed(5)
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2,
                                                    num_heads=4, use_mhla=True).to(DEV).train()
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    names = [k for k, _ in m.named_parameters()]
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2, weight_decay=0.05)
    ropt = torch.optim.AdamW([sd[k] for k in names], lr=1e-2, weight_decay=0.05)
    x = torch.randn(4, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (4,), device=DEV)
    worst = 0.0
    for step in range(3):
        opt.zero_grad()
        loss = torch.nn.CrossEntropyLoss()(m(x), y)
        loss.backward()
        opt.step()
        ropt.zero_grad()
        lo = O.cross_entropy(O.vit_mhla_forward(x.cpu(), sd, 4, 4, 7, True), y.cpu())
        lo.backward()
        ropt.step()
        worst = max(worst, abs(loss.item() - lo.item()) / max(1.0, abs(lo.item())))
    print(f"[fp32x3] worst loss deviation from the oracle over three AdamW steps: {worst:.2e}")
    assert worst < TRAIN_TOL
    assert lo.item() < 2.0


def test_frozen_layers_with_the_fused_optimizer_fp32x3(favit):
    """test_frozen_layers_with_the_fused_optimizer restated for fp32x3: frozen blocks, trainable head / latent_proj,
    gradients in the fused optimizer's flat buffers, against the oracle."""
    from oracle import favit_oracle as O
    favit.set_compute_dtype("fp32x3")
    try:
        torch.manual_seed(9)
        m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, num_classes=10, embed_dim=128, depth=3,
                                                        num_heads=2, use_mhla=True).to(DEV).train()
        for n, p in m.named_parameters():
            p.requires_grad = ("head" in n) or ("latent_proj" in n)
        opt = favit.train.FusedAdamW(favit.train.param_groups(m, lr=1e-3, head_lr=1e-2), lr=1e-3, distributed=False)
        x = torch.randn(32, 3, 32, 32, device=DEV)
        y = torch.randint(0, 10, (32,), device=DEV)
        sd = {k: v.detach().cpu().clone().requires_grad_(("head" in k) or ("latent_proj" in k)) for k, v in m.state_dict().items()}
        lo = O.cross_entropy(O.vit_mhla_forward(x.cpu(), sd, 4, 2, 7, True), y.cpu())
        lo.backward()
        for _ in range(2):
            opt.zero_grad()
            loss = favit.train.cross_entropy(m(x), y)
            loss.backward()
        e_loss = abs(loss.item() - lo.item()) / max(1.0, abs(lo.item()))
        worst = 0.0
        for n, p in m.named_parameters():
            if p.requires_grad:
                gbuf = favit.functional._gt(p)
                assert gbuf is not None, n
                worst = max(worst, rel_l2(gbuf.cpu(), sd[n].grad))
            else:
                assert p.grad is None and favit.functional._gt(p) is None, n
        print(f"[fp32x3] frozen-layer flow: loss deviation {e_loss:.2e}, worst gradient rel-L2 vs the oracle {worst:.2e}")
        assert e_loss < TRAIN_TOL
        assert worst < TRAIN_TOL
    finally:
        favit.set_compute_dtype("fp32")
        favit.functional.clear_lp_mirrors()
        favit.functional.set_grad_ready_hook(None)
