"""Attention maps on the GPU (csrc/attn_maps.hip) against the float64 restatement of
tests/_attention_ref.py, computed from the SAME stored values (bf16 inputs upcast exactly).

Tolerances.  Kernels: rel-L2 < 2e-5, this suite's bound for fp32-accumulated results of exact inputs
(test_gpu_kernels.py).  Rollout mass: |sum - 1| < 1e-4 (each step adds at most W + 2 fp32 terms per key; twelve steps
stay below 1e-5 relative, a lost slot costs orders of magnitude more).  Whole models: 1e-4 in fp32 mode and 2e-2 in bf16
mode (test_gpu_modules.py); logits under capture against the shipped, pruned eval forward: 2e-4, the pruned-against-full
bound of test_gpu_cls_only.py, in both modes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attention_ref as R
from conftest import rel_l2
from oracle import favit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5


def _tol(dtype):                                    # test_gpu_kernels.py: the bound of K.mhla_attn_fwd's own test
    return 2e-5 if dtype == torch.float32 else 1e-2


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


@pytest.fixture(autouse=True)
def _fp32_mode(favit):
    favit.set_compute_dtype("fp32")
    yield
    favit.set_compute_dtype("fp32")


def _qkv(B, L, H, hd, dtype, seed, gain=1.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * L, 3 * H * hd, generator=g) * gain).to(dtype).to(DEV)


def _check(got, want, what):
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), what
    err = rel_l2(got, want)
    print(f"{what}: rel-L2 {err:.3e}")
    assert err < TOL, (what, err)


# ---------------------------------------------------------------------------------------------------------------
# MHLA probabilities
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd", [16, 32, 64, 128])
@pytest.mark.parametrize("L,W", [(5, 7), (7, 7), (8, 7), (17, 3), (65, 7), (40, 15)])
def test_mhla_probs_match_float64_of_the_stored_values(K, L, W, hd, dtype):
    for H in (1, 3):
        for B in (1, 3):
            qkv = _qkv(B, L, H, hd, dtype, 7 * L + W + hd + H + B)
            want = R.mhla_probs(qkv, B, L, H, hd, W)
            per_head = K.mhla_attn_probs(qkv, B, L, H, hd, W)
            mean = K.mhla_attn_probs(qkv, B, L, H, hd, W, head_mean=True)
            assert tuple(per_head.shape) == (B, H, L, W) and tuple(mean.shape) == (B, L, W)
            assert per_head.dtype == mean.dtype == torch.float32
            _check(per_head, want, f"per-head B{B} H{H}")
            _check(mean, want.mean(dim=1), f"head-mean B{B} H{H}")
            assert (per_head.sum(-1) - 1).abs().max().item() < 1e-5
            assert (mean.sum(-1) - 1).abs().max().item() < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("L,W,hd", [(17, 3, 16), (65, 7, 64), (40, 15, 32), (5, 7, 128)])
def test_mhla_probs_padding_mask(K, L, W, hd, dtype):
    B, H = 3, 3
    qkv = _qkv(B, L, H, hd, dtype, 31 * L + W)
    n_b = [L, max(1, L // 2), 1]
    mask = torch.zeros(B, L, L, dtype=torch.uint8)
    for b in range(B):
        mask[b, :, :n_b[b]] = 1                                   # mask[b, :, j] = j < n_b
    idx = torch.from_numpy(O.window_indices(L, W))
    slot_keep = torch.stack([mask[b][torch.arange(L)[:, None], idx] for b in range(B)]) != 0       # [B, L, W]
    dead = ~slot_keep.any(-1)                                     # rows with every slot masked
    assert dead.any() or L <= W, "the shapes are chosen so that dead rows exist"
    want = R.mhla_probs(qkv, B, L, H, hd, W, mask)
    for head_mean in (False, True):
        got = K.mhla_attn_probs(qkv, B, L, H, hd, W, mask.to(DEV), head_mean=head_mean).cpu()
        assert torch.isfinite(got).all()
        g4 = got[:, None] if head_mean else got
        assert (g4[dead[:, None].expand(B, g4.shape[1], L)] == 0).all(), "dead rows are all zero"
        assert (g4[(~slot_keep)[:, None].expand(B, g4.shape[1], L, W)] == 0).all(), "masked slots are exactly 0"
        live = ~dead
        assert (g4.sum(-1)[live[:, None].expand(B, g4.shape[1], L)] - 1).abs().max().item() < 1e-5
        _check(got, want.mean(1) if head_mean else want, f"padding mask head_mean={head_mean}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("L,W,hd", [(8, 7, 16), (65, 7, 64), (40, 15, 128)])
def test_mhla_probs_random_mask(K, L, W, hd, dtype):
    B, H = 3, 3
    qkv = _qkv(B, L, H, hd, dtype, 17 * L + W)
    g = torch.Generator().manual_seed(L + W)
    mask = (torch.rand(B, L, L, generator=g) < 0.5).to(torch.uint8)
    want = R.mhla_probs(qkv, B, L, H, hd, W, mask)
    idx = torch.from_numpy(O.window_indices(L, W))
    slot_keep = torch.stack([mask[b][torch.arange(L)[:, None], idx] for b in range(B)]) != 0
    for head_mean in (False, True):
        got = K.mhla_attn_probs(qkv, B, L, H, hd, W, mask.to(DEV), head_mean=head_mean).cpu()
        g4 = got[:, None] if head_mean else got
        assert (g4[(~slot_keep)[:, None].expand(B, g4.shape[1], L, W)] == 0).all()
        _check(got, want.mean(1) if head_mean else want, f"random mask head_mean={head_mean}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("L,W,hd,H", [(5, 7, 16, 3), (65, 7, 64, 3), (40, 15, 32, 1), (17, 3, 128, 3)])
def test_mhla_probs_reproduce_the_shipped_forward(K, L, W, hd, H, dtype):
    """sum_w P[.., w] * v~[idx[i, w]] is K.mhla_attn_fwd's output, within that kernel's own tolerance."""
    B, D = 3, H * hd
    qkv = _qkv(B, L, H, hd, dtype, 3 * L + hd)
    P = K.mhla_attn_probs(qkv, B, L, H, hd, W).cpu().to(torch.float64)                       # [B, H, L, W]
    v = qkv.cpu().to(torch.float64).reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)[2]        # [B, H, L, hd]
    idx = torch.from_numpy(O.window_indices(L, W))
    want = (P[..., None] * v[:, :, idx, :]).sum(3).transpose(1, 2).reshape(B * L, D)
    out = K.mhla_attn_fwd(qkv, B, L, H, hd, W)
    err = rel_l2(out.float(), want)
    print(f"forward from the probabilities: rel-L2 {err:.3e}")
    assert err < _tol(dtype)


def test_mhla_probs_refuses_unsupported_shapes_before_any_write(favit):
    A = favit._abi
    lib = A.lib()
    st = favit.kernels._st
    qkv = torch.zeros(10, 3 * 24, device=DEV)
    probs = torch.full((2 * 5 * 7 + 64,), 12345.0, device=DEV)
    p = lambda t: t.data_ptr()
    for hd, W, code in [(24, 7, A.ERR_UNSUPPORTED), (8, 7, A.ERR_UNSUPPORTED), (16, 17, A.ERR_UNSUPPORTED),
                        (16, 4, A.ERR_INVALID), (16, 0, A.ERR_INVALID), (16, -3, A.ERR_INVALID)]:
        assert lib.favit_mhla_attn_probs(p(qkv), p(probs), None, 2, 5, 1, hd, W, A.F32, 1, st()) == code, (hd, W)
    assert lib.favit_sdpa_probs(p(qkv), p(probs), None, 2, 5, 1, 24, A.F32, 0.2, 1, st()) == A.ERR_UNSUPPORTED
    ptrs = (ctypes.c_void_p * 1)(p(probs))
    ws = (ctypes.c_int32 * 1)(7)
    assert lib.favit_attn_rollout(1, ptrs, ws, p(probs), 0, 1, A.ROLLOUT_MAX_L + 1, 0.5, st()) == A.ERR_UNSUPPORTED
    assert lib.favit_attn_rollout(1, ptrs, ws, p(probs), 5, 1, 5, 0.5, st()) == A.ERR_INVALID
    assert lib.favit_attn_rollout(33, ptrs, ws, p(probs), 0, 1, 5, 0.5, st()) == A.ERR_INVALID
    torch.cuda.synchronize()
    assert (probs == 12345.0).all(), "a refused call writes nothing"


# ---------------------------------------------------------------------------------------------------------------
# dense probabilities
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd", [16, 64])
@pytest.mark.parametrize("L", [1, 5, 65, 130])
def test_dense_probs_match_float64_of_the_stored_values(K, L, hd, dtype):
    B = 3
    for H in (1, 3):
        qkv = _qkv(B, L, H, hd, dtype, 11 * L + hd + H)
        keep = torch.ones(B, L, dtype=torch.uint8)
        keep[1] = 0                                               # one sample fully masked
        keep[2, L // 2:] = 0 if L > 1 else 1
        for kk in (None, keep):
            want = R.dense_probs(qkv, B, L, H, hd, kk)
            per_head = K.sdpa_probs(qkv, B, L, H, hd, None if kk is None else kk.to(DEV))
            mean = K.sdpa_probs(qkv, B, L, H, hd, None if kk is None else kk.to(DEV), head_mean=True)
            assert tuple(per_head.shape) == (B, H, L, L) and tuple(mean.shape) == (B, L, L)
            _check(per_head, want, f"dense per-head H{H} masked={kk is not None}")
            _check(mean, want.mean(1), f"dense head-mean H{H} masked={kk is not None}")
            if kk is not None:
                assert (per_head[1] == 0).all() and (mean[1] == 0).all(), "an all-masked sample is all zeros"
                assert (per_head.cpu()[:, :, :, :][(kk == 0)[:, None, None, :].expand(B, H, L, L)] == 0).all()
                assert (per_head[0].sum(-1) - 1).abs().max().item() < 1e-5
            else:
                assert (per_head.sum(-1) - 1).abs().max().item() < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# rollout
def _maps(B, L, W, seed):
    """Row-stochastic fp32 maps on the device: [B, L, W], or [B, L, L] for W = 0."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, L, W if W else L, generator=g) + 0.05
    return (p / p.sum(-1, keepdim=True)).to(DEV)


def _stack(kind, n, W):
    if kind == "band":
        return [W] * n
    if kind == "dense":
        return [0] * n
    return [W if k % 2 == 0 else 0 for k in range(n)]             # alternating, banded first


_BAND = [(L, W, n, 0, 0.5) for L in (6, 65, 300, 3137) for W in (7, 15) for n in (1, 2, 12)]
_BAND += [(L, 7, n, L // 2, 0.0) for L in (6, 65, 300, 3137) for n in (2, 12)]
_BAND += [(65, 15, 12, 33, 0.5), (300, 15, 2, 0, 0.0)]
_DENSE = [(L, 7, n, c, res) for L in (6, 65, 300) for n in (1, 2, 12) for c, res in ((0, 0.5),)]
_DENSE += [(65, 7, 2, 30, 0.0), (300, 7, 12, 150, 0.5)]
_ALT = [(L, W, n, 0, 0.5) for L in (6, 65, 300) for W in (7, 15) for n in (2, 12)]
_ALT += [(3137, 7, 2, 0, 0.5), (65, 7, 12, 32, 0.0)]


def _rollout_case(favit, K, kind, L, W, n, cls_row, residual, B=2):
    widths = _stack(kind, n, W)
    probs = [_maps(B, L, w, 1000 * L + 10 * k + w) for k, w in enumerate(widths)]
    got = K.attn_rollout(probs, widths, cls_row=cls_row, residual=residual)
    again = K.attn_rollout(probs, widths, cls_row=cls_row, residual=residual)
    assert tuple(got.shape) == (B, L) and got.dtype == torch.float32
    assert torch.equal(got, again), "two runs are bitwise equal"
    want = R.rollout(probs, widths, cls_row, residual)
    g = got.cpu()
    assert torch.isfinite(g).all()
    err, mass = rel_l2(g, want), (g.double().sum(1) - 1).abs().max().item()
    print(f"rollout {kind} L{L} W{W} n{n} cls{cls_row} res{residual}: rel-L2 {err:.3e}, |sum - 1| {mass:.3e}")
    assert err < TOL
    assert mass < 1e-4
    if kind == "band" and cls_row == 0:
        cone = favit.functional.cls_plan(L, W, n)[0]              # the rows the first block's input contributes
        if cone is not None:
            head, tail = cone
            assert (g[:, head:L - tail] == 0.0).all(), "entries outside the cls_plan cone are exactly 0.0"
            assert (g[:, :head] > 0).all() and (g[:, L - tail:] > 0).all()
    return g


@pytest.mark.parametrize("L,W,n,cls_row,residual", _BAND)
def test_rollout_banded(favit, K, L, W, n, cls_row, residual):
    _rollout_case(favit, K, "band", L, W, n, cls_row, residual)


@pytest.mark.parametrize("L,W,n,cls_row,residual", _DENSE)
def test_rollout_dense(favit, K, L, W, n, cls_row, residual):
    _rollout_case(favit, K, "dense", L, W, n, cls_row, residual)


@pytest.mark.parametrize("L,W,n,cls_row,residual", _ALT)
def test_rollout_alternating(favit, K, L, W, n, cls_row, residual):
    _rollout_case(favit, K, "alt", L, W, n, cls_row, residual)


def test_rollout_at_the_largest_length(favit, K):
    """L = ROLLOUT_MAX_L: the two rows of r take 128 KiB of LDS, above the 64 KiB a launch gets without asking."""
    _rollout_case(favit, K, "band", K.ROLLOUT_MAX_L, 7, 2, 0, 0.5, B=1)


def test_rollout_loses_the_mass_of_fully_masked_rows(K):
    L, W = 9, 3
    P = _maps(1, L, W, 5)
    P[0, 1] = 0                                                   # row 1: every slot masked
    got = K.attn_rollout([P, P], [W, W], residual=0.5).cpu()
    want = R.rollout([P, P], [W, W], 0, 0.5)
    assert rel_l2(got, want) < TOL
    assert want.sum().item() < 1 - 1e-3 and abs(got.sum().item() - want.sum().item()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------
# whole models
def _sharpen(m):
    """Attention of a freshly initialised model is almost uniform (weights of std 0.02, and MHLA's keys pass through
    latent_proj as well): scale the q and k projections (not v: the branch keeps its size) so that the maps have
    structure to compare.  The gains are chosen on the float64 reference alone: the largest probability of a map is
    0.2 .. 0.45 (uniform: 1/65 dense, 1/7 banded), and rounding every linear layer's operands and result to bf16 in
    that reference moves its maps by at most 6e-3 rel-L2 -- inputs on which the bf16 bound of 2e-2 is a fair one.
    (Four times larger gains saturate the softmax at 0.99; the float64 reference with bf16-rounded linears is then
    12 % off its own logits, so nothing could be told from a comparison.)"""
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("attn.in_proj_weight"):                 # nn.MultiheadAttention: Xavier, already of size
                p[:2 * p.shape[1]].mul_(1.5)
            elif n.endswith("attn.qkv.weight"):
                p[:2 * p.shape[1]].mul_(6.0)
            elif n.endswith("latent_proj.weight"):
                p.mul_(6.0)
            elif n.endswith(("attn.qkv.bias", "attn.in_proj_bias", "latent_proj.bias")):
                p.normal_(0.0, 0.1)
    return m


def _segmaps():
    maps = np.stack([O.voronoi_labels(32, 16, seed=3), O.voronoi_labels(32, 16, seed=8)])
    counts = [len(O.map_patches(s, 32, 4)) for s in maps]
    assert counts[0] == counts[1], f"the two label maps must give one token count, got {counts}: pick other seeds"
    return maps


def _model(favit, kind):
    torch.manual_seed(5)
    M = favit.models
    kw = dict(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=3, num_heads=2)
    if kind == "vit":
        m = M.vit.VisionTransformer(**kw)
    elif kind == "sppp_mhla":
        m = M.sppp_mhla.SPPPViTMHLA(window_size=7, use_mhla=True, num_superpixels=16, pooling_type="mean", **kw)
    else:
        m = M.vit_mhla.VisionTransformerMHLA(window_size=7, use_mhla=(kind == "vit_mhla"), **kw)
    return _sharpen(m)


_REF_CACHE = {}


def _reference(kind, m, x, segmaps):
    if kind not in _REF_CACHE:
        _REF_CACHE[kind] = R.model_maps(kind, x, m.state_dict(), 4, 2, 7, segmaps=segmaps)
    return _REF_CACHE[kind]


@pytest.mark.parametrize("mode,tol,logit_tol", [("fp32", 1e-4, 2e-4), ("bf16", 2e-2, 2e-4)])
@pytest.mark.parametrize("kind", ["vit_mhla", "vit_mhla_dense", "vit", "sppp_mhla"])
def test_whole_model_maps(favit, kind, mode, tol, logit_tol):
    m = _model(favit, kind)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(9))
    segmaps = _segmaps() if kind == "sppp_mhla" else None
    ref = _reference(kind, m, x, segmaps)
    favit.set_compute_dtype(mode)
    m.to(DEV).train()
    if segmaps is not None:
        m.segmentation.set_label_maps(torch.from_numpy(segmaps).to(DEV))
    xd = x.to(DEV)
    m.eval()
    with torch.no_grad():
        before = m(xd).clone()
    m.train()
    res = favit.harness.attention_maps(m, xd)
    assert m.training, "the training flag is restored"
    m.eval()
    with torch.no_grad():
        after = m(xd)
    assert torch.equal(before, after), "an ordinary forward after the call is bit-identical to one before it"
    assert favit.functional._CAPTURE["active"] is None
    L = ref["rollout"].shape[1]
    assert tuple(res["rollout"].shape) == (2, L) and tuple(res["cls_attention"].shape) == (2, L)
    assert res["window"] == ref["window"] and len(res["layers"]) == 3
    errs = {"rollout": rel_l2(res["rollout"], ref["rollout"]),
            "cls_attention": rel_l2(res["cls_attention"], ref["cls_attention"]),
            "layers": max(rel_l2(a, b) for a, b in zip(res["layers"], ref["layers"])),
            "logits_vs_ref": rel_l2(res["logits"].float(), ref["logits"]),
            "logits_vs_pruned": rel_l2(res["logits"].float(), before.float())}
    print(f"{kind} {mode}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["rollout"] < tol and errs["cls_attention"] < tol and errs["layers"] < tol
    assert errs["logits_vs_pruned"] < logit_tol
    assert (res["rollout"].sum(1) - 1).abs().max().item() < 1e-4
    grid = res["grid"].cpu()
    assert tuple(grid.shape) == (2, 8, 8)
    roll = res["rollout"].cpu()
    if kind != "sppp_mhla":
        assert torch.equal(grid.reshape(2, 64), roll[:, 1:])
    else:
        for b in range(2):
            mapping = O.map_patches(segmaps[b], 32, 4)            # token r + 1 <- the patches of the r-th entry
            flat = grid[b].reshape(-1)
            for r, patches in enumerate(mapping.values()):
                assert (flat[patches] == roll[b, 1 + r]).all(), "the patches of one superpixel share its token's value"
            assert sorted(set(flat.tolist())) == sorted(set(roll[b, 1:].tolist()))
    # per-head capture: the same maps, head by head
    ph = favit.harness.attention_maps(m, xd, per_head=True)
    assert all(p.dim() == 4 and p.shape[1] == 2 for p in ph["layers"])
    assert max(rel_l2(p.mean(1), q) for p, q in zip(ph["layers"], res["layers"])) < 1e-6
    assert rel_l2(ph["rollout"], res["rollout"]) < 1e-6


def test_capture_records_in_execution_order_and_pruned_rows_are_not_taken(favit):
    m = _model(favit, "vit_mhla").to(DEV).eval()
    x = torch.randn(2, 3, 32, 32, device=DEV)
    F = favit.functional
    with torch.no_grad(), F.capture_attention() as cap:
        m(x)
    assert [(r.kind, r.W, r.B, r.L, r.H) for r in cap.layers] == [("mhla", 7, 2, 65, 2)] * 3
    assert all(tuple(r.probs.shape) == (2, 65, 7) for r in cap.layers)
    m.train()
    with F.capture_attention():
        with pytest.raises(RuntimeError, match="training"):
            m(x)


# ---------------------------------------------------------------------------------------------------------------
# tool
def test_tool_writes_the_four_arrays(tmp_path):
    rs = np.random.RandomState(0)
    data = tmp_path / "d.npz"
    np.savez(data, x_train=rs.randint(0, 256, (4, 32, 32, 3)).astype(np.uint8), y_train=np.arange(4) % 3,
             x_test=rs.randint(0, 256, (4, 32, 32, 3)).astype(np.uint8), y_test=np.arange(4) % 3)
    out = tmp_path / "maps"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "attention_maps.py"), "--experiment", "mhla", "--data", str(data),
           "--img_size", "32", "--patch_size", "4", "--embed_dim", "64", "--depth", "3", "--num_heads", "2",
           "--num_images", "4", "--out", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    shapes = {n: np.load(out / f"{n}.npy").shape for n in ("rollout", "grid", "cls_attention", "logits")}
    assert shapes == {"rollout": (4, 65), "grid": (4, 8, 8), "cls_attention": (4, 65), "logits": (4, 3)}
    roll = np.load(out / "rollout.npy")
    assert np.isfinite(roll).all() and np.abs(roll.sum(1) - 1).max() < 1e-4
