"""GPU tests of every kernel that draws a dropout mask, against float64 references built with the EXPLICIT mask.

No kernel stores its mask: each recomputes the element index and draws from favit_keep (csrc/common.h).  The mask is a
pure function of (seed, index, p), so tests/_dropout_ref.py restates the draw on the host, builds the mask, and runs
plain float64 attention with it under autograd.  That pins O, dQ, dK and dV of the dropout instantiations per row --
the consistency tests of test_gpu_kernels.py only tie forward and dV together in one scalar, and would pass if forward
and backward agreed on a mask other than the documented one.

  a. keep_mask == favit_dropout, bit for bit (everything below leans on it);
  b. the MHLA core: fp32 / generic kernels, the bf16 MFMA forward with the default two-owner-pass backward and with
     the 8-lanes-per-row backward (mhla_bwd_kernel), and the saved-statistics pair at 3 and 5 chunks, with and without
     a [B, L, L] mask.  NOT covered: the table formulation, mhla_bwd_mfma_kernel.  Nothing launches it:
     FAVIT_MHLA_BWD_TABLES (like FAVIT_MHLA_VALU) only turns the default backward off, and the call then reaches
     mhla_bwd_kernel.  The cases under that switch are kept so that the switch stays checked, and they are counted
     as what they run: a second pass of the 8-lanes-per-row kernel.  The dropout draw of the table kernel is unchecked
     until the switch is wired to it, or the kernel is removed;
  c. the fused dense attention (forward, dQ, dK / dV) at 4 and 5 waves, and the contract of a fully masked query row;
  d. the GEMM dropout epilogue of every kernel family (asserted with favit_gemm_last_kernel), favit_ln_gemm, the fp8
     GEMM, odd N, and the refusals.

References start from the bf16-rounded inputs.  Global rel-L2 gates are those of the p = 0 tests of the same kernels
(test_gpu_kernels.py): MHLA out 2e-5 / 1e-2, dqkv 5e-5 / 1.5e-2, lse 2e-3 absolute; SDPA o 2e-5 / 1e-2, gradients
5e-5 / 2e-2, lse 2e-5 (+ 3e-3 for bf16) rel-L2; GEMM 2e-5 / 1e-2 and 1e-6 for the fp32 "kept" comparison.

Per-row error (a wrong draw on the 2h edge rows of a window hides in a global norm): |got - ref| of a [D] row over
(|ref row| + 1e-3 * |ref| / sqrt(rows)), the denominator of test_mhla_saved_statistics_backward_sweep.  bf16 takes that
sweep's gate, 6e-2.  fp32 is gated at 4x the worst per-row error the SAME kernels show at p = 0 against the same
float64 reference (one factor 2 for 1 / (1 - p) <= 2, one for rows whose norm shrinks when most slots drop); the p = 0
cases stay in the grid, so the measurement is repeated by every run and printed at teardown ("rows p=0" groups):
  measured at p = 0:  MHLA fp32 7.16e-7 (L=5 W=7 hd=16, masked, dq)   SDPA fp32 1.35e-6 (Lq=130 Lk=64 hd=192, dq)
  gates (4x):         MHLA fp32 2.9e-6                               SDPA fp32 5.4e-6
  worst with dropout: MHLA fp32 1.23e-6, SDPA fp32 1.59e-6; bf16 9.7e-3 (MHLA) and 1.1e-2 (SDPA) against 6e-2
A wrong slot gives an O(1) per-row error, so any gate below ~0.3 discriminates."""
import math

import pytest
import torch

import _dropout_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

ROW_GATE = {("mhla", F32): 2.9e-6, ("sdpa", F32): 5.4e-6, ("mhla", BF16): 6e-2, ("sdpa", BF16): 6e-2}

_WORST = {}         # (group, gate) -> worst error seen in this run (printed at module teardown; visible with -s)
# Cases that ran to the end, and cases that were entered.  "tables switch" counts the cases under FAVIT_MHLA_BWD_TABLES,
# which run mhla_bwd_kernel like the "valu" ones (module docstring): the count says the switch was exercised, no more.
# _ENTERED is counted after the skip for a switch that does not apply (hd < 32: such a case could never run) and
# before the skip for an unsupported saved-statistics shape (that one must show as a case that did not run).
_RAN = {"lse": 0, "tables switch": 0, "valu": 0}
_ENTERED = {"lse": 0, "tables switch": 0, "valu": 0}
_NEED = {"lse": 20, "tables switch": 12, "valu": 12}


@pytest.fixture(scope="module")
def K(favit):
    favit.functional.set_dropout_epoch(None)        # seeds as given: the restatement knows no epoch word
    yield favit.kernels
    for (group, gate), e in sorted(_WORST.items()):
        print(f"\n[dropout masks] {group}: worst {e:.3e} (gate {gate:g})", end="")
    print(f"\n[dropout masks] cases run: {_RAN}")
    for k, need in _NEED.items():       # a whole-module run enters 96 / 28 / 28; a -k selection is held to what it entered
        assert _RAN[k] >= min(need, _ENTERED[k]), f"{k}: {_RAN[k]} of {_ENTERED[k]} cases ran (skipped or failed), {need} needed"


def _tol(dtype):
    return 2e-5 if dtype == F32 else 1e-2


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rand(shape, dtype, g, scale=1.0):
    return (torch.randn(shape, generator=g, device=DEV, dtype=F32) * scale).to(dtype)


def _note(group, gate, e):
    _WORST[(group, gate)] = max(_WORST.get((group, gate), 0.0), e)


def _vanishes(ref, gross):
    """Is the reference zero by cancellation (R.sdpa_grad_scale)?  Then errors are measured against the cancelling terms."""
    return gross is not None and ref.double().norm().item() <= 1e-9 * gross.double().norm().item()


def _close(group, got, ref, tol, what="", gross=None):
    e = rel_l2(got, ref)
    if _vanishes(ref, gross):
        e = (got.double() - ref.double()).norm().item() / max(gross.double().norm().item(), 1e-300)   # (all dropped: 0 / tiny)
    _note(group, tol, e)
    print(f"{group} {what}: rel-L2 {e:.3e} (gate {tol:g})")
    assert math.isfinite(e) and e < tol, f"{group} {what}: rel-L2 {e:.3e} >= {tol:g}"


def _rows(group, got, ref, rows, gate, what="", gross=None):
    """Worst per-row error of a [rows, D] result; the denominator of test_mhla_saved_statistics_backward_sweep."""
    a, b = got.double().reshape(rows, -1), ref.double().reshape(rows, -1)
    d = gross.double().reshape(rows, -1) if _vanishes(ref, gross) else b
    err = (a - b).norm(dim=-1) / (d.norm(dim=-1) + 1e-3 * d.norm() / rows ** 0.5).clamp_min(1e-300)
    e = err.max().item()
    _note(group, gate, e)
    print(f"{group} {what}: worst row {e:.3e} at row {int(err.argmax())} (gate {gate:g})")
    assert math.isfinite(e) and e < gate, f"{group} {what}: per-row error {e:.3e} at row {int(err.argmax())} >= {gate:g}"


def _raises_code(code, fn, *a, **kw):
    with pytest.raises(RuntimeError, match=rf"\(code {code}\)"):
        fn(*a, **kw)


# --------------------------------------------------------------------------------------
# a. The restatement is the library's draw
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("seed", [1, 0x42, 0x123456789ABCDEF, 0x7FFFFFFF00000005])
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_mask_is_the_dropout_kernels_draw(K, favit, p, seed, dtype):
    assert favit.functional.get_dropout_epoch() is None, "the dropout epoch word must be unset"
    n = (1 << 20) + 3
    y = K.dropout(torch.ones(n, dtype=dtype, device=DEV), p, seed)
    want = torch.from_numpy(R.keep_mask(seed, n, p)).to(DEV)
    got = y != 0
    assert torch.equal(got, want), f"{int((got != want).sum())} of {n} elements differ, first at {int((got != want).nonzero()[0])}"
    scale = torch.tensor(R.keep_scale(p), dtype=F32).to(dtype).to(DEV)
    assert bool((y[want] == scale).all()), "kept values are 1 / (1 - p) in the dtype"


# --------------------------------------------------------------------------------------
# b. MHLA core
# --------------------------------------------------------------------------------------
MHLA_B, MHLA_H, MHLA_SEED = 2, 3, 0x1234567800000005
_MHLA_CACHE = {}


def _mhla_case(dtype, L, W, hd, p, masked):
    """Inputs (shared by every p / mask / kernel of one shape) and the float64 reference with the explicit mask;
    computed once and never written to."""
    B, H = MHLA_B, MHLA_H
    D = H * hd
    ikey = (dtype, L, W, hd)
    if ikey not in _MHLA_CACHE:
        g = _gen(L * 31 + W * 7 + hd)
        qkv, dout = _rand((B * L, 3 * D), dtype, g), _rand((B * L, D), dtype, g)
        mask = torch.rand(B, L, L, generator=g, device=DEV) > 0.4          # density and diagonal rule of
        mask |= torch.eye(L, dtype=torch.bool, device=DEV)                 # test_mhla_core_fwd_bwd_vs_window_gather
        _MHLA_CACHE[ikey] = (qkv, dout, mask.to(torch.uint8).contiguous())
    qkv, dout, mask = _MHLA_CACHE[ikey]
    mask = mask if masked else None
    key = ikey + (p, masked)
    if key not in _MHLA_CACHE:
        keep = R.mhla_keep(MHLA_SEED, B, H, L, W, p, DEV) if p > 0 else None
        _MHLA_CACHE[key] = R.mhla_ref(qkv.double(), dout.double(), B, L, H, hd, W, mask, keep, p)
    return qkv, dout, mask, _MHLA_CACHE[key]


def _mhla_check(K, dtype, L, W, hd, p, masked, lse_pair, tag):
    B, H = MHLA_B, MHLA_H
    D = H * hd
    qkv, dout, mask, (o_ref, g_ref, lse_ref) = _mhla_case(dtype, L, W, hd, p, masked)
    if lse_pair:
        out, lse = K.mhla_attn_fwd(qkv, B, L, H, hd, W, mask, p, MHLA_SEED, want_lse=True)
        assert lse is not None
        dqkv = K.mhla_attn_bwd(qkv, dout, B, L, H, hd, W, mask, p, MHLA_SEED, o=out, lse=lse)
    else:
        out = K.mhla_attn_fwd(qkv, B, L, H, hd, W, mask, p, MHLA_SEED)
        dqkv = K.mhla_attn_bwd(qkv, dout, B, L, H, hd, W, mask, p, MHLA_SEED)
    what = f"{tag} L={L} W={W} hd={hd} p={p} mask={masked}"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all()), what
    grp = f"mhla {_name(dtype)}"
    rgrp = f"mhla {_name(dtype)} rows" + (" p=0" if p == 0 else "")
    gate = ROW_GATE[("mhla", dtype)]
    _close(grp + " out", out.float(), o_ref, _tol(dtype), what)
    _rows(rgrp, out.float(), o_ref, B * L, gate, what + " out")
    if lse_pair:
        e = (lse.double() - lse_ref).abs().max().item()      # the lse of the UNDROPPED scores
        _note("mhla lse (abs)", 2e-3, e)
        assert e < 2e-3, f"{what}: lse differs by {e:.3e}"
    gtol = 5e-5 if dtype == F32 else 1.5e-2
    for part, nm in enumerate(("dq", "dk", "dv")):           # separately first: a dK-only error is named
        a, b = dqkv[:, part * D:(part + 1) * D].float(), g_ref[:, part * D:(part + 1) * D]
        _close(grp + " " + nm, a, b, gtol, what)
        _rows(rgrp, a, b, B * L, gate, what + " " + nm)
    _close(grp + " dqkv", dqkv.float(), g_ref, gtol, what)


MHLA_F32 = [(5, 3, 16), (5, 7, 16), (17, 5, 32), (40, 15, 16)]                 # dispatch_dpl<float, 7 | 15>; L < W
MHLA_MFMA = [(12, 7, 64), (40, 3, 32), (33, 9, 128), (65, 7, 64), (70, 7, 64), (197, 7, 64), (40, 11, 64)]
MHLA_LSE = [(L, 7) for L in (8, 17, 48, 49, 70, 197)] + [(40, 11), (100, 3)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("L,W,hd", MHLA_F32)
def test_mhla_fp32_kernels(K, L, W, hd, p, masked):
    """p = 0 is the baseline the fp32 per-row gate is derived from (module docstring)."""
    _mhla_check(K, F32, L, W, hd, p, masked, False, "fp32")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("bwd_kernel", ["default", "tables-switch", "valu"])
@pytest.mark.parametrize("L,W,hd", [(40, 7, 16)] + MHLA_MFMA)
def test_mhla_bf16_kernels(K, L, W, hd, bwd_kernel, p, masked, monkeypatch):
    """hd = 16: the generic bf16 kernels; hd >= 32: the MFMA forward with the default two-owner-pass backward, and
    with the 8-lanes-per-row backward, which both FAVIT_MHLA_VALU ("valu": VALU forward too) and FAVIT_MHLA_BWD_TABLES
    ("tables-switch": MFMA forward) select.  The table formulation itself (mhla_bwd_mfma_kernel) is unreachable from
    the library's entry points, so no case here runs it and its draw stays unchecked."""
    counted = {"tables-switch": "tables switch", "valu": "valu"}.get(bwd_kernel)
    if counted:
        if hd < 32:
            pytest.skip("kernel selection only exists for bf16, hd >= 32")
        _ENTERED[counted] += 1
        monkeypatch.setenv("FAVIT_MHLA_BWD_TABLES" if bwd_kernel == "tables-switch" else "FAVIT_MHLA_VALU", "1")   # read per call
    _mhla_check(K, BF16, L, W, hd, p, masked, False, bwd_kernel)
    if counted:
        _RAN[counted] += 1


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("waves", [0, 1, 4])
@pytest.mark.parametrize("L,W", MHLA_LSE)
def test_mhla_saved_statistics_pair(K, L, W, waves, p, masked, monkeypatch):
    """The training path's pair (forward leaves lse, backward takes it and the output), at the default block size and
    at 1 and 4 tiles per block (the 3- and 5-chunk instantiations), without a mask (<false, N, true>) and with one."""
    _ENTERED["lse"] += 1
    if not K.mhla_attn_lse_supported(L, 64, W, BF16):
        pytest.skip("saved-statistics kernels: bf16, hd = 64, W <= 7 (11 with L > 16), L >= W + 1")
    if waves:
        monkeypatch.setenv("FAVIT_MHLA_LSE_WAVES", str(waves))
    _mhla_check(K, BF16, L, W, 64, p, masked, True, f"lse waves={waves}")
    _RAN["lse"] += 1


# --------------------------------------------------------------------------------------
# c. Fused dense attention
# --------------------------------------------------------------------------------------
SDPA_SEED = 0x1234567800000005
SDPA_SHAPES = [(2, 3, 65, 65, 64, None), (2, 2, 17, 17, 16, None), (3, 2, 5, 41, 32, "full"), (2, 1, 33, 21, 64, "keys"),
               (1, 3, 70, 100, 48, "keys"), (1, 1, 130, 64, 192, None), (2, 2, 1, 1, 16, None), (1, 2, 197, 197, 64, None)]
_SDPA_CACHE = {}


def _sdpa_inputs(dtype, B, H, Lq, Lk, hd, mask_kind, dead_row=None):
    key = (dtype, B, H, Lq, Lk, hd, mask_kind, dead_row)
    if key in _SDPA_CACHE:
        return _SDPA_CACHE[key]
    g = _gen(B * 1000 + Lq * 10 + hd + Lk)
    D = H * hd
    c = {}
    if Lq == Lk:         # q, k, v interleaved in one [B*L, 3D] buffer, as the fused qkv projection writes them
        c["qkv"] = _rand((B * Lq, 3 * D), dtype, g)
        c["qf"], c["kf"], c["vf"] = (c["qkv"].reshape(B, Lq, 3, H, hd)[:, :, s].permute(0, 2, 1, 3) for s in range(3))
    else:
        c["qt"], c["kt"], c["vt"] = _rand((B * Lq, D), dtype, g), _rand((B * Lk, D), dtype, g), _rand((B * Lk, D), dtype, g)
        c["qf"] = c["qt"].reshape(B, Lq, H, hd).permute(0, 2, 1, 3)
        c["kf"], c["vf"] = (t.reshape(B, Lk, H, hd).permute(0, 2, 1, 3) for t in (c["kt"], c["vt"]))
    c["dot"] = _rand((B * Lq, D), dtype, g)
    c["mask"], c["m_sb"], c["m_sq"], c["mb"] = None, 0, 0, None
    if mask_kind == "full":
        mb = torch.rand(B, Lq, Lk, generator=g, device=DEV) > 0.4
        mb[..., 0] = True
        if dead_row is not None:
            mb[dead_row[0], dead_row[1]] = False
        c["mask"], c["m_sb"], c["m_sq"], c["mb"] = mb.to(torch.uint8).contiguous(), Lq * Lk, Lk, mb[:, None]
    elif mask_kind == "keys":
        mk = torch.rand(B, Lk, generator=g, device=DEV) > 0.3
        mk[:, 0] = True
        c["mask"], c["m_sb"], c["m_sq"], c["mb"] = mk.to(torch.uint8).contiguous(), Lk, 0, mk[:, None, None, :]
    _SDPA_CACHE[key] = c
    return c


def _sdpa_ref(c, B, H, Lq, Lk, hd, p):
    rkey = ("ref", p)
    if rkey not in c:
        keep = R.sdpa_keep(SDPA_SEED, B, H, Lq, Lk, p, DEV) if p > 0 else None
        dof = c["dot"].reshape(B, Lq, H, hd).permute(0, 2, 1, 3)
        args = (c["qf"], c["kf"], c["vf"], dof, 1.0 / math.sqrt(hd), c["mb"], keep, p)
        c[rkey] = R.sdpa_ref(*args) + R.sdpa_grad_scale(*args)
    return c[rkey]


def _sdpa_run(K, favit, c, dtype, B, H, Lq, Lk, hd, p):
    """Forward and backward through the library; returns (o, lse, dq, dk, dv) as [B*L, D] tensors (lse [B, H, Lq])."""
    V = favit.functional._View
    D = H * hd
    if Lq == Lk:
        q, k, v = (V(c["qkv"], s * D, 3 * D, Lq * 3 * D, hd) for s in range(3))
    else:
        q, k, v = V(c["qt"], 0, D, Lq * D, hd), V(c["kt"], 0, D, Lk * D, hd), V(c["vt"], 0, D, Lk * D, hd)
    scale = 1.0 / math.sqrt(hd)
    ot = torch.empty((B * Lq, D), dtype=dtype, device=DEV)
    o = V(ot, 0, D, Lq * D, hd)
    lse = K.sdpa_fwd(q, k, v, o, B, H, Lq, Lk, hd, scale, c["mask"], c["m_sb"], c["m_sq"], p, SDPA_SEED)
    dqt = torch.empty((B * Lq, D), dtype=dtype, device=DEV)
    dkt, dvt = (torch.empty((B * Lk, D), dtype=dtype, device=DEV) for _ in range(2))
    K.sdpa_bwd(q, k, v, o, V(c["dot"], 0, D, Lq * D, hd), V(dqt, 0, D, Lq * D, hd), V(dkt, 0, D, Lk * D, hd),
               V(dvt, 0, D, Lk * D, hd), lse, B, H, Lq, Lk, hd, scale, c["mask"], c["m_sb"], c["m_sq"], p, SDPA_SEED)
    return ot, lse.reshape(B, H, Lq), dqt, dkt, dvt


def _merged(t, B, L, H, hd):
    """[B, H, L, hd] -> [B*L, H*hd], the layout the library writes."""
    return t.permute(0, 2, 1, 3).reshape(B * L, H * hd)


def _sdpa_check(K, favit, dtype, B, H, Lq, Lk, hd, mask_kind, p, what, dead_row=None):
    c = _sdpa_inputs(dtype, B, H, Lq, Lk, hd, mask_kind, dead_row)
    o_ref, lse_ref, dq_ref, dk_ref, dv_ref, dq_gross, dk_gross = _sdpa_ref(c, B, H, Lq, Lk, hd, p)
    ot, lse, dqt, dkt, dvt = _sdpa_run(K, favit, c, dtype, B, H, Lq, Lk, hd, p)
    for t in (ot, dqt, dkt, dvt):
        assert bool(torch.isfinite(t.float()).all()), what + ": a non-finite value"
    grp = f"sdpa {_name(dtype)}"
    rgrp = f"sdpa {_name(dtype)} rows" + (" p=0" if p == 0 else "")
    gate = ROW_GATE[("sdpa", dtype)]
    gtol = 5e-5 if dtype == F32 else 2e-2
    _close(grp + " o", ot.float(), _merged(o_ref, B, Lq, H, hd), _tol(dtype), what)
    _rows(rgrp, ot.float(), _merged(o_ref, B, Lq, H, hd), B * Lq, gate, what + " o")
    live = torch.isfinite(lse_ref)
    assert torch.equal(torch.isfinite(lse), live), what + ": lse is -inf exactly on the fully masked rows"
    assert bool((lse[~live] == float("-inf")).all())
    _close(grp + " lse", lse[live], lse_ref[live], 2e-5 + (0 if dtype == F32 else 3e-3), what)   # of the UNDROPPED scores
    # (Lk = 1: dq = dk = 0 identically, measured against the cancelling terms; see R.sdpa_grad_scale)
    for nm, got, ref, gross, L in (("dq", dqt, dq_ref, dq_gross, Lq), ("dk", dkt, dk_ref, dk_gross, Lk), ("dv", dvt, dv_ref, None, Lk)):
        gm = _merged(gross, B, L, H, hd) if gross is not None else None
        _close(grp + " " + nm, got.float(), _merged(ref, B, L, H, hd), gtol, what, gm)
        _rows(rgrp, got.float(), _merged(ref, B, L, H, hd), B * L, gate, what + " " + nm, gm)
    return ot, dqt


@pytest.mark.parametrize("waves", [0, 4, 5])
@pytest.mark.parametrize("dtype,p", [(F32, 0.0), (F32, 0.1), (F32, 0.5), (BF16, 0.1), (BF16, 0.5)])
@pytest.mark.parametrize("B,H,Lq,Lk,hd,mask_kind", SDPA_SHAPES)
def test_sdpa_fused(K, favit, B, H, Lq, Lk, hd, mask_kind, dtype, waves, p, monkeypatch):
    """o, lse, dq, dk, dv of the three kernel modes with a.thresh != 0, at the library's own choice of four or five waves
    and with either forced.  fp32 p = 0 is the baseline of the fp32 per-row gate (bf16 p = 0: test_sdpa_fused_fwd_bwd)."""
    if waves:
        monkeypatch.setenv("FAVIT_SDPA_WAVES", str(waves))
    _sdpa_check(K, favit, dtype, B, H, Lq, Lk, hd, mask_kind, p, f"B={B} H={H} Lq={Lq} Lk={Lk} hd={hd} {mask_kind} waves={waves} p={p}")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_sdpa_fully_masked_query_row(K, favit, dtype, p):
    """The contract of include/favit.h: a query row with every key masked gives o = 0 and lse = -inf, dq = 0 for it and
    nothing in dk / dv; every other row matches the reference and nothing is non-finite."""
    B, H, Lq, Lk, hd = 2, 2, 37, 41, 32
    dead = (1, 5)
    ot, dqt = _sdpa_check(K, favit, dtype, B, H, Lq, Lk, hd, "full", p, f"fully masked row p={p}", dead_row=dead)
    row = dead[0] * Lq + dead[1]
    assert bool((ot[row] == 0).all()) and bool((dqt[row] == 0).all())


# --------------------------------------------------------------------------------------
# d. GEMM epilogue with dropout, per kernel family
# --------------------------------------------------------------------------------------
GEMM_SEED, GEMM_P = 0x1234567800000005, 0.1
_KEEP_CACHE = {}


def _gemm_keep(M, N):
    """keep_mask(seed, m*N + n, p) with the LOGICAL N."""
    if (M, N) not in _KEEP_CACHE:
        _KEEP_CACHE.clear()                                       # one shape at a time: the large ones are 17M elements
        _KEEP_CACHE[(M, N)] = torch.from_numpy(R.keep_mask(GEMM_SEED, M * N, GEMM_P).reshape(M, N)).to(DEV)
    return _KEEP_CACHE[(M, N)]


def _last(favit):
    return favit._abi.lib().favit_gemm_last_kernel().decode()


def _check_dropped_epilogue(group, what, out, plain, res, keep, kept_tol):
    """out: with dropout (+ residual), plain: the same call without dropout and without residual, both [M, N] views."""
    M, N = keep.shape
    assert bool(torch.isfinite(out.float()).all()), what
    r = res if res is not None else torch.zeros((), dtype=out.dtype, device=DEV)
    r = r.expand(M, N)
    # dropped: the residual exactly (0 without one), in the output dtype
    assert torch.equal(out[~keep], r[~keep].to(out.dtype)), f"{what}: a dropped element is not the residual"
    # kept: (out - residual) == plain / (1 - p)
    s = R.keep_scale(GEMM_P)
    want = plain.double() * s
    _close(group, (out.double() - r.double())[keep], want[keep], kept_tol, what + " kept")
    # the dropped set is the mask's set: a kept element equals the residual only where plain / (1 - p) vanishes beside it
    stuck = keep & (out == r.to(out.dtype)) & (want.abs() > 2.0 ** -22 * r.double().abs() + 1e-30)
    assert not bool(stuck.any()), f"{what}: {int(stuck.sum())} kept elements were dropped, first at {stuck.nonzero()[0].tolist()}"
    drop = 1.0 - keep.float().mean().item()
    assert abs(drop - GEMM_P) < 5 * (GEMM_P * (1 - GEMM_P) / (M * N)) ** 0.5 + 1.0 / 65536


def _gemm_epilogue_case(K, favit, in_kind, M, N, Kd, epi, ldc=None, family=None, in_dtype=None):
    """One of the three epilogues functional.lin_fwd / lin_bwd_x issue, with and without dropout.
    in_kind: "f32", "bf16" or "fp8"; fp32 operands write fp32 (the library has no fp32 -> bf16 GEMM)."""
    A_ = favit._abi
    ldc = ldc or N
    g = _gen(M * 7 + N * 3 + Kd + len(epi))
    dt_in = F32 if in_kind == "f32" else BF16
    bk = epi not in ("mulaux", "dgelu") or in_kind == "fp8"          # the input-gradient layout; fp8 is NT only
    a = _rand((M, Kd), dt_in, g, Kd ** -0.5)
    b = _rand((N, Kd) if bk else (Kd, N), dt_in, g)
    kw = dict(b_kmajor=bk)
    if in_dtype is not None:
        kw["in_dtype"] = in_dtype
    if in_kind == "fp8":
        a, _, sa = K.fp8_quantize(a, torch.float8_e4m3fn)
        b, _, sb = K.fp8_quantize(b, torch.float8_e4m3fn)
        kw.update(scale_a=sa, scale_b=sb)
    bias = _rand((N,), F32, g)
    out_dtype = F32 if (epi in ("res", "acc") or in_kind == "f32") else BF16
    res = aux = None
    if epi == "res":
        res = _rand((M, ldc), F32, g)[:, :N]
        kw.update(bias=bias)
    elif epi == "acc":
        kw.update(accumulate=True)
    elif epi == "gelu":
        kw.update(bias=bias, act=A_.ACT_GELU_SAVEGRAD if dt_in == BF16 else A_.ACT_GELU)
    else:
        aux = _rand((M, ldc), dt_in, g)[:, :N]
        kw.update(act=A_.ACT_MULAUX if epi == "mulaux" else A_.ACT_DGELU, aux_in=aux, ld_aux_in=ldc)
    sentinel = 7.0

    def run(drop):
        buf = torch.full((M, ldc), sentinel, dtype=out_dtype, device=DEV)
        k2 = dict(kw)
        pre = None
        if epi == "gelu":
            pre = torch.full((M, ldc), sentinel, dtype=out_dtype, device=DEV)
            k2.update(aux_out=pre, ld_aux_out=ldc)
        if drop:
            k2.update(dropout_p=GEMM_P, dropout_seed=GEMM_SEED)
            if res is not None:
                k2.update(residual=res, ld_res=ldc)
        if epi == "acc":
            if drop:
                buf.copy_(acc0)
            else:
                buf.zero_()
        K.gemm(a, b, buf, M, N, Kd, Kd, b.stride(0), ldc, **k2)
        return buf, pre, _last(favit)

    acc0 = _rand((M, ldc), F32, g) if epi == "acc" else None
    plain, pre0, fam0 = run(False)
    out, pre1, fam1 = run(True)
    what = f"{in_kind} {M}x{N}x{Kd} ldc={ldc} {epi} [{fam1}]"
    print(what)
    assert fam0 == fam1, f"{what}: dropout changed the kernel family ({fam0} without)"
    if family is not None:
        assert fam1 in family, f"{what}: expected one of {family}"
    if ldc != N:
        assert bool((out[:, N:] == sentinel).all()), f"{what}: columns past N were written"
    if pre1 is not None:
        assert torch.equal(pre1[:, :N], pre0[:, :N]), f"{what}: the saved pre-activation / derivative is never dropped"
    kept_tol = 1e-6 if out_dtype == F32 else 1e-2
    r = acc0[:, :N] if epi == "acc" else res
    _check_dropped_epilogue(f"gemm {in_kind} -> {_name(out_dtype)} kept", what, out[:, :N], plain[:, :N], r, _gemm_keep(M, N), kept_tol)
    return fam1


# (id, operands, M, N, K, ldc, families that may run, epilogues, environment)
GEMM_CASES = [
    ("scalar-f32", "f32", 130, 70, 50, None, ("t128",), ("res", "gelu", "mulaux", "dgelu", "acc"), None),
    ("scalar-bf16", "bf16", 130, 70, 50, None, ("t128",), ("res", "gelu", "mulaux", "dgelu"), None),
    ("vector-f32", "f32", 256, 384, 128, None, ("t128",), ("res", "gelu", "mulaux", "acc"), None),
    ("vector-bf16", "bf16", 256, 384, 128, None, ("s64",), ("res", "gelu", "mulaux"), None),
    ("oddN-ldc197-f32", "f32", 130, 197, 64, 197, None, ("res", "gelu", "mulaux"), None),
    ("oddN-ldc200-f32", "f32", 130, 197, 64, 200, None, ("res", "gelu", "mulaux"), None),
    ("oddN-ldc197-bf16", "bf16", 130, 197, 64, 197, None, ("res", "gelu", "mulaux"), None),
    ("oddN-ldc200-bf16", "bf16", 130, 197, 64, 200, None, ("res", "gelu", "mulaux"), None),
    ("s64k2", "bf16", 1000, 200, 256, None, ("s64k2",), ("res", "gelu", "mulaux", "dgelu"), None),
    ("s64", "bf16", 4096, 1152, 384, None, ("s64",), ("res", "gelu", "mulaux"), None),
    ("p4", "bf16", 8192, 1152, 384, None, ("p4",), ("res", "gelu", "mulaux"), None),
    ("K544", "bf16", 8232, 2048, 544, None, ("t128",), ("res", "gelu", "mulaux"), None),
    ("p7", "bf16", 8232, 2048, 576, None, ("p7",), ("res", "gelu"), None),
    ("p7-shape-mn-major-B", "bf16", 8232, 2048, 576, None, ("p4",), ("mulaux",), None),
    ("pp", "bf16", 1024, 200, 128, None, ("pp",), ("res", "gelu", "mulaux"), "FAVIT_GEMM_PP"),
    ("p4f", "f32", 8232, 1152, 400, None, ("p4f", "p4f128"), ("res", "gelu", "mulaux"), None),
    ("p4x3", "f32x3", 32772, 200, 64, None, ("p4x3", "p4x3_128"), ("res", "gelu", "mulaux"), None),
    ("fp8", "fp8", 300, 200, 128, None, ("p4",), ("res", "gelu", "mulaux"), None),
]


@pytest.mark.parametrize("name,kind,M,N,Kd,ldc,family,epis,env", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_dropout_epilogue_per_family(K, favit, name, kind, M, N, Kd, ldc, family, epis, env, monkeypatch):
    """Dropped elements are the residual exactly, kept ones the undropped result times 1 / (1 - p), and the dropped set is
    keep_mask(seed, m*N + n, p) -- for the kernel family that really ran.  (4096, 1152, 384) runs the 64-row kernel
    without the in-workgroup split (144 tiles of 256x128 do not fill the device); (8192, 1152, 384) is the smallest
    multiple that the 256x128 kernel takes.  K = 544 (the shape of test_gemm_256x256_tile_kernel) is no multiple of the
    64-wide DMA step, so that problem runs the generic 128x128 kernel; K = 576 runs the 256x256 kernel, and its
    mn-major-B twin the 256x128 kernel with a quarter-tile tail.  odd N: the element pairs of one draw straddle rows."""
    if env:
        monkeypatch.setenv(env, "1")
    in_dtype = favit._abi.F32X3 if kind == "f32x3" else None
    for epi in epis:
        _gemm_epilogue_case(K, favit, "f32" if kind == "f32x3" else kind, M, N, Kd, epi, ldc, family, in_dtype)


@pytest.mark.parametrize("mode", ["res", "gelu", "mulaux"])
def test_ln_gemm_dropout_epilogue(K, favit, mode):
    """favit_ln_gemm (LayerNorm fused into the 64-row GEMM) with dropout: the same three assertions.  The library takes
    only a k-major B here, so the third epilogue is MULAUX + dropout with the weight as it lies."""
    A_ = favit._abi
    M, D, N = 64 * 65, 192, 576
    g = _gen(M + D + N)
    x = torch.randn(M, D, device=DEV, generator=g) * 1.7 + 0.3
    gamma = torch.randn(D, device=DEV, generator=g) * 0.2 + 1.0
    beta = torch.randn(D, device=DEV, generator=g) * 0.1
    w = (torch.randn(N, D, device=DEV, generator=g) * 0.05).to(BF16)
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    res = _rand((M, N), F32, g) if mode == "res" else None
    out_dtype = F32 if mode == "res" else BF16
    aux = _rand((M, N), BF16, g) if mode == "mulaux" else None
    act = {"res": A_.ACT_NONE, "gelu": A_.ACT_GELU_SAVEGRAD, "mulaux": A_.ACT_MULAUX}[mode]
    outs = []
    for drop in (False, True):
        out = torch.full((M, N), 7.0, dtype=out_dtype, device=DEV)
        pre = torch.full((M, N), 7.0, dtype=BF16, device=DEV) if mode == "gelu" else None
        r = K.ln_gemm(x, D, gamma, beta, w, out, M, N, D, bias=None if aux is not None else bias, act=act, aux_in=aux,
                      ld_aux_in=N if aux is not None else 0, aux_out=pre, residual=res if drop else None, dropout_p=GEMM_P if drop else 0.0, dropout_seed=GEMM_SEED)
        assert r is not None, "the library must take this shape"
        assert _last(favit) == "s64ln"
        outs.append((out, pre, r))
    (plain, pre0, r0), (out, pre1, r1) = outs
    assert all(torch.equal(u, v) for u, v in zip(r0, r1)), "xn / mean / rstd do not depend on dropout"
    if pre1 is not None:
        assert torch.equal(pre0, pre1)
    _check_dropped_epilogue(f"gemm ln -> {_name(out_dtype)} kept", f"ln_gemm {mode}", out, plain, res, _gemm_keep(M, N),
                            1e-6 if out_dtype == F32 else 1e-2)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gemm_dropout_refusals(K, favit, dtype):
    """split_k > 1 and batch > 1 together with dropout: FAVIT_ERR_UNSUPPORTED and C untouched.  (accumulate = 1 with
    dropout is not refused: the "acc" epilogue above checks what it computes.)"""
    g = _gen(17)
    M, N, Kd, Bz = 256, 128, 256, 3
    a, b = _rand((Bz, M, Kd), dtype, g), _rand((Bz, N, Kd), dtype, g)
    C = torch.full((Bz, M, N), 7.0, device=DEV)
    drop = dict(dropout_p=GEMM_P, dropout_seed=GEMM_SEED)
    _raises_code(-2, K.gemm, a, b, C, M, N, Kd, Kd, Kd, N, split_k=2, **drop)
    _raises_code(-2, K.gemm, a, b, C, M, N, Kd, Kd, Kd, N, batch=Bz, sA=(M * Kd, 0), sB=(N * Kd, 0), sC=(M * N, 0), **drop)
    _raises_code(-2, K.gemm, a, b, C, M, N, Kd, Kd, Kd, N, batch=Bz, split_k=2, sA=(M * Kd, 0), sB=(N * Kd, 0),
                 sC=(M * N, 0), **drop)
    torch.cuda.synchronize()
    assert bool((C == 7.0).all()), "a refused call must not have launched"
    # the same calls without dropout are taken
    K.gemm(a, b, C, M, N, Kd, Kd, Kd, N, split_k=2)
    K.gemm(a, b, C, M, N, Kd, Kd, Kd, N, batch=Bz, sA=(M * Kd, 0), sB=(N * Kd, 0), sC=(M * N, 0))
    _close("gemm refusals: the undropped twin", C, a.double() @ b.double().transpose(1, 2), 2e-5)
