"""Dense attention at head widths the fused kernel does not take (hd % 16 != 0): functional.sdpa_fwd / sdpa_bwd then run
a batched Q.K^T GEMM, favit_softmax_fwd and a batched P.V GEMM, and four more batched GEMMs around favit_softmax_bwd.

  1. the chain at op level, through functional.sdpa_fwd / sdpa_bwd (the branch choice is under test: every case asserts
     that two GEMMs ran forward, four backward, and that (P, Pd) was saved), laid out as the modules lay it out:
     interleaved [B*L, 3D] qkv with dq / dk / dv as views of one dqkv buffer, separate buffers where Lq != Lk.
     Reference: _dropout_ref.sdpa_ref (float64, explicit dropout mask) from the dtype-rounded inputs.  Output buffers
     start as NaN, so an element the chain does not write fails the finiteness check;
  2. favit_softmax_fwd / _bwd alone at the edges of their one-wave-per-row layout (Lk around 64, 1 to 4 live waves in
     the last workgroup, the three mask forms with z / H), per row, and one case that fails without the max subtraction;
  3. fully masked query rows: the contract of include/favit.h (o = 0, dq = 0, nothing into dk / dv, nothing non-finite,
     P = Pd = 0) for the unfused chain and for the softmax kernel;
  4. the modules (vit.MultiHeadAttention, vit.TransformerBlock, vit_mhla.TransformerBlock(use_mhla=False),
     CrossAttention, MultiHeadCrossAttention, CrossAttentionTransformerBlock) at hd 24, 20, 12, 40 and the hd-32 fused
     controls against oracle/favit_oracle.py in float64 (pinned to the goldens by tests/test_head_widths_host.py), in
     every compute mode; a dead mask row; train-mode attention dropout against finite differences; and the refusals of
     MultiHeadLatentAttention at head widths its fold has no instantiation for.

Gates.  Op level, global rel-L2: o 2e-5 / 1e-2, gradients 5e-5 / 2e-2 (test_sdpa_fused_fwd_bwd).  Op level per row
(denominator of test_gpu_dropout_masks._rows): bf16 6e-2 (ROW_GATE there); fp32 the global gates applied row by row.
No gate had to be measured.  Worst figures of a whole-module run on an MI355X (printed at teardown, visible with -s):
op level fp32 o 3.4e-7, gradients 3.8e-7, rows 5.2e-7 / 1.2e-5; bf16 o 2.8e-3, gradients 3.0e-3, rows 4.2e-3 / 4.6e-2 (a
row of dk of (3, 2, 5, 41, 24, full) at p = 0.5: few query rows keep that key; 5.4e-3 at p = 0); softmax kernel fp32 2.4e-7 (P, Pd), 9.9e-6 (dS),
bf16 3.8e-3; modules fp32 and fp32x3 3.1e-7 / 6.5e-7, bf16 3.5e-3 / 8.7e-3, fp8 1.8e-2 and 1.9 % on gradient norms.  Softmax kernel per row: fp32 2e-5 (P, Pd) and 5e-5 (dS), the gates above; bf16
4e-3: every stored element is one round-to-nearest of an fp32 value and bf16 keeps 8 significant bits, so its relative
error is at most 2^-8 = 3.906e-3 and a correct row is within that of the float64 row in rel-L2 (a one-key row with
dropout, P / (1 - p) = 1.111 -> 1.109, comes close to the bound); the fp32 arithmetic before the rounding adds ~1e-5 at
most.  The bound is a guarantee of the format, not a typical value, so the gate sits right above it.  A wrong element,
mask byte or draw is an O(1) row error.  Module level: the gates of test_gpu_modules.py for the mode (fp32 and
fp32x3 1e-4 / 5e-4, bf16 2e-2 / 4e-2, fp8 those of test_cfg2_fp8_mode_within_stated_tolerance: 0.15 and gradient norms
within 25 %); analytically zero gradients as test_gpu_modules._run handles them."""
import math

import numpy as np
import pytest
import torch

import _dropout_ref as R
import test_gpu_dropout_masks as DM          # _sdpa_inputs / _sdpa_ref / _merged: the inputs and references of the fused tests
from conftest import rel_l2
from oracle import favit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SEED = DM.SDPA_SEED
GEMM_FAMILIES = {"t128", "s64", "s64k2", "p4", "p7", "pp", "p4f", "p4f128", "p4x3", "p4x3_128"}
ROW_BF16 = DM.ROW_GATE[("sdpa", BF16)]
SM_ROW = {F32: (2e-5, 5e-5), BF16: (4e-3, 4e-3)}        # softmax kernel per row: (P / Pd, dS)

_WORST = {}
_RAN = {"op": 0, "op dead row": 0, "draw": 0, "softmax": 0, "softmax dead": 0, "module": 0, "module key bias": 0,
        "module dead row": 0, "finite differences": 0, "refusal": 0}
_ENTERED = dict(_RAN)
# a whole-module run: 9 shapes x 2 dtypes x 3 p; 2 x 2 x 2; 2 x 2; 7 row layouts x 2 dtypes x (5 Lk x 3 masks x 2 p) + 2
# large-score cases; 2 x 2; self modules 7 (D, H) x 3 modes x (3 + 3 + 6) + 9 in fp8, cross modules 3 modes x 4 x
# (7 + 7 + 3 + 3), and the cross modules again for the key bias; 2 x 2; 6 families; 2
_NEED = {"op": 54, "op dead row": 8, "draw": 4, "softmax": 422, "softmax dead": 4, "module": 501, "module key bias": 240,
         "module dead row": 4, "finite differences": 6, "refusal": 2}


@pytest.fixture(scope="module")
def K(favit, request):
    favit.functional.set_dropout_epoch(None)        # seeds as given: the host restatement knows no epoch word
    yield favit.kernels
    for (group, gate), e in sorted(_WORST.items()):
        print(f"\n[head widths] {group}: worst {e:.3e} (gate {gate:g})", end="")
    print(f"\n[head widths] cases run: {_RAN}")
    cfg = request.config
    whole = not cfg.getoption("keyword") and not any("::" in a for a in cfg.args)
    for k, need in _NEED.items():       # a selection is held to what it entered, a whole-module run to the full grid
        want = need if whole else min(need, _ENTERED[k])
        assert _RAN[k] >= want and _RAN[k] == _ENTERED[k], f"{k}: {_RAN[k]} of {_ENTERED[k]} cases ran, {want} needed"


@pytest.fixture(autouse=True)
def _fp32_mode(favit):
    favit.set_compute_dtype("fp32")
    yield
    favit.set_compute_dtype("fp32")


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _note(group, gate, e):
    _WORST[(group, gate)] = max(_WORST.get((group, gate), 0.0), e)


def _close(group, got, ref, tol, what="", gross=None):
    """test_gpu_dropout_masks._close, recorded in this module's table."""
    e = rel_l2(got, ref)
    if DM._vanishes(ref, gross):
        e = (got.double() - ref.double()).norm().item() / max(gross.double().norm().item(), 1e-300)
    _note(group, tol, e)
    print(f"{group} {what}: rel-L2 {e:.3e} (gate {tol:g})")
    assert math.isfinite(e) and e < tol, f"{group} {what}: rel-L2 {e:.3e} >= {tol:g}"


def _rows(group, got, ref, rows, gate, what="", gross=None):
    """test_gpu_dropout_masks._rows, recorded in this module's table."""
    a, b = got.double().reshape(rows, -1), ref.double().reshape(rows, -1)
    d = gross.double().reshape(rows, -1) if DM._vanishes(ref, gross) else b
    err = (a - b).norm(dim=-1) / (d.norm(dim=-1) + 1e-3 * d.norm() / rows ** 0.5).clamp_min(1e-300)
    e = err.max().item()
    _note(group, gate, e)
    print(f"{group} {what}: worst row {e:.3e} at row {int(err.argmax())} (gate {gate:g})")
    assert math.isfinite(e) and e < gate, f"{group} {what}: per-row error {e:.3e} at row {int(err.argmax())} >= {gate:g}"


def _last(favit):
    return favit._abi.lib().favit_gemm_last_kernel().decode()


def _finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


# --------------------------------------------------------------------------------------
# 1. The unfused chain through functional.sdpa_fwd / sdpa_bwd
# --------------------------------------------------------------------------------------
OP_CASES = [
    (2, 4, 17, 17, 24, None),       # vector loads on, K % 16 != 0
    (2, 4, 33, 33, 20, "keys"),     # bf16 operand strides break the 16-byte loads
    (2, 6, 40, 40, 12, "full"),     # hd < 16
    (2, 4, 9, 9, 10, None),         # C stride no multiple of 4
    (1, 4, 19, 19, 5, "full"),      # odd hd, nothing aligned
    (2, 3, 21, 64, 40, "keys"),     # hd > 16, Lq != Lk, Lk a multiple of 8
    (3, 2, 5, 41, 24, "full"),      # odd Lk as the leading dimension of P
    (2, 2, 1, 1, 24, None),         # one row, one key
    (1, 3, 65, 130, 72, None),      # one tile boundary in each of Lq, Lk
]


def _unfused_run(favit, c, dtype, B, H, Lq, Lk, hd, p):
    """Forward and backward through functional.sdpa_fwd / sdpa_bwd; returns (o, dq, dk, dv) as [B*L, D] tensors and the
    saved (P, Pd).  Asserts that the unfused branch ran: (P, Pd) saved, two GEMMs forward and four backward."""
    Fn, Kk = favit.functional, favit.kernels
    V = Fn._View
    D = H * hd
    nan = float("nan")
    if Lq == Lk:        # as DenseChain lays it out: q, k, v column blocks of one projection output, dqkv likewise
        q, k, v = (V(c["qkv"], s * D, 3 * D, Lq * 3 * D, hd) for s in range(3))
        dqkv = torch.full((B * Lq, 3 * D), nan, dtype=dtype, device=DEV)
        dq, dk, dv = (V(dqkv, s * D, 3 * D, Lq * 3 * D, hd) for s in range(3))
        grads = tuple(dqkv[:, s * D:(s + 1) * D] for s in range(3))
    else:               # as CrossChain lays it out
        q, k, v = V(c["qt"], 0, D, Lq * D, hd), V(c["kt"], 0, D, Lk * D, hd), V(c["vt"], 0, D, Lk * D, hd)
        grads = tuple(torch.full((B * L, D), nan, dtype=dtype, device=DEV) for L in (Lq, Lk, Lk))
        dq, dk, dv = (V(t, 0, D, L * D, hd) for t, L in zip(grads, (Lq, Lk, Lk)))
    ot = torch.full((B * Lq, D), nan, dtype=dtype, device=DEV)
    o = V(ot, 0, D, Lq * D, hd)
    scale = 1.0 / math.sqrt(hd)
    margs = (c["mask"], c["m_sb"], c["m_sq"], p, SEED)
    assert Kk.GEMM_TRACE is None
    try:
        Kk.GEMM_TRACE = []
        saved = Fn.sdpa_fwd(q, k, v, o, B, H, Lq, Lk, hd, scale, *margs)
        fwd, last = [e[5] for e in Kk.GEMM_TRACE], _last(favit)
        Kk.GEMM_TRACE = []
        Fn.sdpa_bwd(q, k, v, o, V(c["dot"], 0, D, Lq * D, hd), dq, dk, dv, saved, B, H, Lq, Lk, hd, scale, *margs)
        bwd = [e[5] for e in Kk.GEMM_TRACE]
    finally:
        Kk.GEMM_TRACE = None
    assert len(saved) == 2, "functional.sdpa_fwd took the fused branch"
    assert len(fwd) == 2 and len(bwd) == 4 and set(fwd + bwd) <= GEMM_FAMILIES, (fwd, bwd)
    assert last == fwd[-1] and last in GEMM_FAMILIES, f"last kernel after the forward: {last}"
    assert (saved[1] is saved[0]) == (p == 0)
    return ot, grads, saved


def _op_check(favit, dtype, B, H, Lq, Lk, hd, mask_kind, p, dead_row=None):
    what = f"B={B} H={H} Lq={Lq} Lk={Lk} hd={hd} {mask_kind} p={p}" + (f" dead={dead_row}" if dead_row else "")
    c = DM._sdpa_inputs(dtype, B, H, Lq, Lk, hd, mask_kind, dead_row)
    o_ref, _, dq_ref, dk_ref, dv_ref, dq_gross, dk_gross = DM._sdpa_ref(c, B, H, Lq, Lk, hd, p)
    ot, (dqt, dkt, dvt), (P, Pd) = _unfused_run(favit, c, dtype, B, H, Lq, Lk, hd, p)
    assert _finite(ot, dqt, dkt, dvt, P, Pd), what + ": a non-finite (or unwritten) value"
    grp = f"op {_name(dtype)}"
    rgrp = grp + " rows" + (" p=0" if p == 0 else "")
    otol, gtol = (2e-5, 5e-5) if dtype == F32 else (1e-2, 2e-2)
    orow, grow = (otol, gtol) if dtype == F32 else (ROW_BF16, ROW_BF16)
    _close(grp + " o", ot.float(), DM._merged(o_ref, B, Lq, H, hd), otol, what)
    _rows(rgrp + " o", ot.float(), DM._merged(o_ref, B, Lq, H, hd), B * Lq, orow, what + " o")
    for nm, got, ref, gross, L in (("dq", dqt, dq_ref, dq_gross, Lq), ("dk", dkt, dk_ref, dk_gross, Lk), ("dv", dvt, dv_ref, None, Lk)):
        gm = DM._merged(gross, B, L, H, hd) if gross is not None else None
        _close(grp + " " + nm, got.float(), DM._merged(ref, B, L, H, hd), gtol, what, gm)
        _rows(rgrp + " grads", got.float(), DM._merged(ref, B, L, H, hd), B * L, grow, what + " " + nm, gm)
    return ot, dqt, P, Pd


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("B,H,Lq,Lk,hd,mask_kind", OP_CASES)
def test_unfused_chain(K, favit, B, H, Lq, Lk, hd, mask_kind, dtype, p):
    _ENTERED["op"] += 1
    _op_check(favit, dtype, B, H, Lq, Lk, hd, mask_kind, p)
    _RAN["op"] += 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_softmax_dropout_draw_is_the_fused_kernels_draw(K, dtype, p):
    """The softmax kernel's counter is row*Lk + k with row = (b*H + h)*Lq + q, the index of R.sdpa_keep: with S = 0
    every probability is 1 / Lk > 0, so Pd != 0 is the keep mask, bit for bit."""
    _ENTERED["draw"] += 1
    B, H, Lq, Lk = 2, 3, 21, 65
    S = torch.zeros(B * H, Lq, Lk, device=DEV)
    P, Pd = K.softmax_fwd(S, dtype, H, B * H, Lq, Lk, None, 0, 0, p, SEED)
    keep = R.sdpa_keep(SEED, B, H, Lq, Lk, p, DEV).reshape(B * H, Lq, Lk)
    assert bool((P != 0).all())
    got = Pd != 0
    assert torch.equal(got, keep), f"{int((got != keep).sum())} of {keep.numel()} slots differ"
    want = (torch.tensor(1.0 / Lk, dtype=F32) * R.keep_scale(p)).to(dtype).to(DEV)
    assert bool((Pd[keep] == want).all()), "kept slots are P / (1 - p) in the dtype"
    _RAN["draw"] += 1


# --------------------------------------------------------------------------------------
# 2. favit_softmax_fwd / favit_softmax_bwd alone
# --------------------------------------------------------------------------------------
SM_LAYOUTS = [(1, 1, 1), (3, 1, 1), (3, 3, 1), (2, 1, 2), (1, 1, 5), (5, 1, 1), (6, 3, 9)]      # (Z, H, Lq): Z*Lq = 1, 3, 3, 4, 5, 5, 54
SM_LK = [1, 63, 64, 65, 130]


def _sm_mask(kind, Z, H, Lq, Lk, g, dead=None):
    """(uint8 mask, m_sb, m_sq, bool [Z, Lq, Lk]) for "none" / "full" / "keys"; dead: ("row", b, q) or ("image", b)."""
    Bm = Z // H
    if kind == "none":
        return None, 0, 0, None
    if kind == "full":
        mb = torch.rand(Bm, Lq, Lk, generator=g, device=DEV) > 0.4
        mb[..., 0] = True
        if dead is not None:
            mb[dead[1], dead[2]] = False
        return mb.to(torch.uint8).contiguous(), Lq * Lk, Lk, mb.repeat_interleave(H, 0)
    mk = torch.rand(Bm, Lk, generator=g, device=DEV) > 0.3
    mk[:, 0] = True
    if dead is not None:
        mk[dead[1]] = False
    return mk.to(torch.uint8).contiguous(), Lk, 0, mk[:, None, :].expand(Bm, Lq, Lk).repeat_interleave(H, 0)


def _softmax_ref(S64, mb):
    """float64 softmax of the masked scores; a row with every key masked is 0 (R._sdpa_probs)."""
    if mb is None:
        return torch.softmax(S64, -1)
    dead = ~mb.any(-1, keepdim=True)
    return torch.softmax(S64.masked_fill(~mb, float("-inf")).masked_fill(dead, 0.0), -1).masked_fill(dead | ~mb, 0.0)


def _softmax_case(K, dtype, Z, H, Lq, Lk, kind, p, g, S=None, dead=None, backward=True):
    what = f"Z={Z} H={H} Lq={Lq} Lk={Lk} {kind} p={p}" + (f" dead={dead}" if dead else "")
    rows = Z * Lq
    if S is None:
        S = torch.randn(Z, Lq, Lk, generator=g, device=DEV) * 3      # the scale of test_softmax_fwd_bwd
    mask, m_sb, m_sq, mb = _sm_mask(kind, Z, H, Lq, Lk, g, dead)
    P, Pd = K.softmax_fwd(S, dtype, H, Z, Lq, Lk, mask, m_sb, m_sq, p, SEED)
    assert (Pd is P) == (p == 0) and _finite(P, Pd), what
    P_ref = _softmax_ref(S.double(), mb)
    keep = R.sdpa_keep(SEED, Z, 1, Lq, Lk, p, DEV).reshape(Z, Lq, Lk).double() / (1.0 - p) if p > 0 else None
    grp = f"softmax {_name(dtype)}"
    ptol, stol = SM_ROW[dtype]
    _rows(grp + " P", P.float(), P_ref, rows, ptol, what + " P")
    if mb is not None:
        assert bool((P[~mb] == 0).all()) and bool((Pd[~mb] == 0).all()), what + ": a masked entry is not 0"
    if p > 0:
        _rows(grp + " Pd", Pd.float(), P_ref * keep, rows, ptol, what + " Pd")
        assert bool((Pd[keep == 0] == 0).all()), what + ": a dropped entry is not 0"
    if backward:
        dPd = torch.randn(Z, Lq, Lk, generator=g, device=DEV)
        dS = K.softmax_bwd(P, dPd, Z, Lq, Lk, p, SEED)
        assert _finite(dS), what
        Pk = P.double()                         # backward takes the stored P: the reference starts from it too
        dp = dPd.double() * keep if p > 0 else dPd.double()
        _rows(grp + " dS", dS.float(), Pk * (dp - (Pk * dp).sum(-1, keepdim=True)), rows, stol, what + " dS")
    return P, Pd, mb


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("Z,H,Lq", SM_LAYOUTS)
def test_softmax_kernel_edges(K, Z, H, Lq, dtype):
    """One wave per row, four rows per workgroup, lanes striding Lk by 64: Lk on either side of 64 and past 128, 1 to 4
    live waves in the last workgroup, every mask form (z / H picks the image), with and without dropout, per row."""
    g = _gen(Z * 100 + H * 10 + Lq)
    for Lk in SM_LK:
        for kind in ("none", "full", "keys"):
            for p in (0.0, 0.1):
                _ENTERED["softmax"] += 1
                _softmax_case(K, dtype, Z, H, Lq, Lk, kind, p, g)
                _RAN["softmax"] += 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_softmax_kernel_subtracts_the_row_maximum(K, dtype):
    """Scores at scale 30 with a per-row offset of +-200: exp overflows (or every term underflows) without the max
    subtraction, which unit-scale scores never show.  Forward only: such rows are one-hot to within 1e-10 or less, so
    dS = P (dp - sum P dp) is the rounding residue of a cancellation in fp32 and float64 alike."""
    _ENTERED["softmax"] += 1
    Z, H, Lq, Lk = 6, 3, 9, 130
    g = _gen(77)
    S = torch.randn(Z, Lq, Lk, generator=g, device=DEV) * 30
    S += (torch.randint(0, 2, (Z, Lq, 1), generator=g, device=DEV).float() * 2 - 1) * 200
    _softmax_case(K, dtype, Z, H, Lq, Lk, "full", 0.1, g, S=S, backward=False)
    _RAN["softmax"] += 1


# --------------------------------------------------------------------------------------
# 3. Fully masked query rows
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("B,H,Lq,Lk,hd,dead", [(2, 6, 40, 40, 12, (1, 5)), (3, 2, 5, 41, 24, (2, 3))])
def test_unfused_chain_fully_masked_query_row(K, favit, B, H, Lq, Lk, hd, dead, dtype, p):
    """include/favit.h, for both branches: o = 0 and dq = 0 on the dead row, nothing into dk / dv (every other row
    matches the reference, which has P = 0 there), nothing non-finite, P = Pd = 0 on the row."""
    _ENTERED["op dead row"] += 1
    ot, dqt, P, Pd = _op_check(favit, dtype, B, H, Lq, Lk, hd, "full", p, dead_row=dead)
    row = dead[0] * Lq + dead[1]
    assert bool((ot[row] == 0).all()) and bool((dqt[row] == 0).all())
    z = slice(dead[0] * H, (dead[0] + 1) * H)
    assert bool((P[z, dead[1]] == 0).all()) and bool((Pd[z, dead[1]] == 0).all())
    _RAN["op dead row"] += 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("kind,dead", [("full", ("row", 1, 4)), ("keys", ("image", 0))])
def test_softmax_kernel_fully_masked_rows(K, kind, dead, dtype):
    """A dead row ("full") and a whole dead image ("keys"): P = Pd = 0 and dS = 0 there, the other rows as always."""
    _ENTERED["softmax dead"] += 1
    Z, H, Lq, Lk = 6, 3, 9, 65
    for p in (0.0, 0.1):
        P, Pd, mb = _softmax_case(K, dtype, Z, H, Lq, Lk, kind, p, _gen(5), dead=dead)
        gone = ~mb.any(-1)
        assert int(gone.sum()) == (H if kind == "full" else H * Lq)
        assert bool((P[gone] == 0).all()) and bool((Pd[gone] == 0).all())
        dS = K.softmax_bwd(P, torch.randn(Z, Lq, Lk, generator=_gen(6), device=DEV), Z, Lq, Lk, p, SEED)
        assert _finite(dS) and bool((dS[gone] == 0).all())
    _RAN["softmax dead"] += 1


# --------------------------------------------------------------------------------------
# 4. Modules
# --------------------------------------------------------------------------------------
MODE_TOL = {"fp32": (1e-4, 5e-4), "fp32x3": (1e-4, 5e-4), "bf16": (2e-2, 4e-2)}
DH = [(96, 4), (192, 8), (80, 4), (72, 6), (120, 3), (64, 2), (128, 4)]      # hd 24, 24, 20, 12, 40; 32, 32 (fused controls)
CA_D = [72, 40, 96]                                                          # CrossAttention: one head of width D
SELF_L = [5, 17, 65]
CROSS_L = [(5, 40), (33, 21)]
MB = 2


def _build(favit, seed, make):
    """The module with torch's default initialisation under a fixed seed; every vector (biases, LayerNorm) perturbed so
    that none stays at its 0 / 1 default."""
    torch.manual_seed(seed)
    m = make(favit.models)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for prm in m.parameters():
            if prm.dim() == 1:
                prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    return m.to(DEV)


def _spy_softmax(favit, monkeypatch):
    calls = {"n": 0}
    real = favit.kernels.softmax_fwd

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(favit.kernels, "softmax_fwd", counted)
    return calls


def _module_check(favit, mode, m, oracle, ins, kw, what, unfused, calls, vanishing="check"):
    """Output, input gradients and every parameter gradient against the float64 oracle (test_gpu_modules._run).
    vanishing: "check" the analytically zero gradients with everything else, "skip" them, or check them "only"."""
    favit.set_compute_dtype(mode)
    m.eval()
    for prm in m.parameters():
        prm.grad = None
    xs = [t.detach().clone().requires_grad_(True) for t in ins]
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    x64 = [t.detach().double().clone().requires_grad_(True) for t in ins]
    n0 = calls["n"]
    y = m(*xs, **kw)
    assert (calls["n"] > n0) == unfused, what + ": the other attention branch ran"
    y64 = oracle(sd, *x64)
    gout = torch.randn(y.shape, generator=_gen(y.numel()), device=DEV)
    (y * gout).sum().backward()
    (y64 * gout.double()).sum().backward()
    if mode == "fp8":
        e = rel_l2(y.detach(), y64.detach())
        _note("module fp8 out", 0.15, e)
        assert e < 0.15, f"{what}: forward {e:.3e}"
        for k, prm in m.named_parameters():
            r = sd[k].grad.norm().item()
            e = abs(prm.grad.double().norm().item() - r) / max(r, 1e-12)
            _note("module fp8 gradient norms", 0.25, e)
            assert e < 0.25, f"{what}: gradient norm of {k} off by {e:.3f}"
        return
    ftol, gtol = MODE_TOL[mode]
    if vanishing != "only":
        e = rel_l2(y.detach(), y64.detach())
        _note(f"module {mode} out", ftol, e)
        assert e < ftol, f"{what}: forward {e:.3e}"
        for i, (t, r) in enumerate(zip(xs, x64)):
            e = rel_l2(t.grad, r.grad)
            _note(f"module {mode} grads", gtol, e)
            assert e < gtol, f"{what}: grad input {i}: {e:.3e}"
    seen = 0
    for k, prm in m.named_parameters():
        ref = sd[k].grad
        got = prm.grad if prm.grad is not None else torch.zeros_like(prm)
        if ref.abs().max().item() < 1e-5:         # analytically zero (the key bias of the cross modules)
            seen += 1
            if vanishing == "skip":
                continue
            z = got.abs().max().item()
            _note(f"module {mode} zero gradients (abs)", 1e-4, z)
            print(f"{what}: {k} max {z:.3e}")
            assert z < 1e-4, f"{what}: {k} should vanish, max {z:.3e}"
        elif vanishing == "only":
            continue
        else:
            e = rel_l2(got, ref)
            _note(f"module {mode} grads", gtol, e)
            assert e < gtol, f"{what}: grad {k}: {e:.3e}"
    return seen


def _self_inputs(D, L, seed):
    g = _gen(seed)
    x = torch.randn(MB, L, D, generator=g, device=DEV)
    keep = torch.rand(MB, L, generator=g, device=DEV) > 0.3
    keep[:, 0] = True
    return x, keep


def _cross_inputs(D, Lq, Lk, seed):
    g = _gen(seed)
    q, kv = torch.randn(MB, Lq, D, generator=g, device=DEV), torch.randn(MB, Lk, D, generator=g, device=DEV)
    mask = torch.rand(MB, Lq, Lk, generator=g, device=DEV) > 0.4
    mask[..., 0] = True
    return q, kv, mask.to(torch.uint8)


def _self_family(favit, monkeypatch, mode, D, H, family):
    unfused = (D // H) % 16 != 0
    calls = _spy_softmax(favit, monkeypatch)
    make, oracle = {
        "mha": (lambda M: M.vit.MultiHeadAttention(D, H), lambda mask: lambda sd, x: O.dense_mha(x, sd, "", H)),
        "vit_block": (lambda M: M.vit.TransformerBlock(D, H), lambda mask: lambda sd, x: O.vit_block(x, sd, "", H)),
        "vm_block": (lambda M: M.vit_mhla.TransformerBlock(D, H, use_mhla=False),
                     lambda mask: lambda sd, x: O.vit_mhla_block(x, sd, "", H, 7, False, mask)),
    }[family]
    m = _build(favit, D * 7 + H, make)
    for L in SELF_L:
        x, keep = _self_inputs(D, L, D + L)
        for masked in ((False, True) if family == "vm_block" else (False,)):
            _ENTERED["module"] += 1
            kw = {"attention_mask": keep} if masked else {}
            _module_check(favit, mode, m, oracle(keep if masked else None), [x], kw,
                          f"{family}({D}, {H}) L={L} mask={masked} {mode}", unfused, calls)
            _RAN["module"] += 1


@pytest.mark.parametrize("mode", ["fp32", "fp32x3", "bf16"])
@pytest.mark.parametrize("D,H", DH)
@pytest.mark.parametrize("family", ["mha", "vit_block", "vm_block"])
def test_self_attention_modules(K, favit, monkeypatch, family, D, H, mode):
    """L = 5, 17, 65; the nn.MultiheadAttention-style block also with a key-keep mask [B, L]."""
    _self_family(favit, monkeypatch, mode, D, H, family)


@pytest.mark.parametrize("family", ["vit_block", "vm_block"])
def test_self_attention_blocks_fp8_mode(K, favit, monkeypatch, family):
    """(192, 8): D is a multiple of 64, so fp8 mode takes the blocks' nn.Linear GEMMs; attention stays the unfused bf16
    chain at hd 24."""
    _self_family(favit, monkeypatch, "fp8", 192, 8, family)


def _cross_family(favit, monkeypatch, mode, D, H, family, vanishing, counter):
    hd = D if family in ("ca", "ca_block") else D // H
    unfused = hd % 16 != 0
    calls = _spy_softmax(favit, monkeypatch)
    make, oracle = {
        "ca": (lambda M: M.attention.CrossAttention(D), lambda mk: lambda sd, q, kv: O.cross_attention(q, kv, sd, "", mk)),
        "mhca": (lambda M: M.attention.MultiHeadCrossAttention(D, H),
                 lambda mk: lambda sd, q, kv: O.multihead_cross_attention(q, kv, sd, "", H, mk)),
        "ca_block": (lambda M: M.attention.CrossAttentionTransformerBlock(D, H, use_multi_head=False),
                     lambda mk: lambda sd, q, kv: O.cross_block(q, kv, sd, "", H, False, mk)),
        "mhca_block": (lambda M: M.attention.CrossAttentionTransformerBlock(D, H, use_multi_head=True),
                       lambda mk: lambda sd, q, kv: O.cross_block(q, kv, sd, "", H, True, mk)),
    }[family]
    m = _build(favit, D * 11 + H, make)
    failed = []
    for Lq, Lk in CROSS_L:
        q, kv, mask = _cross_inputs(D, Lq, Lk, D + Lq)
        for masked in (False, True):
            _ENTERED[counter] += 1
            kw = {"attention_mask": mask} if masked else {}
            try:
                seen = _module_check(favit, mode, m, oracle(mask if masked else None), [q, kv], kw,
                                     f"{family}({D}, {H}) Lq={Lq} Lk={Lk} mask={masked} {mode}", unfused, calls, vanishing)
                assert seen == 1, "k_proj.bias is the one parameter whose gradient vanishes"
            except AssertionError as err:
                if vanishing != "only":
                    raise
                failed.append(str(err))         # every sub-case is measured and counted before the test fails
            _RAN[counter] += 1
    assert not failed, "\n".join(failed)


CROSS_GRID = [(f, D, H) for f in ("mhca", "mhca_block") for D, H in DH] + [(f, D, 4) for f in ("ca", "ca_block") for D in CA_D]


@pytest.mark.parametrize("mode", ["fp32", "fp32x3", "bf16"])
@pytest.mark.parametrize("family,D,H", CROSS_GRID)
def test_cross_attention_modules(K, favit, monkeypatch, family, D, H, mode):
    """(Lq, Lk) = (5, 40) and (33, 21), with and without a [B, Lq, Lk] mask: the output and every gradient that does not
    vanish analytically (k_proj.bias does: the test below)."""
    _cross_family(favit, monkeypatch, mode, D, H, family, "skip", "module")


@pytest.mark.parametrize("mode", ["fp32", "fp32x3", "bf16"])
@pytest.mark.parametrize("family,D,H", CROSS_GRID)
def test_cross_attention_modules_key_bias_gradient_vanishes(K, favit, monkeypatch, family, D, H, mode):
    """The same cases, the one analytically zero gradient: softmax is invariant to a per-query constant, so k_proj.bias
    gets none.  Handled as test_gpu_modules._run handles such gradients in every mode: where the reference's is below
    1e-5, the module's is below 1e-4 in absolute value.

    This test found that bf16 mode did not meet the bound, at fused and unfused widths alike: CrossChain.bwd took the
    bias gradient as the column sum of the stored dk, whose exact value is 0, so what was left was the sum of B * Lk
    bf16 roundings of elements of size 0.1 to 1 -- 5.6e-4 (mhca(192, 8), Lq 5, Lk 40) to 5.9e-3 (ca(96), Lq 33, Lk 21,
    masked) over the 80 bf16 sub-cases.  The chain now does not form that sum: the gradient is zero by the identity
    above, in every mode, mask and dropout setting."""
    _cross_family(favit, monkeypatch, mode, D, H, family, "only", "module key bias")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("family,D,H", [("mhca", 72, 6), ("ca", 40, 1)])
def test_cross_attention_module_with_a_dead_mask_row(K, favit, monkeypatch, family, D, H, mode):
    """A query row whose mask row is all zero at an unfused width: the oracle's torch.softmax gives NaN there, so the
    reference is _dropout_ref.cross_attention_ref (P = 0 on the row; tied to the oracle by test_head_widths_host.py).
    Output and every gradient are finite and match; the row's output is out_proj.bias."""
    _ENTERED["module dead row"] += 1
    calls = _spy_softmax(favit, monkeypatch)
    M = favit.models.attention
    m = _build(favit, D + H, (lambda _: M.CrossAttention(D)) if family == "ca" else (lambda _: M.MultiHeadCrossAttention(D, H)))
    q, kv, mask = _cross_inputs(D, 5, 40, 3)
    mask[1, 2] = 0
    _module_check(favit, mode, m, lambda sd, a, b: R.cross_attention_ref(a, b, sd, H, mask), [q, kv], {"attention_mask": mask},
                  f"{family}({D}, {H}) dead row {mode}", True, calls, vanishing="skip")     # (k_proj.bias: the test above)
    with torch.no_grad():
        y = m(q, kv, attention_mask=mask)
    assert _finite(y, *[prm.grad for prm in m.parameters()])
    e = rel_l2(y[1, 2], m.out_proj.bias.detach())
    assert e < MODE_TOL[mode][0], f"the dead row's output is out_proj.bias: {e:.3e}"
    _RAN["module dead row"] += 1


FD_FAMILIES = {
    "mha": (lambda M: M.vit.MultiHeadAttention(96, 4, dropout=0.1), 1),
    "vit_block": (lambda M: M.vit.TransformerBlock(96, 4, attn_dropout=0.1), 1),
    "vm_block": (lambda M: M.vit_mhla.TransformerBlock(96, 4, attn_dropout=0.1, use_mhla=False), 1),
    "ca": (lambda M: M.attention.CrossAttention(72, dropout=0.1), 2),
    "mhca": (lambda M: M.attention.MultiHeadCrossAttention(96, 4, dropout=0.1), 2),
    "mhca_block": (lambda M: M.attention.CrossAttentionTransformerBlock(96, 4, attn_dropout=0.1, use_multi_head=True), 2),
}


@pytest.mark.parametrize("family", sorted(FD_FAMILIES))
def test_train_mode_attention_dropout_gradients_match_finite_differences(K, favit, monkeypatch, family):
    """The method of test_train_mode_dropout_gradients_match_finite_differences at an unfused width: the dropout seeds
    come from torch's CPU generator, so under a fixed torch.manual_seed the dropped module is a deterministic function
    of its parameters and inputs, and the analytic gradient along random directions (parameters and inputs) must match
    central differences.  fp32 mode.  The loss is sum(y * w) / (B * Lq): the directional derivatives are O(1) to O(10),
    the fp32 evaluation noise of the loss (~1e-6) over 2 eps = 2e-3 is below 1e-3, and the modules are smooth at this
    step (also at 20 eps on the inputs, which are O(1))."""
    _ENTERED["finite differences"] += 1
    make, n_in = FD_FAMILIES[family]
    calls = _spy_softmax(favit, monkeypatch)
    m = _build(favit, 31 + n_in, make).train()
    D = 72 if family == "ca" else 96
    g = _gen(9)
    ins = [torch.randn(MB, L, D, generator=g, device=DEV).requires_grad_(True) for L in ((17,) if n_in == 1 else (9, 21))]
    w = torch.randn(ins[0].shape, generator=g, device=DEV).double()

    def loss():
        torch.manual_seed(1234)                      # same dropout seeds on every evaluation
        return (m(*ins).double() * w).sum() / (MB * ins[0].shape[1])

    l0 = loss()
    assert calls["n"] == 1, "the unfused branch"
    l0.backward()
    assert float(loss().detach()) == float(l0.detach()), "a fixed torch seed must give the same masks"
    m.eval()
    assert float(loss().detach()) != float(l0.detach()), "train mode must drop something"
    m.train()
    leaves = list(m.parameters()) + ins
    grads = [t.grad.detach().clone().double() for t in leaves]
    gen = _gen(5)
    eps = 1e-3
    for trial in range(4):
        dirs = [torch.randn(t.shape, device=DEV, generator=gen) for t in leaves]
        if trial == 3:       # the inputs alone, 20 x as far: their share of the derivative is otherwise lost in the 2e-3
            dirs = [20 * d if i >= len(leaves) - n_in else torch.zeros_like(d) for i, d in enumerate(dirs)]
        analytic = sum(float((gr * d.double()).sum()) for gr, d in zip(grads, dirs))
        with torch.no_grad():
            for t, d in zip(leaves, dirs): t.add_(d, alpha=eps)
            lp = float(loss())
            for t, d in zip(leaves, dirs): t.add_(d, alpha=-2 * eps)
            lm = float(loss())
            for t, d in zip(leaves, dirs): t.add_(d, alpha=eps)
        numeric = (lp - lm) / (2 * eps)
        print(f"{family} trial {trial}: analytic {analytic:.6f} numeric {numeric:.6f}")
        assert abs(numeric - analytic) <= 5e-3 * max(abs(analytic), abs(numeric)) + 2e-3, (trial, numeric, analytic)
    _RAN["finite differences"] += 1


@pytest.mark.parametrize("D,H", [(96, 4), (256, 2)])
def test_mhla_module_refuses_head_widths_without_a_fold(K, favit, D, H):
    """MultiHeadLatentAttention at hd 24 and hd 128: the latent_proj fold is instantiated for hd 16, 32 and 64 only.  A
    RuntimeError that names the call and the code, before anything is launched that could leave a HIP error behind."""
    _ENTERED["refusal"] += 1
    m = _build(favit, D, lambda M: M.mhla.MultiHeadLatentAttention(D, H, window_size=7))
    x = torch.randn(2, 17, D, device=DEV)
    for mode in ("fp32", "bf16"):
        favit.set_compute_dtype(mode)
        for train in (False, True):
            m.train(train)
            with pytest.raises(RuntimeError, match=r"favit_mhla_\w+ failed: .*\(code -\d+\)"):
                m(x)
            torch.cuda.synchronize()
    y = torch.ones(4, device=DEV) * 2                # the device still computes
    assert float(y.sum()) == 8.0
    _RAN["refusal"] += 1
