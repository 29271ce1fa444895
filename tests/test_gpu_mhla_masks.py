"""GPU tests of the MHLA core's mask argument: dead rows, padding masks, structured masks, kept bytes other than 1.

Every older test builds a random 60 % mask with the diagonal kept, so no query row ever had all of its W window slots
masked.  A padding mask (mask[b, :, j] = j < n_b) produces such rows by the dozen: rows n_b + h <= i <= L - 1 - h of
image b.  The contract (include/favit.h, at favit_mhla_attn_fwd) is that of the dense kernels: such a row has o = 0 and
lse = -inf, gets dq = 0, adds nothing to dk or dv, leaves every other row alone, and nothing non-finite is written.

Masks are the five families of _dropout_ref.mask_family ("rows" stores its kept entries as 1, 2 or 255); the reference
is _dropout_ref.mhla_ref in float64 with the explicit dropout mask (P = 0 on a dead row), from the dtype-rounded
inputs.  B = 2, H = 2, p in {0, 0.25}.  Shapes are the smallest that reach each kernel's branches:
  fp32 generic forward + backward (dispatch_dpl<float, 7 / 15>)      (5, 7, 16), (17, 5, 32), (40, 15, 16)
  bf16 generic (hd 16)                                               (40, 7, 16)
  bf16 MFMA forward + the default two-owner-pass backward            (12, 7, 64), (40, 3, 32), (33, 9, 128), (70, 7, 64), (40, 11, 64)
  MFMA forward + 8-lanes-per-row backward (FAVIT_MHLA_BWD_TABLES),
  VALU forward + backward (FAVIT_MHLA_VALU)                          (70, 7, 64), (33, 9, 128)
  saved-statistics pair, FAVIT_MHLA_LSE_WAVES unset, 1 and 4         L = 8, 17, 49, 70 at W = 7, (40, 11); hd 64
Nothing reports which MHLA kernel ran, so a selection is pinned as the sibling files pin it: by the switches, by
mhla_attn_lse_supported (asserted, not skipped on), and by the case counters checked at teardown.

Gates are those the same kernels already have (tests/test_gpu_dropout_masks.py): rel-L2 of out 2e-5 / 1e-2, of the
gradients 5e-5 / 1.5e-2, lse 2e-3 absolute on live rows, per row 2.9e-6 / 6e-2.  Rows of out and dv are measured
against |ref row| + 1e-3 |ref| / sqrt(rows) as there.  Rows of dq and dk are measured against the gross-term rows of
_dropout_ref.mhla_grad_scale instead: a row with one or two surviving keys cancels (one key: dq = dk = 0 identically),
and against |ref row| even the float64 reference's own formulation run in float32 misses the fp32 gate on these masks,
while against the gross terms it stays below it on every family (tests/test_dropout_ref_host.py measures and prints
both).  A part that is zero in the reference as a whole (identity: dq, dk) is measured against the gross terms in the
rel-L2 too (the _vanishes rule of the sibling file).

identity (p = 0): P is exactly 1 on one slot, so out is bit-equal to the v block and dv to dout on the interior rows
h <= i <= L - 1 - h.  The 2h edge rows have pad copies in their windows; they are held to one unit in the last place of
the storage dtype per element (two values of the storage dtype cannot differ by less).

The refusals of a mask of the wrong shape or type have NO test here: on code without the host check such a call reads
out of bounds on the device (tests/test_mask_shapes_host.py exercises them with CPU tensors).

Before the guards in csrc/mhla.hip, 214 of the 280 core cases failed on an MI355X, all with "a non-finite value": every
case whose mask has a dead row (the 66 others are identity, and padding / ends at shapes too short for a dead row):
  fp32 generic, 20 of 30:            "fp32 L=5 W=7 hd=16 p=0.0 rows: a non-finite value"       (row_softmax: exp(-inf + inf))
  bf16 generic, 8 of 10:             "bf16 generic L=40 W=7 hd=16 p=0.0 rows: a non-finite value"
  MFMA forward + default, 40 of 50:  "default L=12 W=7 hd=64 p=0.0 rows: a non-finite value"   (0 * (1 / 0) in both kernels)
  the two switches, 32 of 40:        "tables switch L=70 W=7 hd=64 p=0.0 rows: a non-finite value"
  saved-statistics pair, 114 of 150: "lse waves=0 L=8 W=7 hd=64 p=0.0 rows: a non-finite value" (the forward's NaN row; the
                                     backward needed no change once the forward writes o = 0 and lse = -inf)."""
import math

import pytest
import torch

import _dropout_ref as R
from conftest import rel_l2
from oracle import favit_oracle as O
from test_gpu_dropout_masks import ROW_GATE, _WORST, _close, _gen, _name, _note, _rand, _rows, _tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
B, H, SEED = 2, 2, 0x1234567800000005
PS = [0.0, 0.25]
MODE_TOL = {"fp32": (1e-4, 5e-4), "fp32x3": (1e-4, 5e-4), "bf16": (2e-2, 4e-2)}      # tests/test_gpu_head_widths.py

F32_SHAPES = [(5, 7, 16), (17, 5, 32), (40, 15, 16)]
MFMA_SHAPES = [(12, 7, 64), (40, 3, 32), (33, 9, 128), (70, 7, 64), (40, 11, 64)]
SWITCH_SHAPES = [(70, 7, 64), (33, 9, 128)]
LSE_SHAPES = [(8, 7), (17, 7), (49, 7), (70, 7), (40, 11)]

# cases that ran to the end / were entered, per kernel path; a whole-module run must have run every one of them
_RAN = {"fp32": 0, "bf16 generic": 0, "mfma default": 0, "tables switch": 0, "valu": 0, "lse": 0, "module": 0}
_ENTERED = dict(_RAN)
_NEED = {"fp32": 30, "bf16 generic": 10, "mfma default": 50, "tables switch": 20, "valu": 20, "lse": 150, "module": 24}


@pytest.fixture(scope="module")
def K(favit, request):
    favit.functional.set_dropout_epoch(None)        # seeds as given: the restatement knows no epoch word
    yield favit.kernels
    for (group, gate), e in sorted(_WORST.items()):
        if group.startswith("mhla masks"):
            print(f"\n[mhla masks] {group}: worst {e:.3e} (gate {gate:g})", end="")
    print(f"\n[mhla masks] cases run: {_RAN}")
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


_CACHE = {}


def _case(dtype, L, W, hd, family, p):
    """Inputs of one shape (shared by every family, p and kernel), the family's mask, and the float64 reference with
    the explicit dropout mask; computed once and never written to."""
    D = H * hd
    ikey = (dtype, L, W, hd)
    if ikey not in _CACHE:
        g = _gen(L * 31 + W * 7 + hd)
        _CACHE[ikey] = (_rand((B * L, 3 * D), dtype, g), _rand((B * L, D), dtype, g))
    qkv, dout = _CACHE[ikey]
    mkey = (L, W, family)
    if mkey not in _CACHE:
        g = torch.Generator().manual_seed(L * 131 + W)
        mb = R.mask_family(family, B, L, W, g)
        _CACHE[mkey] = (R.mask_to_u8(family, mb, g).to(DEV), R.mhla_dead_rows(mb, L, W).to(DEV))
    mask, dead = _CACHE[mkey]
    key = ikey + (family, p)
    if key not in _CACHE:
        keep = R.mhla_keep(SEED, B, H, L, W, p, DEV) if p > 0 else None
        _CACHE[key] = R.mhla_ref(qkv.double(), dout.double(), B, L, H, hd, W, mask, keep, p) + \
            (R.mhla_grad_scale(qkv.double(), dout.double(), B, L, H, hd, W, mask, keep, p),)
    return qkv, dout, mask, dead, _CACHE[key]


def _gross_rows(group, got, ref, gross, rows, gate, what):
    """Worst per-row error of dq / dk against the gross-term rows (module docstring)."""
    err = R.row_error(got, ref, gross, rows)
    e = err.max().item()
    _note(group, gate, e)
    print(f"{group} {what}: worst row {e:.3e} at row {int(err.argmax())} (gate {gate:g}, gross denominator)")
    assert math.isfinite(e) and e < gate, f"{group} {what}: per-row error {e:.3e} at row {int(err.argmax())} >= {gate:g}"


def _check(K, dtype, L, W, hd, family, p, lse_pair, tag):
    D = H * hd
    qkv, dout, mask, dead, (o_ref, g_ref, lse_ref, gross) = _case(dtype, L, W, hd, family, p)
    n_dead = int(dead.sum())
    assert n_dead == R.mask_family_dead_count(family, B, L, W), "the family lost its dead rows"
    if lse_pair:
        out, lse = K.mhla_attn_fwd(qkv, B, L, H, hd, W, mask, p, SEED, want_lse=True)
        assert lse is not None
        dqkv = K.mhla_attn_bwd(qkv, dout, B, L, H, hd, W, mask, p, SEED, o=out, lse=lse)
    else:
        out = K.mhla_attn_fwd(qkv, B, L, H, hd, W, mask, p, SEED)
        dqkv = K.mhla_attn_bwd(qkv, dout, B, L, H, hd, W, mask, p, SEED)
    what = f"{tag} L={L} W={W} hd={hd} p={p} {family}"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all()), what + ": a non-finite value"
    dr = dead.reshape(B * L)
    assert bool((out[dr] == 0).all()), what + ": the output row of a dead row is exactly 0"
    assert bool((dqkv[dr, :D] == 0).all()), what + ": dq of a dead row is exactly 0"
    if lse_pair:
        dh = dead[:, None].expand(B, H, L)
        assert bool((lse[dh] == float("-inf")).all()), what + ": lse of a dead row is -inf"
        assert bool(torch.isfinite(lse[~dh]).all()), what + ": lse of a live row is finite"
        assert torch.equal(torch.isfinite(lse_ref), ~dh)
        if n_dead < B * L:
            e = (lse[~dh].double() - lse_ref[~dh]).abs().max().item()      # the lse of the UNDROPPED scores
            _note("mhla masks lse (abs)", 2e-3, e)
            assert e < 2e-3, f"{what}: lse differs by {e:.3e}"
    grp = f"mhla masks {_name(dtype)}"
    rgrp = grp + " rows"
    gate = ROW_GATE[("mhla", dtype)]
    _close(grp + " out", out.float(), o_ref, _tol(dtype), what)
    _rows(rgrp, out.float(), o_ref, B * L, gate, what + " out")
    gtol = 5e-5 if dtype == F32 else 1.5e-2
    for part, nm in enumerate(("dq", "dk", "dv")):
        sl = slice(part * D, (part + 1) * D)
        a, b = dqkv[:, sl].float(), g_ref[:, sl]
        _close(grp + " " + nm, a, b, gtol, what, gross[:, sl] if part < 2 else None)
        if part < 2:
            _gross_rows(rgrp + " (gross)", a, b, gross[:, sl], B * L, gate, what + " " + nm)
        else:
            _rows(rgrp, a, b, B * L, gate, what + " " + nm)
    _close(grp + " dqkv", dqkv.float(), g_ref, gtol, what)
    if family == "identity" and p == 0:
        h = W // 2
        i = torch.arange(L, device=DEV)
        inner = ((i >= h) & (i <= L - 1 - h)).repeat(B)
        v = qkv[:, 2 * D:]
        assert torch.equal(out[inner], v[inner]), what + ": out is the v block, bit for bit, on interior rows"
        assert torch.equal(dqkv[inner, 2 * D:], dout[inner]), what + ": dv is dout, bit for bit, on interior rows"
        ulp = torch.finfo(dtype).eps
        for got, want, nm in ((out, v, "out"), (dqkv[:, 2 * D:], dout, "dv")):
            d = (got[~inner].double() - want[~inner].double()).abs()
            assert bool((d <= ulp * want[~inner].double().abs()).all()), f"{what}: {nm} of an edge row is off by more than one ulp"


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("family", R.MASK_FAMILIES)
@pytest.mark.parametrize("L,W,hd", F32_SHAPES)
def test_fp32_kernels(K, L, W, hd, family, p):
    _ENTERED["fp32"] += 1
    _check(K, F32, L, W, hd, family, p, False, "fp32")
    _RAN["fp32"] += 1


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("family", R.MASK_FAMILIES)
def test_bf16_generic_kernels(K, family, p):
    """hd = 16: no MFMA kernel takes it."""
    _ENTERED["bf16 generic"] += 1
    _check(K, BF16, 40, 7, 16, family, p, False, "bf16 generic")
    _RAN["bf16 generic"] += 1


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("family", R.MASK_FAMILIES)
@pytest.mark.parametrize("L,W,hd", MFMA_SHAPES)
def test_bf16_mfma_forward_and_default_backward(K, L, W, hd, family, p, monkeypatch):
    """mhla_fwd_mfma_kernel<hd, false> and mhla_bwd_mfma2_kernel<hd, false>: one block (12), two 16-row tiles and a
    partial third (40, 33), two balanced blocks of 35 rows (70), W = 11 with L > 16."""
    for env in ("FAVIT_MHLA_VALU", "FAVIT_MHLA_BWD_TABLES", "FAVIT_MHLA_BWD_MFMA", "FAVIT_MHLA_BLOCKS"):
        monkeypatch.delenv(env, raising=False)
    _ENTERED["mfma default"] += 1
    _check(K, BF16, L, W, hd, family, p, False, "default")
    _RAN["mfma default"] += 1


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("family", R.MASK_FAMILIES)
@pytest.mark.parametrize("switch", ["tables switch", "valu"])
@pytest.mark.parametrize("L,W,hd", SWITCH_SHAPES)
def test_bf16_switched_kernels(K, L, W, hd, switch, family, p, monkeypatch):
    """FAVIT_MHLA_BWD_TABLES: MFMA forward, 8-lanes-per-row backward; FAVIT_MHLA_VALU: the generic bf16 forward and
    backward at an MFMA head size (both read per call)."""
    monkeypatch.setenv("FAVIT_MHLA_BWD_TABLES" if switch == "tables switch" else "FAVIT_MHLA_VALU", "1")
    _ENTERED[switch] += 1
    _check(K, BF16, L, W, hd, family, p, False, switch)
    _RAN[switch] += 1


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("family", R.MASK_FAMILIES)
@pytest.mark.parametrize("waves", [0, 1, 4])
@pytest.mark.parametrize("L,W", LSE_SHAPES)
def test_saved_statistics_pair(K, L, W, waves, family, p, monkeypatch):
    """The training path's pair with a mask (mhla_bwd_lse_kernel<false, N>): L = 8 is the shortest sequence it takes,
    17 and 49 put one row into a tile of its own, 49 and 70 cross the 48-row block seam of the default block size."""
    monkeypatch.delenv("FAVIT_MHLA_VALU", raising=False)
    monkeypatch.delenv("FAVIT_MHLA_NO_LSE", raising=False)
    _ENTERED["lse"] += 1
    assert K.mhla_attn_lse_supported(L, 64, W, BF16), "every shape of this grid is taken by the saved-statistics kernels"
    if waves:
        monkeypatch.setenv("FAVIT_MHLA_LSE_WAVES", str(waves))
    else:
        monkeypatch.delenv("FAVIT_MHLA_LSE_WAVES", raising=False)
    _check(K, BF16, L, W, 64, family, p, True, f"lse waves={waves}")
    _RAN["lse"] += 1


# --------------------------------------------------------------------------------------
# Modules
# --------------------------------------------------------------------------------------
MD, MH_, MW, ML = 128, 2, 7, 40


def _build(favit, seed, make):
    """torch's default initialisation under a fixed seed; every vector (biases, LayerNorm) perturbed off its 0 / 1 default."""
    torch.manual_seed(seed)
    m = make(favit.models)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for prm in m.parameters():
            if prm.dim() == 1:
                prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    return m.to(DEV)


def _block_ref(sd, x, mask):
    """oracle.favit_oracle.vit_mhla_block (use_mhla) around mhla_attention_ref."""
    x = x + R.mhla_attention_ref(O.layer_norm(x, sd["norm1.weight"], sd["norm1.bias"]), sd, "attn.", MH_, MW, mask)
    return x + O.mlp(O.layer_norm(x, sd["norm2.weight"], sd["norm2.bias"]), sd, "mlp.")


@pytest.mark.parametrize("mode", ["fp32", "fp32x3", "bf16"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("family", ["padding", "rows"])
@pytest.mark.parametrize("module", ["attention", "block"])
def test_modules_with_dead_rows(K, favit, module, family, training, mode):
    """MultiHeadLatentAttention(128, 2, window 7) and vit_mhla.TransformerBlock(128, 2, use_mhla=True) at L = 40
    (hd = 64: in bf16 the training forward takes the saved-statistics pair; all dropouts are 0, so train == eval in
    value).  Output, input gradient and every parameter gradient against the float64 reference, nothing non-finite,
    and every dead row of the attention module's output is proj.bias."""
    _ENTERED["module"] += 1
    if module == "attention":
        m = _build(favit, 17, lambda M: M.mhla.MultiHeadLatentAttention(MD, MH_, MW))
        ref = lambda sd, x, mk: R.mhla_attention_ref(x, sd, "", MH_, MW, mk)
    else:
        m = _build(favit, 18, lambda M: M.vit_mhla.TransformerBlock(MD, MH_, window_size=MW, use_mhla=True))
        ref = _block_ref
    g = torch.Generator().manual_seed(ML + len(family))
    mb = R.mask_family(family, B, ML, MW, g)
    dead = R.mhla_dead_rows(mb, ML, MW).to(DEV)
    assert int(dead.sum()) == R.mask_family_dead_count(family, B, ML, MW) > 0
    mask = R.mask_to_u8(family, mb, g).to(DEV)
    x = torch.randn(B, ML, MD, generator=_gen(5), device=DEV)
    favit.set_compute_dtype(mode)
    m.train(training)
    for prm in m.parameters():
        prm.grad = None
    xs = x.clone().requires_grad_(True)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    x64 = x.double().clone().requires_grad_(True)
    y = m(xs, attention_mask=mask)
    y64 = ref(sd, x64, mask)
    gout = torch.randn(y.shape, generator=_gen(y.numel()), device=DEV)
    (y * gout).sum().backward()
    (y64 * gout.double()).sum().backward()
    what = f"{module} {family} {'train' if training else 'eval'} {mode}"
    ftol, gtol = MODE_TOL[mode]
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xs.grad).all()), what + ": a non-finite value"
    e = rel_l2(y.detach(), y64.detach())
    _note(f"mhla masks module {mode} out", ftol, e)
    assert e < ftol, f"{what}: forward {e:.3e}"
    e = rel_l2(xs.grad, x64.grad)
    _note(f"mhla masks module {mode} grads", gtol, e)
    assert e < gtol, f"{what}: input gradient {e:.3e}"
    for k, prm in m.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), f"{what}: gradient of {k}"
        e = rel_l2(prm.grad, sd[k].grad)
        _note(f"mhla masks module {mode} grads", gtol, e)
        assert e < gtol, f"{what}: grad {k}: {e:.3e}"
    if module == "attention":
        bias = m.proj.bias.detach().expand(int(dead.sum()), MD)
        e = rel_l2(y.detach()[dead], bias)
        _note(f"mhla masks module {mode} dead rows", ftol, e)
        assert e < ftol, f"{what}: a dead row's output is proj.bias: {e:.3e}"
    _RAN["module"] += 1
