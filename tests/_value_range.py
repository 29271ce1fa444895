"""Inputs far from unit scale, and float32 restatements of the references, for tests/test_value_range_host.py (CPU) and
tests/test_gpu_value_range.py (GPU).  Host only: torch on the CPU, tests/_dropout_ref.py and tests/_distill_ref.py.

Every older GPU test draws attention inputs and logits from randn at unit scale: scores stay within +-5, logits within
+-10, LayerNorm rows have a mean of a few standard deviations, GELU pre-activations stay below |x| = 4.  There a softmax
that never subtracted the row maximum, a one-pass variance E[x^2] - mu^2 and a GELU that is wrong in its tails all pass.
The recipes below take that cover away (c = sqrt(120 / sqrt(hd))):

  spread      q, k = 6 randn: scores reach +-140, P is nearly one-hot
  offset+     q, k = randn + c: every score is near +120 (exp overflows without the max), P stays soft
  offset-     q = randn + c, k = randn - c: every score is near -120 (every exp underflows: 0 / 0 without the max)
  late-max    spread with key row j times 1 + j / 16: the running maximum of a streamed softmax rises at every block
  early-max   the reverse: the maximum is final after the first block and every later rescale factor underflows
  logits      randn s + o, (s, o) in (3, 0), (30, +100), (30, -100), (100, 0)
  LayerNorm   rows of randn + 100, constant rows (0, 3, -1024: their sums are exact in fp32 in any order), 1e-20 randn
  GELU grid   every bf16 value with 2^-10 <= |x| <= 12, and +-0, +-13.5, +-30

A gate of the GPU module comes from here and never from a kernel: it is an existing gate of the suite, or a rule
(units in the last place of the operands of a subtraction), or FOUR TIMES the error of the float64 reference's own
formulation run in float32 on the same inputs.  gate_table() measures every such restatement against float64 beside the
gate it has to stay a quarter of; `python tests/_value_range.py` prints the table."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _distill_ref as DR                                   # noqa: E402
import _dropout_ref as R                                    # noqa: E402

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SEED = 0x1234567800000005                                   # the dropout seed of the sibling modules
U24 = 2.0 ** -24                                            # half a unit in the last place of an fp32 value of size 1

ATTN_RECIPES = ("spread", "offset+", "offset-")
STREAM_RECIPES = ("late-max", "early-max")
LOGIT_RECIPES = ((3.0, 0.0), (30.0, 100.0), (30.0, -100.0), (100.0, 0.0))

# The gates of the GPU module.  A gate of the suite (or a rule of the issue) is kept where the float32 restatement stays
# within a quarter of it.  Where it does not, no fp32 kernel can be held to it either -- rounding a score of size 120
# moves P by 2^-24 * 120 whatever the summation order -- and the gate is 4 x the restatement's worst error over the whole
# grid of the GPU module, rounded up to two digits.  gate_table() repeats every measurement; the host test holds each to
# a quarter of its gate.  Measured on the CPU (float32 restatement against float64), never on a kernel:
#   fp32 per-row, MHLA   worst row 2.75e-5 (dv, offset+)   -> 1.1e-4    (unit scale: 2.9e-6, tests/test_gpu_dropout_masks.py)
#   fp32 per-row, SDPA   worst row 6.70e-5 (dv, late-max)  -> 2.7e-4    (unit scale: 5.4e-6)
#   SDPA o rel-L2        1.93e-5 (offset+)                 -> 7.8e-5    (unit scale: 2e-5)
#   SDPA dq / dk / dv    2.19e-5 (dk, offset-)             -> 8.8e-5    (unit scale: 5e-5)
#   dense maps rel-L2    6.31e-6                           -> 2.6e-5    (unit scale: 2e-5)
#   MHLA out / dqkv / lse, window maps, dlogits, SDPA lse: within a quarter of the suite's gates, which are kept
# Rows of out and dv are measured against |ref row| + 1e-3 |ref| / sqrt(rows), rows of dq and dk against the gross-term
# rows of mhla_grad_scale / sdpa_grad_scale (a nearly one-hot P makes dq and dk sums of cancelling terms).
ROW_GATE_F32 = {"mhla": 1.1e-4, "sdpa": 2.7e-4}
ROW_GATE_BF16 = 6e-2                                        # tests/test_gpu_dropout_masks.py: rounding of P to bf16
MHLA_OUT_TOL = {F32: 2e-5, BF16: 1e-2}
MHLA_GRAD_TOL = {F32: 5e-5, BF16: 1.5e-2}
MHLA_LSE_ABS = 2e-3
SDPA_OUT_TOL = {F32: 7.8e-5, BF16: 1e-2}
SDPA_GRAD_TOL = {F32: 8.8e-5, BF16: 2e-2}
SDPA_LSE_TOL = {F32: 2e-5, BF16: 2e-5 + 3e-3}
MAPS_TOL = {"window": 2e-5, "dense": 2.6e-5}                # tests/test_gpu_attention_maps.py: 2e-5
MAPS_ROW_SUM, ROLLOUT_MASS = 1e-5, 1e-4
DLOGITS_TOL = 2e-5
# |loss row - ref| <= LOSS_UNITS * 2^-24 * loss_scale(row), by member of the family (loss_group).  plain: the issue's eight
# units (restatement: below 2).  A smoothed or mixed target adds the roundings of (1 - eps) x_a, lam x_a + (1 - lam) x_b
# and eps mean(x) to that of lse and of the difference, a teacher term those of two more log-softmaxes: the restatement
# reaches 3.36 and 4.32 units, so these take 4 x that.
LOSS_UNITS = {"plain": 8.0, "weighted": 13.5, "teacher": 17.3}
# LayerNorm on rows of randn + 100, rel-L2 except the mean (units of 2^-23 |mean|).  The error of the mean shifts a whole
# row of y, and an fp32 sum of D values near 100 rounds at the size of 100 D: the restatement has 1.38 units in the mean,
# 6.1e-6 in y and 6.9e-6 in dgamma (all three from that one rounding), so these three take 4 x that and not the 4 units /
# 2e-5 that hold for rstd, dx and dbeta.
LN_TOL = {"y": 2.5e-5, "mean": 5.6, "rstd": 2e-5, "dx": 2e-5, "dgamma": 2.8e-5, "dbeta": 2e-5}
LN_TOL_BF16_Y = 1e-2                                        # test_layernorm_fwd_bwd: a bf16 y


def attn_c(hd):
    return math.sqrt(120.0 / math.sqrt(hd))


# --------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------
def attn_inputs(recipe, B, Lq, Lk, D, hd, seed):
    """float32 q [B*Lq, D], k, v [B*Lk, D], dout [B*Lq, D] (column h*hd + d) of one recipe, seeded, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    q, k = torch.randn(B * Lq, D, generator=g), torch.randn(B * Lk, D, generator=g)
    v, dout = torch.randn(B * Lk, D, generator=g), torch.randn(B * Lq, D, generator=g)
    c = attn_c(hd)
    if recipe in ("spread",) + STREAM_RECIPES:
        q, k = 6.0 * q, 6.0 * k
        if recipe in STREAM_RECIPES:
            j = torch.arange(Lk, dtype=F32)
            f = 1.0 + (j if recipe == "late-max" else (Lk - 1 - j)) / 16.0
            k = k * f.repeat(B)[:, None]
    elif recipe == "offset+":
        q, k = q + c, k + c
    elif recipe == "offset-":
        q, k = q + c, k - c
    else:
        raise ValueError(recipe)
    return q, k, v, dout


def mhla_inputs(recipe, dtype, B, L, H, hd, W):
    """(qkv [B*L, 3D], dout [B*L, D]) rounded to dtype, on the CPU."""
    D = H * hd
    q, k, v, dout = attn_inputs(recipe, B, L, L, D, hd, L * 31 + W * 7 + hd + 1000 * len(recipe))
    return torch.cat((q, k, v), 1).to(dtype), dout.to(dtype)


def padding_mask(B, L, W):
    """The "padding" family of _dropout_ref.mask_family as the uint8 tensor the kernels read."""
    return R.mask_to_u8("padding", R.mask_family("padding", B, L, W, torch.Generator().manual_seed(0)), None)


def mhla_run(qkv, dout, B, L, H, hd, W, mask, keep, p, dtype):
    """_dropout_ref.mhla_ref's body at `dtype`: float64 is the reference, float32 its restatement.
    Returns (out [B*L, D], dqkv [B*L, 3D], lse [B, H, L])."""
    D = H * hd
    t = qkv.to(dtype).reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).detach().clone().requires_grad_(True)
    o, lse = R.mhla_core(t[0], t[1], t[2], W, mask, keep, p)
    out = o.transpose(1, 2).reshape(B * L, D)
    out.backward(dout.to(dtype))
    return out.detach(), t.grad.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * D), lse


def mhla_scores(qkv, B, L, H, hd, W, mask=None, dtype=F64):
    """Window scores [B, H, L, W] at `dtype` (masked slots -inf), as mhla_core forms them."""
    from oracle import favit_oracle as O
    t = qkv.to(dtype).reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    idx = torch.from_numpy(O.window_indices(L, W))
    s = (t[0].unsqueeze(3) @ t[1][:, :, idx].transpose(-2, -1)).squeeze(3) / (hd ** 0.5)
    if mask is not None:
        wm = torch.gather(mask[:, None].expand(B, H, L, L), 3, idx[None, None].expand(B, H, L, W)) != 0
        s = s.masked_fill(~wm, float("-inf"))
    return s


def heads(t, B, L, H, hd):
    """[B*L, H*hd] -> [B, H, L, hd]"""
    return t.reshape(B, L, H, hd).permute(0, 2, 1, 3)


def merged(t, B, L, H, hd):
    """[B, H, L, hd] -> [B*L, H*hd], the layout the library writes."""
    return t.permute(0, 2, 1, 3).reshape(B * L, H * hd)


def sdpa_inputs(recipe, dtype, B, H, Lq, Lk, hd):
    """(q, k, v, dout) as [rows, D] tensors rounded to dtype, on the CPU."""
    q, k, v, dout = attn_inputs(recipe, B, Lq, Lk, H * hd, hd, B * 1000 + Lq * 10 + hd + Lk + 7919 * len(recipe))
    return tuple(t.to(dtype) for t in (q, k, v, dout))


def key_mask(B, Lk):
    """bool [B, Lk], the "keys" mask of tests/test_gpu_dropout_masks.py: 70 % kept, key 0 always."""
    mk = torch.rand(B, Lk, generator=torch.Generator().manual_seed(B * 100 + Lk)) > 0.3
    mk[:, 0] = True
    return mk


def sdpa_run(q, k, v, dout, B, H, Lq, Lk, hd, mk, keep, p, dtype):
    """_dropout_ref.sdpa_ref's body at `dtype` on [rows, D] inputs.  Returns (o, lse, dq, dk, dv), heads split."""
    qr, kr, vr = (heads(t.to(dtype), B, L, H, hd).detach().clone().requires_grad_(True) for t, L in ((q, Lq), (k, Lk), (v, Lk)))
    s, P = R._sdpa_probs(qr, kr, 1.0 / math.sqrt(hd), None if mk is None else mk[:, None, None, :])
    if keep is not None:
        P = P * keep.to(P.dtype) / (1.0 - p)
    o = P @ vr
    o.backward(heads(dout.to(dtype), B, Lq, H, hd))
    return o.detach(), torch.logsumexp(s.detach(), -1), qr.grad, kr.grad, vr.grad


def _bf16(t):
    return t.to(BF16).to(F64)


def sdpa_bf16_restatement(q, k, v, dout, B, H, Lq, Lk, hd, mk):
    """The fused dense attention in float64 with the roundings of its bf16 kernels (csrc/sdpa.hip) and no others:
    exp(s - max) is rounded to bf16 for the P V product while its row sum is not, o is stored in bf16 and delta =
    rowsum(dO * o) reads that; dS * scale and P are rounded to bf16 for the three gradient products; dq, dk and dv are
    stored in bf16.  Returns (o, dq, dk, dv), heads split."""
    qh, kh, vh, gh = (heads(t.double(), B, L, H, hd) for t, L in ((q, Lq), (k, Lk), (v, Lk), (dout, Lq)))
    scale = 1.0 / math.sqrt(hd)
    s = (qh @ kh.transpose(-2, -1)) * scale
    if mk is not None:
        s = s.masked_fill(~mk[:, None, None, :], float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    o = _bf16((_bf16(e) @ vh) / l)
    P = e / l
    dS = _bf16(P * (gh @ vh.transpose(-2, -1) - (gh * o).sum(-1, keepdim=True)) * scale)
    return o, _bf16(dS @ kh), _bf16(dS.transpose(-2, -1) @ qh), _bf16(_bf16(P).transpose(-2, -1) @ gh)


def sdpa_bf16_gates(q, k, v, dout, B, H, Lq, Lk, hd, mk, ref):
    """rel-L2 gates (o, dq, dk, dv) of one bf16 case: the suite's 1e-2 / 2e-2, but where sdpa_bf16_restatement itself
    misses that against the float64 reference `ref` (sdpa_run), and no kernel with these roundings can meet it: there
    the gate is twice the restatement's error.  That is dq on the offset recipes at hd = 16 and nowhere else: k carries
    the common component c = 5.5, dq = sum_j dS_ij k_j relies on sum_j dS_ij = 0 to cancel it, and the bf16-rounded
    dS do not sum to 0.  The restatement's dq is off by 6.0e-2 / 5.5e-2 there (2.3e-2 with the key mask).
    Returns (gates, the restatement's errors)."""
    r = sdpa_bf16_restatement(q, k, v, dout, B, H, Lq, Lk, hd, mk)
    errs = [_rel(a, b) for a, b in zip(r, (ref[0], ref[2], ref[3], ref[4]))]
    base = (SDPA_OUT_TOL[BF16],) + (SDPA_GRAD_TOL[BF16],) * 3
    return tuple(2.0 * e if e > b else b for b, e in zip(base, errs)), errs


def naive_softmax32(s):
    """exp(s) / sum exp(s) in float32: what a kernel without the row maximum computes."""
    e = torch.exp(s.to(F32))
    return e / e.sum(-1, keepdim=True)


# The grids of the GPU module.  B = 2, H = 2 for MHLA.
MHLA_B, MHLA_H = 2, 2
F32_SHAPES = [(5, 7, 16), (17, 5, 32), (40, 15, 16)]
BF16_GENERIC = [(40, 7, 16)]
MFMA_SHAPES = [(12, 7, 64), (40, 3, 32), (33, 9, 128), (70, 7, 64), (40, 11, 64)]
SWITCH_SHAPES = [(70, 7, 64), (33, 9, 128)]
LSE_SHAPES = [(8, 7, 64), (17, 7, 64), (49, 7, 64), (70, 7, 64), (40, 11, 64)]
MHLA_PATHS = {"fp32": (F32, F32_SHAPES), "bf16 generic": (BF16, BF16_GENERIC), "mfma default": (BF16, MFMA_SHAPES),
              "tables switch": (BF16, SWITCH_SHAPES), "valu": (BF16, SWITCH_SHAPES), "lse": (BF16, LSE_SHAPES)}
DROP_P = 0.25


def mhla_grid():
    """(path, L, W, hd, recipe, masked, p, waves) of every MHLA core case: three recipes x {no mask, padding} per shape,
    the saved-statistics pair also at 1 and 4 tiles per block on offset+, and one dropout case per path."""
    out = []
    for path, (_, shapes) in MHLA_PATHS.items():
        for L, W, hd in shapes:
            for recipe in ATTN_RECIPES:
                for masked in (False, True):
                    for waves in ((0, 1, 4) if path == "lse" and recipe == "offset+" else (0,)):
                        out.append((path, L, W, hd, recipe, masked, 0.0, waves))
        L, W, hd = shapes[-1]
        out.append((path, L, W, hd, "offset+", False, DROP_P, 0))
    return out


MHLA_NEED = {"fp32": 19, "bf16 generic": 7, "mfma default": 31, "tables switch": 13, "valu": 13, "lse": 51}   # len by path
SDPA_NEED = 64

SDPA_SHAPES = [(2, 3, 65, 65, 64), (2, 2, 17, 17, 16), (1, 3, 70, 100, 48), (1, 1, 130, 64, 192)]
STREAM_SHAPE = (1, 3, 70, 100, 48)


def sdpa_grid():
    """(dtype, B, H, Lq, Lk, hd, recipe, mask kind, waves)"""
    out = []
    for dtype in (F32, BF16):
        for shape in SDPA_SHAPES:
            for recipe in ATTN_RECIPES:
                for mk in (None, "keys"):
                    out.append((dtype,) + shape + (recipe, mk, 0))
        for recipe in STREAM_RECIPES:
            for mk in (None, "keys"):
                for waves in ((0, 4, 5) if recipe == "late-max" else (0,)):
                    out.append((dtype,) + STREAM_SHAPE + (recipe, mk, waves))
    return out


def dtype_name(dtype):
    return "fp32" if dtype == F32 else "bf16"


# --------------------------------------------------------------------------------------
# logits
# --------------------------------------------------------------------------------------
CE_B = 9
CE_CLASSES = (1, 2, 63, 64, 65, 1000, 21843)
CE_KINDS = ("ce", "ls", "mix", "soft1", "soft4", "hard")     # kernel, with: eps 0.1 | eps 0.1 + lam | tau 1 | tau 4 | hard


def logits_case(s, o, Cn, B=CE_B):
    """(logits, teacher, labels, lam) on the CPU: logits = randn s + o, the teacher the same recipe with another seed."""
    g = torch.Generator().manual_seed(int(s) * 100003 + int(o) * 101 + Cn)
    logits = torch.randn(B, Cn, generator=g) * s + o
    labels = torch.randint(0, Cn, (B,), generator=g)
    lam = torch.tensor([(0.0, 0.3, 1.0, 0.75)[b % 4] for b in range(B)])
    g2 = torch.Generator().manual_seed(int(s) * 7919 + int(o) * 13 + Cn + 1)
    teacher = torch.randn(B, Cn, generator=g2) * s + o
    return logits, teacher, labels, lam


def ce_args(kind):
    """(eps, mixed, alpha, tau, distill kind or None) of one member of the family."""
    return {"ce": (0.0, False, 0.0, 1.0, None), "ls": (0.1, False, 0.0, 1.0, None), "mix": (0.1, True, 0.0, 1.0, None),
            "soft1": (0.0, False, 0.5, 1.0, "soft"), "soft4": (0.1, True, 0.5, 4.0, "soft"),
            "hard": (0.0, False, 0.5, 1.0, "hard")}[kind]


def loss_group(kind):
    """plain: one-hot target (also favit_eval_metrics); weighted: label smoothing / mixed targets; teacher: distilled."""
    return {"ce": "plain", "ls": "weighted", "mix": "weighted"}.get(kind, "teacher")


def ce_reference(logits, teacher, labels, lam, kind):
    """float64 (tests/_distill_ref.py; alpha = 0 is the loss without a teacher): dict with loss_rows, kd_rows, grad (of
    the mean), and the per-row scales of loss_scale()."""
    eps, mixed, alpha, tau, dk = ce_args(kind)
    lam = lam if mixed else None
    ref = DR.reference(logits, teacher, labels, lam, eps, alpha, tau, dk or "soft")
    base_s, kd_s = loss_scale(logits, teacher, labels, lam, eps, tau, dk)
    ref["kd_scale"] = kd_s
    ref["loss_scale"] = (1.0 - alpha) * base_s + alpha * kd_s if dk else base_s
    return ref


def loss_scale(logits, teacher, labels, lam, eps, tau, dk):
    """The size of the operands whose difference a loss row is, float64 [B] each (base, kd); never below 1.

    base = lse(x) - sum_j t_j x_j: max(|lse(x)|, sum_j t_j |x_j|).  With a one-hot target that is max(|lse|, |x_label|).
    |lse| alone does not bound the rounding of the row: at logits = 30 randn - 100 the row maximum can sit near 0 while
    x_label is near -200, and then the correctly rounded fp32 value of the loss itself is off by up to 2^-24 * 200.
    soft kd = tau^2 (sum_j q_j (z_j - x_j) / tau - lse(z / tau) + lse(x / tau)): tau^2 times the largest of the two lse
    and the two q-weighted sums.  hard kd = lse(x) - x[argmax z]."""
    x, z = logits.double(), teacher.double()
    t = DR.targets(labels, lam, eps, x.shape[1])
    one = torch.ones(x.shape[0], dtype=F64)
    base = torch.stack((one, torch.logsumexp(x, 1).abs(), (t * x.abs()).sum(1))).max(0).values
    if dk == "soft":
        q = torch.softmax(z / tau, 1)
        terms = (torch.logsumexp(x / tau, 1).abs(), torch.logsumexp(z / tau, 1).abs(), (q * x.abs()).sum(1) / tau,
                 (q * z.abs()).sum(1) / tau)
        kd = torch.stack((one,) + tuple(tau * tau * v for v in terms)).max(0).values
    elif dk == "hard":
        xa = x.gather(1, DR.lowest_argmax(z)[:, None])[:, 0]
        kd = torch.stack((one, torch.logsumexp(x, 1).abs(), xa.abs())).max(0).values
    else:
        kd = one
    return base, kd


def ce_f32(logits, teacher, labels, lam, kind):
    """The family in float32 with the row maximum subtracted by hand.  base = lse(x) - (1 - eps) (lam x_a + (1 - lam) x_b)
    - eps mean(x), the difference loss_scale() describes; the teacher term element by element from the two
    log-softmaxes, (u - max) - log sum exp(u - max).  Returns (loss_rows, kd_rows, dlogits of the mean)."""
    eps, mixed, alpha, tau, dk = ce_args(kind)
    x, z = logits.to(F32), teacher.to(F32)
    hot = DR.targets(labels, lam if mixed else None, 0.0, x.shape[1]).to(F32)

    def lsm(u):
        m = u.max(1, keepdim=True).values
        return m, (u - m) - torch.log(torch.exp(u - m).sum(1, keepdim=True))

    m, lp = lsm(x)
    lx = (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))[:, 0]
    base = lx - (1 - eps) * (hot * x).sum(1)
    if eps:
        base = base - eps * x.mean(1)
    sm = torch.exp(lp)
    grad = sm - ((1 - eps) * hot + eps / x.shape[1])
    kd = torch.zeros_like(base)
    if dk == "soft":
        (_, lq), (_, lpt) = lsm(z / tau), lsm(x / tau)
        kd = tau * tau * (torch.exp(lq) * (lq - lpt)).sum(1)
        grad = (1 - alpha) * grad + alpha * tau * (torch.exp(lpt) - torch.exp(lq))
    elif dk == "hard":
        am = DR.lowest_argmax(z)
        kd = lx - x.gather(1, am[:, None])[:, 0]
        grad = (1 - alpha) * grad + alpha * (sm - torch.nn.functional.one_hot(am, x.shape[1]).to(F32))
    return (1 - alpha) * base + alpha * kd, kd, grad / x.shape[0]


def naive_lse32(x):
    return torch.log(torch.exp(x.to(F32)).sum(1))


# --------------------------------------------------------------------------------------
# LayerNorm
# --------------------------------------------------------------------------------------
LN_ROWS = 37
LN_DIMS = (64, 384, 512, 768, 2048)
LN_KINDS = ("+100", "const", "tiny")
LN_EPS = 1e-5
LN_CONSTANTS = (0.0, 3.0, -1024.0)


def ln_case(kind, rows, D):
    """(x [rows, D], gamma, beta, dy) in float32 on the CPU.  const: row r holds LN_CONSTANTS[r % 3]."""
    g = torch.Generator().manual_seed(rows * 131 + D + len(kind))
    x = torch.randn(rows, D, generator=g)
    if kind == "+100":
        x = x + 100.0
    elif kind == "const":
        x = torch.tensor(LN_CONSTANTS)[torch.arange(rows) % 3][:, None].expand(rows, D).contiguous()
    elif kind == "tiny":
        x = 1e-20 * x
    else:
        raise ValueError(kind)
    return x, 1 + 0.2 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g), torch.randn(rows, D, generator=g)


def ln_run(x, gamma, beta, dy, dtype, one_pass=False):
    """LayerNorm written out at `dtype` (two-pass variance, or E[x^2] - mu^2 with one_pass): y, mean, rstd, dx, dgamma,
    dbeta, the gradients by autograd through the same expressions."""
    x = x.to(dtype).detach().clone().requires_grad_(True)
    gamma, beta = (t.to(dtype).detach().clone().requires_grad_(True) for t in (gamma, beta))
    mu = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mu * mu if one_pass else ((x - mu) ** 2).mean(-1, keepdim=True)
    rs = (var + LN_EPS).rsqrt()
    y = (x - mu) * rs * gamma + beta
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), dy.to(dtype))
    return y.detach(), mu.detach()[:, 0], rs.detach()[:, 0], dx, dg, db


# --------------------------------------------------------------------------------------
# GELU
# --------------------------------------------------------------------------------------
def gelu_values():
    """The grid as a float32 vector: every bf16 value with 2^-10 <= |x| <= 12, then +-0, +-13.5, +-30."""
    pos = torch.arange(0, 0x7F80, dtype=torch.int32).to(torch.int16).view(BF16).float()
    pos = pos[(pos >= 2.0 ** -10) & (pos <= 12.0)]
    return torch.cat((pos, -pos, torch.tensor([0.0, -0.0, 13.5, -13.5, 30.0, -30.0])))


def gelu_grid(M, N=64):
    """[M, N] float32: the grid values laid out row after row, repeated to fill (M * N >= the grid's length)."""
    v = gelu_values()
    assert M * N >= v.numel()
    return v[torch.arange(M * N) % v.numel()].reshape(M, N)


def gelu_ref(x):
    """float64 (GELU, GELU') by erfc, which keeps the negative tail that 1 + erf loses."""
    x = x.double()
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_fast_f32(x):
    """gelu_terms_fast of csrc/common.h (Abramowitz-Stegun 7.1.26) restated in torch float32: (GELU, GELU')."""
    x = x.to(F32)
    ax = x.abs()
    e = torch.exp(-0.5 * x * x)
    t = 1.0 / (torch.tensor(0.3275911 * 0.70710678118654752440, dtype=F32) * ax + 1.0)
    poly = torch.tensor(1.061405429, dtype=F32) * t + torch.tensor(-1.453152027, dtype=F32)
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = poly * t + torch.tensor(c, dtype=F32)
    erfa = 1.0 - poly * t * e
    cdf = 0.5 * (1.0 + torch.copysign(erfa, x))
    pdf = torch.tensor(0.39894228040143267794, dtype=F32) * e
    return x * cdf, x * pdf + cdf


def gelu_erf_f32(x):
    """gelu_f / dgelu_f of csrc/common.h in torch float32: 0.5 x (1 + erf(x / sqrt 2)) and its derivative."""
    x = x.to(F32)
    cdf = 0.5 * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752440, dtype=F32)))
    pdf = torch.tensor(0.39894228040143267794, dtype=F32) * torch.exp(-0.5 * x * x)
    return x * cdf, cdf + x * pdf


def gelu_gate_bf16(x, ref):
    """Per element, bf16 in / bf16 out: half a bf16 unit of the result twice over, and 1e-6 max(1, |x|) for the fast
    erf (about 5x / 3.4x the float32 restatement's 1.8e-7 / 2.9e-7, which gate_table() measures again)."""
    return 2.0 ** -8 * ref.abs() + 1e-6 * x.double().abs().clamp_min(1.0)


def gelu_erf_unit():
    """max |float32 erf formula - float64| / max(1, |x|) over the grid: (GELU, GELU')."""
    x = gelu_values()
    scale = x.double().abs().clamp_min(1.0)
    return tuple(((a.double() - r).abs() / scale).max().item() for a, r in zip(gelu_erf_f32(x), gelu_ref(x)))


# measured by gelu_erf_unit() on the CPU (gate_table() repeats it and holds it to these): the fp32 epilogue gets 4 x this
# times max(1, |x|), plus 4 units in the last place of the reference
GELU_ERF_UNIT = (8.3e-8, 9.8e-8)


def gelu_gate_f32(x, ref, which):
    return 4.0 * GELU_ERF_UNIT[which] * x.double().abs().clamp_min(1.0) + 4.0 * 2.0 ** -23 * ref.abs()


# --------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------
def _rel(a, b, gross=None):
    a, b = a.double(), b.double()
    den = b.norm().item()
    if gross is not None and den <= 1e-9 * gross.double().norm().item():
        den = gross.double().norm().item()
    return (a - b).norm().item() / (den if den > 0 else 1.0)


_TABLE = None


def gate_table(detail=False):
    """[(what, measured, gate, factor)]: the error against float64 of every reference's float32 restatement over the inputs of
    the GPU module, beside the gate the GPU module applies there; measured <= gate / factor must hold (factor 4 but for the fast GELU').  Computed once per process (about 10 s on the CPU)."""
    global _TABLE
    if _TABLE is not None and not detail:
        return _TABLE
    w, tag = {}, [""]

    def note(key, e, gate, factor=4.0):
        key = key + (f" [{tag[0]}]" if detail and tag[0] else "")
        w[(key, gate, factor)] = max(w.get((key, gate, factor), 0.0), e)

    B, H = MHLA_B, MHLA_H
    for path, L, W, hd, recipe, masked, p, waves in mhla_grid():
        if waves:
            continue                                                   # the same inputs as waves = 0
        dtype, D = MHLA_PATHS[path][0], H * hd
        tag[0] = recipe
        qkv, dout = mhla_inputs(recipe, dtype, B, L, H, hd, W)
        mask = padding_mask(B, L, W) if masked else None
        keep = R.mhla_keep(SEED, B, H, L, W, p) if p > 0 else None
        o64, g64, l64 = mhla_run(qkv, dout, B, L, H, hd, W, mask, keep, p, F64)
        o32, g32, l32 = mhla_run(qkv, dout, B, L, H, hd, W, mask, keep, p, F32)
        gross = R.mhla_grad_scale(qkv.double(), dout.double(), B, L, H, hd, W, mask, keep, p)
        rg = ROW_GATE_F32["mhla"]
        note("mhla out rel-L2", _rel(o32, o64), MHLA_OUT_TOL[F32])
        note("mhla out worst row", R.row_error(o32, o64, o64, B * L).max().item(), rg)
        for part, nm in enumerate(("dq", "dk", "dv")):
            sl = slice(part * D, (part + 1) * D)
            note(f"mhla {nm} rel-L2", _rel(g32[:, sl], g64[:, sl], gross[:, sl] if part < 2 else None), MHLA_GRAD_TOL[F32])
            den = gross[:, sl] if part < 2 else g64[:, sl]
            note(f"mhla {nm} worst row" + (" (gross)" if part < 2 else ""), R.row_error(g32[:, sl], g64[:, sl], den, B * L).max().item(), rg)
        live = torch.isfinite(l64)
        note("mhla lse abs", (l32.double() - l64)[live].abs().max().item() if bool(live.any()) else 0.0, MHLA_LSE_ABS)
    for dtype, B, H, Lq, Lk, hd, recipe, mkind, waves in sdpa_grid():
        if waves:
            continue
        tag[0] = recipe
        q, k, v, dout = sdpa_inputs(recipe, dtype, B, H, Lq, Lk, hd)
        mk = key_mask(B, Lk) if mkind else None
        r64 = sdpa_run(q, k, v, dout, B, H, Lq, Lk, hd, mk, None, 0.0, F64)
        r32 = sdpa_run(q, k, v, dout, B, H, Lq, Lk, hd, mk, None, 0.0, F32)
        gq, gk = R.sdpa_grad_scale(*(heads(t.double(), B, L_, H, hd) for t, L_ in ((q, Lq), (k, Lk), (v, Lk), (dout, Lq))),
                                   1.0 / math.sqrt(hd), None if mk is None else mk[:, None, None, :], None, 0.0)
        rg = ROW_GATE_F32["sdpa"]
        m32 = [merged(t, B, L_, H, hd) if t.dim() == 4 else t for t, L_ in zip(r32, (Lq, 0, Lq, Lk, Lk))]      # rows as the
        m64 = [merged(t, B, L_, H, hd) if t.dim() == 4 else t for t, L_ in zip(r64, (Lq, 0, Lq, Lk, Lk))]      # library writes them
        note("sdpa o rel-L2", _rel(m32[0], m64[0]), SDPA_OUT_TOL[F32])
        note("sdpa o worst row", R.row_error(m32[0], m64[0], m64[0], B * Lq).max().item(), rg)
        note("sdpa lse rel-L2", _rel(r32[1], r64[1]), SDPA_LSE_TOL[F32])
        for nm, i, gross, L_ in (("dq", 2, gq, Lq), ("dk", 3, gk, Lk), ("dv", 4, None, Lk)):
            gm = merged(gross, B, L_, H, hd) if gross is not None else None
            note(f"sdpa {nm} rel-L2", _rel(m32[i], m64[i], gm), SDPA_GRAD_TOL[F32])
            note(f"sdpa {nm} worst row" + (" (gross)" if gross is not None else ""),
                 R.row_error(m32[i], m64[i], gm if gm is not None else m64[i], B * L_).max().item(), rg)
    tag[0] = ""
    # attention maps: the probabilities themselves
    for recipe in ("offset+", "spread"):
        for dtype in (F32, BF16):
            qkv, _ = mhla_inputs(recipe, dtype, 2, 17, 2, 64, 7)
            s = mhla_scores(qkv, 2, 17, 2, 64, 7)
            note("maps window P rel-L2", _rel(torch.softmax(mhla_scores(qkv, 2, 17, 2, 64, 7, None, F32), -1), torch.softmax(s, -1)), MAPS_TOL["window"])
            qkv, _ = mhla_inputs(recipe, dtype, 2, 33, 2, 64, 7)
            t = qkv.double().reshape(2, 33, 3, 2, 64).permute(2, 0, 3, 1, 4)
            s32 = (t[0].to(F32) @ t[1].to(F32).transpose(-2, -1)) * (64 ** -0.5)
            note("maps dense P rel-L2", _rel(torch.softmax(s32, -1), torch.softmax((t[0] @ t[1].transpose(-2, -1)) * (64 ** -0.5), -1)), MAPS_TOL["dense"])
    # cross-entropy family
    for s_, o_ in LOGIT_RECIPES:
        for Cn in CE_CLASSES:
            case = logits_case(s_, o_, Cn)
            for kind in CE_KINDS:
                tag[0] = f"{kind} s={s_:g} o={o_:g}"
                ref = ce_reference(*case, kind)
                rows, kd, grad = ce_f32(*case, kind)
                grp = loss_group(kind)
                note(f"loss rows ({grp}), units of 2^-24 scale", ((rows.double() - ref["loss_rows"]).abs() / (U24 * ref["loss_scale"])).max().item(), LOSS_UNITS[grp])
                if ce_args(kind)[4]:
                    note("kd rows, units of 2^-24 scale", ((kd.double() - ref["kd_rows"]).abs() / (U24 * ref["kd_scale"])).max().item(), LOSS_UNITS[grp])
                if Cn > 1:
                    note("dlogits rel-L2", _rel(grad, ref["grad"]), DLOGITS_TOL)
    # LayerNorm
    for D in LN_DIMS:
        tag[0] = f"D={D}"
        x, gamma, beta, dy = ln_case("+100", LN_ROWS, D)
        r64, r32 = ln_run(x, gamma, beta, dy, F64), ln_run(x, gamma, beta, dy, F32)
        for nm, a, b in zip(("y", "mean", "rstd", "dx", "dgamma", "dbeta"), r32, r64):
            if nm == "mean":
                note("layernorm +100 mean, units of 2^-23 |mean|", ((a.double() - b).abs() / (2.0 ** -23 * b.abs())).max().item(), LN_TOL[nm])
            else:
                note(f"layernorm +100 {nm} rel-L2", _rel(a, b), LN_TOL[nm])
    # GELU
    tag[0] = ""
    x = gelu_values()
    ref = gelu_ref(x)
    for which, nm in enumerate(("GELU", "GELU'")):
        fast = gelu_fast_f32(x)[which].double()
        # (the issue sets 1e-6 max(1, |x|) as "about 5x" and "about 3.4x" the restatement: GELU' is held to that ratio)
        note(f"fast {nm}: |err| / max(1, |x|)", ((fast - ref[which]).abs() / x.double().abs().clamp_min(1.0)).max().item(), 1e-6,
             4.0 if which == 0 else 3.4)
        note(f"erf {nm} in float32: |err| / max(1, |x|)", gelu_erf_unit()[which], 4.0 * GELU_ERF_UNIT[which])
    table = [(k, e, g, f) for (k, g, f), e in w.items()]
    if not detail:
        _TABLE = table
    return table


def format_table(table):
    lines = [f"{'float32 restatement against float64 (CPU)':<52}{'measured':>12}{'gate':>12}{'gate / measured':>17}"]
    for what, e, gate, _ in table:
        lines.append(f"{what:<52}{e:>12.3e}{gate:>12.3g}{gate / max(e, 1e-300):>17.1f}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(format_table(gate_table(detail="--detail" in sys.argv)))
