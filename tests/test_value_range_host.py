"""CPU tests of tests/_value_range.py: they pin the inputs and the gates of tests/test_gpu_value_range.py.

  1. every recipe is where it claims to be: the float64 lse lies beyond +-88 (offset) or spans more than 88 (spread),
     88.7 being where exp leaves fp32;
  2. the inputs discriminate: exp(s) / sum exp(s) in float32, without the row maximum, is non-finite on every recipe,
     and a one-pass variance misses the LayerNorm gate on the rows of randn + 100 by a factor of ten and more;
  3. the float32 restatement of every reference stays within a quarter of the gate the GPU module applies to the same
     inputs (the whole table is printed: run with -s).

No kernel runs here, and no number of this file or of _value_range.py was read off one."""
import math

import pytest
import torch

import _dropout_ref as R
import _value_range as VR

F32, BF16, F64 = VR.F32, VR.BF16, VR.F64
EXP_LIMIT = 88.0


def _mhla_lse_and_naive(recipe):
    """(all live float64 lse values, naive float32 rows that came out finite / rows) over the MHLA grid of one recipe."""
    B, H = VR.MHLA_B, VR.MHLA_H
    lse, finite, rows = [], 0, 0
    for path, L, W, hd, rec, masked, p, waves in VR.mhla_grid():
        if rec != recipe or waves or p:
            continue
        qkv, _ = VR.mhla_inputs(recipe, VR.MHLA_PATHS[path][0], B, L, H, hd, W)
        s = VR.mhla_scores(qkv, B, L, H, hd, W, VR.padding_mask(B, L, W) if masked else None)
        live = torch.isfinite(s).any(-1)
        lse.append(torch.logsumexp(s[live], -1))
        ok = torch.isfinite(VR.naive_softmax32(s[live])).all(-1)
        finite, rows = finite + int(ok.sum()), rows + int(live.sum())
    return torch.cat(lse), finite, rows


def _sdpa_lse_and_naive(recipe):
    lse, finite, rows = [], 0, 0
    for dtype, B, H, Lq, Lk, hd, rec, mkind, waves in VR.sdpa_grid():
        if rec != recipe or waves:
            continue
        q, k, _, _ = VR.sdpa_inputs(recipe, dtype, B, H, Lq, Lk, hd)
        s = (VR.heads(q.double(), B, Lq, H, hd) @ VR.heads(k.double(), B, Lk, H, hd).transpose(-2, -1)) / math.sqrt(hd)
        if mkind:
            s = s.masked_fill(~VR.key_mask(B, Lk)[:, None, None, :], float("-inf"))
        lse.append(torch.logsumexp(s, -1).flatten())
        ok = torch.isfinite(VR.naive_softmax32(s)).all(-1)
        finite, rows = finite + int(ok.sum()), rows + ok.numel()
    return torch.cat(lse), finite, rows


@pytest.mark.parametrize("family,recipe", [("mhla", r) for r in VR.ATTN_RECIPES] + [("sdpa", r) for r in VR.ATTN_RECIPES + VR.STREAM_RECIPES])
def test_attention_recipes_leave_the_range_of_exp(family, recipe):
    lse, finite, rows = (_mhla_lse_and_naive if family == "mhla" else _sdpa_lse_and_naive)(recipe)
    lo, hi = lse.min().item(), lse.max().item()
    print(f"{family} {recipe}: lse in [{lo:.1f}, {hi:.1f}]; exp(s) / sum without the maximum is finite on {finite} of {rows} rows")
    if recipe == "offset+":
        assert lo > EXP_LIMIT and finite == 0, "every row overflows"
    elif recipe == "offset-":
        # (exp(-93) is still a denormal on the CPU; a GPU flushes it.  Below -103.3 it is 0 everywhere.)
        assert hi < -EXP_LIMIT and finite < 0.2 * rows, "nearly every row underflows to 0 / 0"
    else:
        assert hi - lo > EXP_LIMIT and hi > EXP_LIMIT
        assert finite <= 0.95 * rows, "at least one row in twenty holds a score beyond the range of exp"


def test_streamed_recipes_move_the_running_maximum():
    """late-max: the maximum over the first 32 j keys rises with j = 1 .. 4 for nearly every query row, so a streamed
    softmax rescales at every block; early-max: it is final after the first block and exp(m_block - m) underflows."""
    B, H, Lq, Lk, hd = VR.STREAM_SHAPE
    for recipe in VR.STREAM_RECIPES:
        q, k, _, _ = VR.sdpa_inputs(recipe, F32, B, H, Lq, Lk, hd)
        s = (VR.heads(q.double(), B, Lq, H, hd) @ VR.heads(k.double(), B, Lk, H, hd).transpose(-2, -1)) / math.sqrt(hd)
        run = torch.stack([s[..., :min(32 * (j + 1), Lk)].max(-1).values for j in range(4)], -1)        # [B, H, Lq, 4]
        block = torch.stack([s[..., 32 * j:min(32 * (j + 1), Lk)].max(-1).values for j in range(4)], -1)
        if recipe == "late-max":
            rises = (run[..., 1:] > run[..., :-1]).float().mean().item()
            print(f"late-max: the running maximum rises at {100 * rises:.0f} % of the block steps")
            assert rises > 0.6
            assert ((run[..., -1] - run[..., 0]) > EXP_LIMIT).float().mean().item() > 0.5, "alpha underflows to 0"
        else:
            final = (run[..., 0] == run[..., -1]).float().mean().item()
            gap = (run[..., -1] - block[..., -1] > EXP_LIMIT).float().mean().item()
            print(f"early-max: the maximum is final after block 0 on {100 * final:.0f} % of the rows; the last block "
                  f"lies more than {EXP_LIMIT:g} below it on {100 * gap:.0f} %")
            assert final > 0.6 and gap > 0.5


@pytest.mark.parametrize("s,o", VR.LOGIT_RECIPES)
def test_logit_recipes(s, o):
    """(3, 0) is the scale of the older tests.  (30, -100) breaks a loss without the maximum only on short rows (with
    63 classes and more the row maximum sits between -50 and +20); it is there for rows whose label's logit lies 200
    below their lse."""
    finite = rows = 0
    lo, hi = math.inf, -math.inf
    for Cn in VR.CE_CLASSES:
        x, z, labels, lam = VR.logits_case(s, o, Cn)
        assert x.shape == z.shape == (VR.CE_B, Cn) and not torch.equal(x, z)
        lse = torch.logsumexp(x.double(), 1)
        lo, hi = min(lo, lse.min().item()), max(hi, lse.max().item())
        ok = torch.isfinite(VR.naive_lse32(x))
        finite, rows = finite + int(ok.sum()), rows + ok.numel()
    print(f"logits {s:g} randn {o:+g}: lse in [{lo:.1f}, {hi:.1f}]; log sum exp without the maximum finite on {finite} of {rows} rows")
    if (s, o) == (3.0, 0.0):
        assert finite == rows
    elif o < 0:
        assert finite < rows and lo < -EXP_LIMIT
    else:
        assert finite < rows and hi > EXP_LIMIT
        for Cn in [Cn for Cn in VR.CE_CLASSES if Cn >= 63]:
            assert not bool(torch.isfinite(VR.naive_lse32(VR.logits_case(s, o, Cn)[0])).any()), "every row overflows"
    if o < 0:
        x, _, labels, _ = VR.logits_case(s, o, 1000)
        gap = torch.logsumexp(x.double(), 1) - x.double().gather(1, labels[:, None])[:, 0]
        assert gap.max().item() > 100, "a label far below the maximum"


@pytest.mark.parametrize("D", VR.LN_DIMS)
def test_one_pass_variance_misses_the_gate(D):
    x, gamma, beta, dy = VR.ln_case("+100", VR.LN_ROWS, D)
    ref = VR.ln_run(x, gamma, beta, dy, F64)
    two, one = VR.ln_run(x, gamma, beta, dy, F32), VR.ln_run(x, gamma, beta, dy, F32, one_pass=True)
    e2, e1 = VR._rel(two[0], ref[0]), VR._rel(one[0], ref[0])
    r2, r1 = VR._rel(two[2], ref[2]), VR._rel(one[2], ref[2])
    print(f"D={D}: y two-pass {e2:.2e}, one-pass {e1:.2e} (gate {VR.LN_TOL['y']:g}); rstd {r2:.2e} / {r1:.2e} (gate {VR.LN_TOL['rstd']:g})")
    assert e2 < VR.LN_TOL["y"] / 4 and r2 < VR.LN_TOL["rstd"] / 4
    assert (not math.isfinite(e1)) or e1 > 10 * VR.LN_TOL["y"]
    assert (not math.isfinite(r1)) or r1 > 10 * VR.LN_TOL["rstd"]


def test_constant_and_tiny_rows():
    """Sums of D <= 2048 copies of 0, 3 or -1024 are exact in fp32 in any order, so mean == the constant and y == beta
    are bit-exact demands; the float64 reference agrees.  Rows of 1e-20 randn have a variance far below eps."""
    for D in VR.LN_DIMS:
        x, gamma, beta, dy = VR.ln_case("const", VR.LN_ROWS, D)
        assert set(x[:, 0].tolist()) == set(VR.LN_CONSTANTS) and bool((x == x[:, :1]).all())
        assert max(abs(c) for c in VR.LN_CONSTANTS) * D < 2 ** 24, "every partial sum is an integer below 2^24"
        y, mu, rs, dx, dg, db = VR.ln_run(x, gamma, beta, dy, F64)
        assert torch.equal(mu, x[:, 0].double()) and torch.equal(y, beta.double().expand_as(y))
        assert bool((rs == 1.0 / math.sqrt(VR.LN_EPS)).all()) and float(dg.abs().max()) == 0.0
        y32 = VR.ln_run(x, gamma, beta, dy, F32)
        assert torch.equal(y32[0], beta.expand_as(y32[0])) and torch.equal(y32[1], x[:, 0])
        xt = VR.ln_case("tiny", VR.LN_ROWS, D)[0]
        assert 0 < float(xt.abs().max()) < 1e-19 and float(xt.double().var(-1).max()) < 1e-6 * VR.LN_EPS


def test_gelu_grid():
    v = VR.gelu_values()
    assert torch.equal(v, v.to(BF16).float()), "every grid value is a bf16 value"
    assert v.numel() <= 200 * 64, "the grid fits the smaller GEMM"
    for x in (0.0, 13.5, -13.5, 30.0, -30.0, 12.0, -12.0, 2.0 ** -10):
        assert bool((v == x).any())
    assert bool(((v == 0) & torch.signbit(v)).any()), "-0 is in the grid"
    inside = v[(v.abs() <= 12) & (v != 0)].abs().unique()
    assert float((inside[1:] / inside[:-1]).max()) <= 1 + 2.0 ** -7 + 1e-9, "no bf16 value of [2^-10, 12] is left out"
    g = VR.gelu_grid(200)
    assert g.shape == (200, 64) and torch.equal(g.flatten()[:v.numel()], v)
    gelu, dgelu = VR.gelu_ref(v)
    assert bool((gelu[v < 0] <= 0).all()) and bool((gelu[v < 0] > -0.17).all())
    assert -0.13 < dgelu.min().item() and dgelu.max().item() < 1.13
    assert gelu[v == 30].item() == 30.0 and abs(gelu[v == -30].item()) < 1e-190
    # 1 + erf loses the negative tail in float64 already; the reference does not
    naive = 0.5 * v.double() * (1 + torch.erf(v.double() / math.sqrt(2)))
    tail = v < -8.5
    assert bool((naive[tail] == 0).all()) and bool((gelu[tail] < 0).all())


def test_grids_hold_the_cases_of_the_issue():
    grid = VR.mhla_grid()
    count = {path: sum(1 for c in grid if c[0] == path) for path in VR.MHLA_PATHS}
    assert count == VR.MHLA_NEED, count
    assert sum(1 for c in grid if c[6] > 0) == len(VR.MHLA_PATHS), "one dropout case per kernel path"
    assert {c[7] for c in grid if c[0] == "lse" and c[4] == "offset+" and c[6] == 0} == {0, 1, 4}
    assert {c[7] for c in grid if not (c[0] == "lse" and c[4] == "offset+")} == {0}
    sg = VR.sdpa_grid()
    assert len(sg) == VR.SDPA_NEED
    assert {c[8] for c in sg if c[6] == "late-max"} == {0, 4, 5} and {c[8] for c in sg if c[6] != "late-max"} == {0}
    for path, L, W, hd, recipe, masked, p, waves in grid:
        if masked:
            dead = R.mhla_dead_rows(VR.padding_mask(VR.MHLA_B, L, W), L, W)
            assert int(dead.sum()) == R.mask_family_dead_count("padding", VR.MHLA_B, L, W)


def test_loss_scale_is_the_issue_rule_where_the_lse_dominates():
    """max(1, |lse|) of the issue, and larger only where an operand of the difference is: at 30 randn - 100 the label's
    logit is near -200 beside an lse near 0, and the correctly rounded fp32 loss is already off by 2^-24 * 200."""
    for s, o in VR.LOGIT_RECIPES:
        x, z, labels, lam = VR.logits_case(s, o, 1000)
        base, _ = VR.loss_scale(x, z, labels, None, 0.0, 1.0, None)
        lse = torch.logsumexp(x.double(), 1)
        xl = x.double().gather(1, labels[:, None])[:, 0]
        assert torch.equal(base, torch.stack((torch.ones_like(lse), lse.abs(), xl.abs())).max(0).values)
        loss = lse - xl
        rounded = loss.to(F32).double()
        print(f"logits {s:g} randn {o:+g}: |lse| {lse.abs().min():.1f} .. {lse.abs().max():.1f}, |x_label| up to {xl.abs().max():.1f}; "
              f"rounding the loss to fp32 costs up to {((rounded - loss).abs() / (VR.U24 * lse.abs().clamp_min(1))).max():.2f} units of |lse|")
        assert bool(((rounded - loss).abs() <= VR.U24 * 2 * base).all())


def test_bf16_dense_attention_gates():
    """The bf16 whole-tensor gates of the dense kernel stay the suite's 1e-2 / 2e-2 but where a float64 restatement
    that rounds P and dS to bf16 where the kernels do misses them itself: dq on the offset recipes at hd = 16, which
    gets twice the restatement's error.  Every gate stays far below the O(1) error of a wrong kernel."""
    over = set()
    for dtype, B, H, Lq, Lk, hd, recipe, mkind, waves in VR.sdpa_grid():
        if dtype != BF16 or waves:
            continue
        q, k, v, dout = VR.sdpa_inputs(recipe, dtype, B, H, Lq, Lk, hd)
        mk = VR.key_mask(B, Lk) if mkind else None
        ref = VR.sdpa_run(q, k, v, dout, B, H, Lq, Lk, hd, mk, None, 0.0, F64)
        gates, errs = VR.sdpa_bf16_gates(q, k, v, dout, B, H, Lq, Lk, hd, mk, ref)
        print(f"Lq={Lq} Lk={Lk} hd={hd} {recipe:9s} {str(mkind):5s} restatement o {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} "
              f"dv {errs[3]:.2e}; gates " + " ".join(f"{g_:.2e}" for g_ in gates))
        assert all(math.isfinite(e) and e < 0.07 for e in errs) and max(gates) < 0.15
        over |= {(nm, hd, recipe) for nm, g_, b_ in zip(("o", "dq", "dk", "dv"), gates, (1e-2, 2e-2, 2e-2, 2e-2)) if g_ != b_}
    assert over == {("dq", 16, "offset+"), ("dq", 16, "offset-")}, over


def test_float32_restatements_stay_within_a_quarter_of_every_gate():
    table = VR.gate_table()
    print("\n" + VR.format_table(table))
    assert len(table) >= 35
    bad = [(what, e, gate) for what, e, gate, factor in table if not (math.isfinite(e) and e <= gate / factor)]
    assert not bad, bad
    # a gate that is 4 x a measurement is no wider than that: the measurement may not have shrunk below a fifth of it
    derived = ("mhla dv worst row", "sdpa dv worst row", "sdpa o rel-L2", "sdpa dk rel-L2", "maps dense P rel-L2",
               "loss rows (weighted)", "kd rows", "layernorm +100 y", "layernorm +100 mean", "layernorm +100 dgamma", "erf GELU")
    for what, e, gate, factor in table:
        if what.startswith(derived):
            assert e > gate / 5, f"{what}: the gate {gate:g} is more than 5 x the restatement's {e:.3e}; derive it again"
