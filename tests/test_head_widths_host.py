"""Host checks behind tests/test_gpu_head_widths.py, which compares the dense attention modules at head widths the
fused kernel does not take with oracle/favit_oracle.py evaluated in FLOAT64.

  a. the float64 path of the oracle reproduces the stored goldens (captured from the reference in fp32) at the
     tolerance tests/test_oracle_golden.py uses for the fp32 path: the oracle's functions are dtype-agnostic, and this
     pins the dtype the GPU tests use;
  b. _dropout_ref.cross_attention_ref (the oracle's two cross-attention functions restated with P = 0 on a query row
     whose keys are all masked) equals the oracle to 1e-12 rel-L2 in float64, output and every gradient, where no row
     is dead;
  c. with a dead row, its output row is out_proj.bias and it contributes nothing to any gradient: the k / v (and every
     other) gradient equals that of the same problem with the query row removed."""
import numpy as np
import pytest
import torch

import _dropout_ref as R
from conftest import case, load_golden, rel_l2, sd_of
from oracle import favit_oracle as O

TOL = 2e-5          # tests/test_oracle_golden.py
D, H = 64, 4
F64 = torch.float64
VP, CR = load_golden("vit_parts.npz"), load_golden("cross.npz")


def _golden_f64(c, fn, n_in=1):
    """test_oracle_golden._fwd_bwd with every tensor promoted to float64."""
    sd = {k: v.double().requires_grad_(True) for k, v in sd_of(c).items()}
    ins = [torch.from_numpy(c[f"in{i}"]).double().requires_grad_(True) for i in range(n_in)]
    y = fn(sd, *ins)
    assert y.dtype == F64
    assert rel_l2(y, c["out"]) < TOL, "forward"
    (y * torch.from_numpy(c["gout"]).double()).sum().backward()
    for i, t in enumerate(ins):
        assert rel_l2(t.grad, c[f"gin{i}"]) < 5 * TOL, f"grad input {i}"
    for k, v in sd.items():
        g = v.grad if v.grad is not None else torch.zeros_like(v)
        ref = c[f"grad/{k}"]
        if np.abs(ref).max() < 1e-5:
            assert g.abs().max().item() < 1e-5, k
        else:
            assert rel_l2(g, ref) < 5 * TOL, f"grad {k}"


def test_float64_oracle_reproduces_the_goldens():
    _golden_f64(case(VP, "mha_L17"), lambda sd, x: O.dense_mha(x, sd, "", H))
    _golden_f64(case(VP, "vm_block_mhla0_L17"), lambda sd, x: O.vit_mhla_block(x, sd, "", H, 7, False))
    c = case(CR, "ca_mask1")
    m = torch.from_numpy(c["attention_mask"])
    _golden_f64(c, lambda sd, q, kv: O.cross_attention(q, kv, sd, "", m), n_in=2)
    c = case(CR, "mhca_mask1")
    m = torch.from_numpy(c["attention_mask"])
    _golden_f64(c, lambda sd, q, kv: O.multihead_cross_attention(q, kv, sd, "", H, m), n_in=2)


def _cross_problem(Dm, B, Lq, Lk, seed, masked):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        sd[f"{n}.weight"] = torch.randn(Dm, Dm, generator=g, dtype=F64) * Dm ** -0.5
        sd[f"{n}.bias"] = torch.randn(Dm, generator=g, dtype=F64) * 0.1
    q, kv = torch.randn(B, Lq, Dm, generator=g, dtype=F64), torch.randn(B, Lk, Dm, generator=g, dtype=F64)
    gout = torch.randn(B, Lq, Dm, generator=g, dtype=F64)
    mask = None
    if masked:
        mask = (torch.rand(B, Lq, Lk, generator=g) > 0.4).to(torch.uint8)
        mask[..., 0] = 1
    return sd, q, kv, gout, mask


def _grads(fn, sd, q, kv, gout):
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    q, kv = q.detach().clone().requires_grad_(True), kv.detach().clone().requires_grad_(True)
    y = fn(q, kv, sd)
    (y * gout).sum().backward()
    return y.detach(), dict({k: v.grad for k, v in sd.items()}, q=q.grad, kv=kv.grad)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Dm,heads", [(72, 1), (40, 1), (96, 4), (72, 6)])
def test_cross_restatement_equals_the_oracle_in_float64(Dm, heads, masked):
    sd, q, kv, gout, mask = _cross_problem(Dm, 2, 5, 40, Dm + heads, masked)
    oracle = (lambda a, b, s: O.cross_attention(a, b, s, "", mask)) if heads == 1 else \
        (lambda a, b, s: O.multihead_cross_attention(a, b, s, "", heads, mask))
    y0, g0 = _grads(oracle, sd, q, kv, gout)
    y1, g1 = _grads(lambda a, b, s: R.cross_attention_ref(a, b, s, heads, mask), sd, q, kv, gout)
    assert rel_l2(y1, y0) < 1e-12
    for k in g0:
        if k == "k_proj.bias":          # analytically zero: both are rounding noise
            assert g0[k].abs().max().item() < 1e-12 and g1[k].abs().max().item() < 1e-12
        else:
            assert rel_l2(g1[k], g0[k]) < 1e-12, k


@pytest.mark.parametrize("Dm,heads", [(72, 1), (72, 6)])
def test_cross_restatement_dead_row_is_bias_and_sends_no_gradient(Dm, heads):
    B, Lq, Lk, dead = 1, 6, 21, 2
    sd, q, kv, gout, mask = _cross_problem(Dm, B, Lq, Lk, 7 * Dm + heads, True)
    mask[0, dead] = 0
    assert torch.isnan(O.multihead_cross_attention(q, kv, sd, "", heads, mask)[0, dead]).all(), "the oracle gives NaN there"
    y, g = _grads(lambda a, b, s: R.cross_attention_ref(a, b, s, heads, mask), sd, q, kv, gout)
    assert torch.isfinite(y).all() and all(torch.isfinite(t).all() for t in g.values())
    assert torch.equal(y[0, dead], sd["out_proj.bias"])
    assert bool((g["q"][0, dead] == 0).all())
    live = [i for i in range(Lq) if i != dead]
    y2, g2 = _grads(lambda a, b, s: R.cross_attention_ref(a, b, s, heads, mask[:, live]), sd, q[:, live], kv, gout[:, live])
    assert rel_l2(y[:, live], y2) < 1e-12
    # the dead row reaches the k / v projections through nothing; out_proj.bias sees its row of the output gradient
    for k in ("k_proj.weight", "v_proj.weight", "v_proj.bias", "q_proj.weight", "q_proj.bias", "out_proj.weight", "kv"):
        assert rel_l2(g[k], g2[k]) < 1e-12, k
    assert rel_l2(g["q"][:, live], g2["q"]) < 1e-12
    assert rel_l2(g["out_proj.bias"], g2["out_proj.bias"] + gout[0, dead]) < 1e-12
