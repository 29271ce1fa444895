"""CLS-only encoders (functional.cls_plan), host side: the closed-form row plan against a brute-force
receptive field built from the oracle's window table, the identity that lets a block run on its kept rows with the
unchanged window rule, and the oracle's own statement of the premise (rows outside the field get a zero gradient)."""
import numpy as np
import pytest
import torch

from oracle import favit_oracle as O

TRIPLES = [(197, 7, 12), (577, 7, 12), (17, 7, 12), (50, 7, 4), (30, 3, 5), (12, 5, 3), (65, 7, 12)]


def _needed_inputs(L, W, depth):
    """need[k] (k = 0 .. depth - 1): the input rows of block k + 1 that row 0 of the last block's output depends on
    (a row depends on itself through the residual and on every key in its window)."""
    idx = O.window_indices(L, W)
    need = [None] * depth
    out = {0}
    for k in range(depth - 1, -1, -1):
        rows = set(out)
        for i in out:
            rows.update(int(j) for j in idx[i])
        need[k] = rows
        out = rows
    return need


def _kept(L, cut):
    return set(range(L)) if cut is None else set(range(cut[0])) | set(range(L - cut[1], L))


@pytest.mark.parametrize("L,W,depth", TRIPLES)
def test_plan_covers_the_brute_force_receptive_field(favit, L, W, depth):
    plan = favit.functional.cls_plan(L, W, depth)
    assert len(plan) == depth
    need = _needed_inputs(L, W, depth)
    h = W // 2
    for k in range(depth):
        assert need[k] <= _kept(L, plan[k]), (k, sorted(need[k] - _kept(L, plan[k])))
        if plan[k] is not None:
            a, b = plan[k]
            assert a + b < L and a >= 1 and b >= 1
            assert need[k] == _kept(L, plan[k]), "the closed form is the field, not a superset"
            if k + 1 < depth:
                assert plan[k + 1] == (a - h, b - h)         # the next cut keeps the first a - h / last b - h kept rows
        elif k:
            assert plan[k - 1] is None                       # once all rows are needed, every block below needs them


def test_plan_row_counts_of_the_benchmark_shapes(favit):
    n2 = [sum(c) for c in favit.functional.cls_plan(197, 7, 12)]
    assert n2 == list(range(71, 4, -6)) and sum(n2) == 456
    plan4 = favit.functional.cls_plan(577, 7, 12)
    assert abs(sum(sum(c) for c in plan4) / (577 * 12) - 0.066) < 1e-3
    assert favit.functional.cls_plan(17, 7, 12)[:10] == [None] * 10       # the SPPP shapes run on all rows nearly everywhere


@pytest.mark.parametrize("L,W,depth", TRIPLES)
def test_compact_windows_equal_the_mapped_originals(favit, L, W, depth):
    """Block k on its n kept rows (head rows, then tail rows) with the window rule at L' = n: for every row the next
    block needs, the compact window, mapped back to original indices, is the original window, pad copies included."""
    plan = favit.functional.cls_plan(L, W, depth)
    need = _needed_inputs(L, W, depth)
    full = O.window_indices(L, W)
    for k in range(depth):
        if plan[k] is None:
            continue
        a, b = plan[k]
        n = a + b
        comp = O.window_indices(n, W)
        wanted = need[k + 1] if k + 1 < depth else {0}
        assert wanted <= _kept(L, plan[k])
        for r in sorted(wanted):
            c = r if r < a else r - (L - n)
            back = np.where(comp[c] < a, comp[c], comp[c] + (L - n))
            np.testing.assert_array_equal(back, full[r], err_msg=f"block {k + 1}, row {r}")


def test_oracle_pos_embed_gradient_is_zero_outside_block_one_rows(favit):
    torch.manual_seed(7)
    L, W, depth, D, H = 50, 7, 4, 32, 2
    m = favit.models.vit_mhla.VisionTransformerMHLA(img_size=112, patch_size=16, num_classes=10, embed_dim=D, depth=depth,
                                                    num_heads=H, window_size=W, use_mhla=True)
    assert m.pos_embed.shape[1] == L
    sd = {k: v.clone().float().requires_grad_(True) for k, v in m.state_dict().items()}
    x = torch.randn(3, 3, 112, 112)
    y = torch.randint(0, 10, (3,))
    O.cross_entropy(O.vit_mhla_forward(x, sd, 16, H, W, True), y).backward()
    g = sd["pos_embed"].grad[0]
    a, b = favit.functional.cls_plan(L, W, depth)[0]
    assert (a, b) == (13, 10)
    inside = torch.zeros(L, dtype=torch.bool)
    inside[:a] = True
    inside[L - b:] = True
    assert torch.count_nonzero(g[~inside]).item() == 0
    assert (g[inside].abs().amax(dim=1) > 0).all()
