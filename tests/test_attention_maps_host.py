"""Attention maps without a GPU: functional.window_indices against the tables captured from the reference, the
properties of the float64 rollout of tests/_attention_ref.py (mass, the cls_plan cone), the header's declarations and
what functional.capture_attention switches off or refuses."""
import os

import numpy as np
import pytest
import torch

import _attention_ref as R
from conftest import load_golden
from oracle import favit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_indices_equal_every_table_captured_from_the_reference(favit):
    g = load_golden("windows.npz")
    assert len(g.files) > 0
    for key in g.files:
        L, W = (int(s[1:]) for s in key.split("_"))
        got = favit.functional.window_indices(L, W)
        assert got.dtype == torch.int64 and tuple(got.shape) == (L, W) and got.device.type == "cpu"
        assert np.array_equal(got.numpy(), g[key]), key


@pytest.mark.parametrize("L,W", [(1, 7), (2, 3), (5, 7), (6, 7), (7, 7), (8, 7), (9, 7), (40, 15), (65, 7)])
def test_window_indices_equal_the_oracle_where_no_table_was_captured(favit, L, W):
    assert np.array_equal(favit.functional.window_indices(L, W).numpy(), O.window_indices(L, W))


def test_window_indices_refuses_even_and_empty(favit):
    for L, W in [(5, 4), (5, 0), (0, 3)]:
        with pytest.raises(ValueError):
            favit.functional.window_indices(L, W)


def _row_stochastic(B, L, W, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, L, W, generator=g, dtype=torch.float64) + 0.05
    return p / p.sum(-1, keepdim=True)


@pytest.mark.parametrize("L,W,depth", [(17, 3, 4), (65, 7, 6), (197, 7, 12), (9, 7, 2), (6, 7, 2), (50, 5, 3)])
def test_reference_rollout_keeps_its_mass_and_stays_inside_the_cls_plan_cone(favit, L, W, depth):
    probs = [_row_stochastic(2, L, W, 1000 * L + 10 * W + k) for k in range(depth)]
    for residual in (0.5, 0.0):
        r = R.rollout(probs, [W] * depth, 0, residual)
        assert tuple(r.shape) == (2, L)
        assert (r.sum(1) - 1).abs().max().item() < 1e-12
        assert (r >= 0).all()
    # after rolling back through block k (1-based) r is the weight on block k's INPUT rows: the rows cls_plan lists
    plan = favit.functional.cls_plan(L, W, depth)
    for k in range(depth, 0, -1):
        r = R.rollout(probs[k - 1:], [W] * (depth - k + 1), 0, 0.5)
        if plan[k - 1] is None:
            continue
        head, tail = plan[k - 1]
        assert (r[:, head:L - tail] == 0).all(), (k, head, tail)
        assert (r[:, :head] > 0).all() and (r[:, L - tail:] > 0).all(), (k, head, tail)


@pytest.mark.parametrize("L,W", [(1, 7), (4, 7), (6, 7), (9, 3), (20, 15)])
def test_reference_rollout_is_the_double_loop_over_row_and_slot(L, W):
    probs = [_row_stochastic(2, L, W, 77 + L + k) for k in range(3)]
    idx = O.window_indices(L, W)
    r = np.zeros((2, L))
    r[:, L // 2] = 1.0
    for P in reversed(probs):
        acc = np.zeros((2, L))
        for i in range(L):
            for w in range(W):
                acc[:, idx[i, w]] += r[:, i] * P[:, i, w].numpy()
        r = 0.3 * r + 0.7 * acc
    assert np.abs(R.rollout(probs, [W] * 3, L // 2, 0.3).numpy() - r).max() < 1e-15


def test_reference_rollout_dense_block_is_a_matrix_product():
    P = _row_stochastic(2, 9, 9, 5)
    r = R.rollout([P], [0], 3, 0.25)
    want = 0.25 * torch.eye(9, dtype=torch.float64)[3] + 0.75 * P[:, 3, :]
    assert (r - want).abs().max().item() < 1e-15


def test_reference_per_key_sums_the_pad_slots():
    P = _row_stochastic(1, 6, 7, 9)
    dense = R.per_key(P, 7)
    idx = O.window_indices(6, 7)
    for i in range(6):
        for j in range(6):
            assert abs(dense[0, i, j].item() - sum(P[0, i, w].item() for w in range(7) if idx[i, w] == j)) < 1e-15


@pytest.mark.parametrize("kind", ["vit", "vit_mhla", "vit_mhla_dense", "sppp_mhla"])
def test_reference_whole_model_agrees_with_the_oracle_forward(favit, kind):
    """The pass that keeps the probabilities computes the logits the oracle's own forward computes."""
    torch.manual_seed(3)
    M = favit.models
    kw = dict(img_size=32, patch_size=4, num_classes=10, embed_dim=64, depth=2, num_heads=2)
    x = torch.randn(2, 3, 32, 32)
    segmaps = None
    if kind == "vit":
        sd = M.vit.VisionTransformer(**kw).state_dict()
        want = O.vit_forward(x, sd, 4, 2)
    elif kind == "sppp_mhla":
        sd = M.sppp_mhla.SPPPViTMHLA(window_size=7, use_mhla=True, num_superpixels=16, **kw).state_dict()
        segmaps = np.stack([O.voronoi_labels(32, 16, seed=3), O.voronoi_labels(32, 16, seed=8)])
        assert len({len(O.map_patches(s, 32, 4)) for s in segmaps}) == 1
        want = O.sppp_vit_mhla_forward(x, segmaps, sd, 4, 2, 7, True)
    else:
        sd = M.vit_mhla.VisionTransformerMHLA(window_size=7, use_mhla=(kind == "vit_mhla"), **kw).state_dict()
        want = O.vit_mhla_forward(x, sd, 4, 2, 7, kind == "vit_mhla")
    got = R.model_maps(kind, x, sd, 4, 2, 7, segmaps=segmaps)
    assert (got["logits"] - want.double()).norm().item() < 1e-5 * want.double().norm().item()
    L = got["rollout"].shape[1]
    assert len(got["layers"]) == 2 and tuple(got["cls_attention"].shape) == (2, L)
    assert (got["rollout"].sum(1) - 1).abs().max().item() < 1e-12
    assert (got["cls_attention"].sum(1) - 1).abs().max().item() < 1e-12


def test_header_declares_the_entry_points_and_the_abi_is_still_8(favit):
    A, K = favit._abi, favit.kernels
    with open(os.path.join(ROOT, "include", "favit.h")) as f:
        text = f.read()
    for name in ("favit_mhla_attn_probs", "favit_sdpa_probs", "favit_attn_rollout"):
        assert name in A.declared_symbols()
        assert name in A._SIGS
        assert f"int {name}(" in text
    assert A.ABI_VERSION == 8
    assert A.ROLLOUT_MAX_LAYERS == 32 and K.ROLLOUT_MAX_LAYERS == 32
    assert len(A._SIGS["favit_mhla_attn_probs"][0]) == 11
    assert len(A._SIGS["favit_sdpa_probs"][0]) == 11
    assert len(A._SIGS["favit_attn_rollout"][0]) == 9
    # L = 3137 (224 / patch 4, plus CLS) has to fit the rollout's two rows in LDS
    assert K.ROLLOUT_MAX_L >= 3137 and 2 * 4 * K.ROLLOUT_MAX_L <= 160 * 1024


def _specs(F, depth, W=7):
    return [F.BlockSpec(F.MHLAChain(4, W), F.MLPChain()) for _ in range(depth)]


def test_capture_switches_pruning_off(favit):
    F = favit.functional
    specs = _specs(F, 4)
    assert F.cls_only_cuts(specs, 65, None, False) is not None
    with F.capture_attention() as cap:
        assert F.cls_only_cuts(specs, 65, None, False) is None
        assert cap.layers == [] and cap.per_head is False
    assert F.cls_only_cuts(specs, 65, None, False) is not None


def test_capture_switches_the_native_blocks_off(favit):
    F = favit.functional
    old = F.get_compute_mode()
    F.set_compute_dtype("bf16")
    try:
        before = F._native_blocks_on()
        with F.capture_attention():
            assert not F._native_blocks_on()
        assert F._native_blocks_on() == before
    finally:
        F.set_compute_dtype(old)


def test_nested_capture_raises_and_the_outer_one_survives(favit):
    F = favit.functional
    with F.capture_attention(per_head=True) as cap:
        with pytest.raises((RuntimeError, ValueError), match="nest"):
            with F.capture_attention():
                pass
        assert F._CAPTURE["active"] is cap and cap.per_head is True
    assert F._CAPTURE["active"] is None


def test_capture_is_released_when_the_body_raises(favit):
    F = favit.functional
    with pytest.raises(KeyError):
        with F.capture_attention():
            raise KeyError("x")
    assert F._CAPTURE["active"] is None


def test_training_mode_forward_raises_under_capture(favit):
    F = favit.functional
    xn = torch.zeros(10, 16)
    with F.capture_attention():
        with pytest.raises(RuntimeError, match="training"):
            F.MHLAChain(2, 3).fwd(xn, [None] * 6, 2, 5, None, None, True)
        with pytest.raises(RuntimeError, match="training"):
            F.DenseChain(2).fwd(xn, [None] * 4, 2, 5, None, None, True)


def test_cross_chain_raises_under_capture(favit):
    F = favit.functional
    with F.capture_attention():
        with pytest.raises(RuntimeError, match="CrossChain"):
            F.CrossChain(1).fwd(torch.zeros(10, 16), torch.zeros(10, 16), [None] * 8, 2, 5, 5, None, None, False)


def test_fp8_mode_raises_under_capture(favit):
    F = favit.functional
    old = F.get_compute_mode()
    F.set_compute_dtype("fp8")
    try:
        with pytest.raises(RuntimeError, match="fp8"):
            with F.capture_attention():
                pass
        assert F._CAPTURE["active"] is None
    finally:
        F.set_compute_dtype(old)


def test_wrappers_name_the_offending_shape(favit):
    K = favit.kernels
    with pytest.raises(ValueError, match=r"\(10, 90\)"):
        K.mhla_attn_probs(torch.zeros(10, 90), 2, 5, 2, 16, 7)
    with pytest.raises(ValueError, match="W = 4"):
        K.mhla_attn_probs(torch.zeros(10, 96), 2, 5, 2, 16, 4)
    with pytest.raises(ValueError, match=r"\(10, 90\)"):
        K.sdpa_probs(torch.zeros(10, 90), 2, 5, 2, 16)
    with pytest.raises(ValueError, match=r"\(2, 4\)"):
        K.sdpa_probs(torch.zeros(10, 96), 2, 5, 2, 16, key_keep=torch.ones(2, 4, dtype=torch.uint8))
    p = torch.zeros(2, 9, 7)
    with pytest.raises(ValueError, match=r"\(2, 9, 5\)"):
        K.attn_rollout([p, torch.zeros(2, 9, 5)], [7, 7])
    with pytest.raises(ValueError, match="33 maps"):
        K.attn_rollout([p] * 33, [7] * 33)
    with pytest.raises(ValueError, match="cls_row = 9"):
        K.attn_rollout([p], [7], cls_row=9)
    with pytest.raises(ValueError, match="residual"):
        K.attn_rollout([p], [7], residual=1.5)
    with pytest.raises(ValueError, match=r"widths\[0\] = 4"):
        K.attn_rollout([torch.zeros(2, 9, 4)], [4])
