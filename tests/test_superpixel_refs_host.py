"""CPU checks of tests/_superpixel_ref.py: the float64 references against the golden-checked oracle, the crafted maps'
component counts against the SLIC restatement, and the seed grid on elongated images."""
import numpy as np
import pytest
import torch

import _superpixel_ref as R
from oracle import favit_oracle as O
from oracle import slic_oracle as SO


def _random_case(seed):
    rs = np.random.RandomState(seed)
    P = int(rs.choice([2, 4, 8]))
    g = int(rs.choice([3, 5, 8]))
    cell = int(rs.choice([1, 2, P, 2 * P]))
    n = (P * g + cell - 1) // cell
    seg = np.kron(rs.randint(0, 9, size=(n, n)), np.ones((cell, cell), dtype=np.int64))[:P * g, :P * g].astype(np.int64)
    return seg, P, g


@pytest.mark.parametrize("kind", R.POOL_KINDS)
@pytest.mark.parametrize("seed", range(4))
def test_float64_pooling_agrees_with_the_oracle(kind, seed):
    """pool_forward in float64 against O.pool.  The bound is O.pool's own fp32 rounding, measured here as the distance
    between O.pool on the fp32 embeddings and O.pool on the same numbers in float64; against the float64 oracle the
    reference may differ by float64 rounding of sums of at most 64 terms only."""
    seg, P, g = _random_case(seed)
    mapping = O.map_patches(seg, P * g, P)
    groups = R.groups_of_mapping(mapping)
    emb = torch.randn(g * g, 24, generator=torch.Generator().manual_seed(seed))
    o32, o64 = O.pool(emb, mapping, kind).double(), O.pool(emb.double(), mapping, kind)
    ref = R.pool_forward(emb.double()[None], [groups], kind, len(groups))[0]
    own = (o32 - o64).abs().max().item()
    assert (ref - o64).abs().max().item() <= 64 * 2.3e-16 * o64.abs().max().item()
    assert (ref - o32).abs().max().item() <= 2 * own, (own,)
    if kind == "max":
        assert own == 0.0 and torch.equal(ref, o64)


@pytest.mark.parametrize("kind", R.POOL_KINDS)
def test_float64_pooling_backward_and_padding(kind):
    """pool_reference's gradient equals autograd over the float64 oracle; a token past the last group is a zero row,
    a dropped group leaves its patches without gradient."""
    seg, P, g = _random_case(7)
    mapping = O.map_patches(seg, P * g, P)
    groups = R.groups_of_mapping(mapping)
    n = len(groups)
    assert n >= 3
    gen = torch.Generator().manual_seed(3)
    emb = torch.randn(1, g * g, 16, generator=gen)
    gout = torch.randn(1, n + 2, 16, generator=gen)
    out, demb = R.pool_reference(emb, [groups], kind, n + 2, gout)
    e = emb[0].double().clone().requires_grad_(True)
    want = O.pool(e, mapping, kind)
    want.backward(gout[0, :n].double())
    assert (out[0, :n] - want.detach()).abs().max().item() <= 1e-13 and (out[0, n:] == 0).all()
    assert (demb[0] - e.grad).abs().max().item() <= 1e-13
    out, demb = R.pool_reference(emb, [groups], kind, n - 2, gout[:, :n - 2])
    dropped = groups[n - 2] + groups[n - 1]
    assert (demb[0, dropped] == 0).all() and (demb[0, groups[0]] != 0).any()
    assert R.groups_of_perm_offs(*R.mapping_tensors(mapping, g * g)[2:4]) == groups


@pytest.mark.parametrize("S", [4, 9, 16, 70])
def test_integer_centroids_agree_with_the_oracle(S):
    """The oracle averages fp32 coordinates (a rounding per pixel); the reference divides exact integer sums once."""
    rs = np.random.RandomState(S)
    segs = np.stack([np.kron(rs.randint(-2, S + 3, size=(8, 8)), np.ones((6, 6), dtype=np.int64)) for _ in range(2)])
    ref = R.centroids_reference(segs, S)
    want = O.superpixel_centroids(segs, S).double().numpy()
    assert np.abs(ref - want).max() <= 48 * 48 * 6e-8         # at most one fp32 rounding of a value <= 1 per pixel summed
    empty = [s for s in range(S) if not (segs[0] == s).any()]
    if empty:
        assert (ref[0, empty] == 0.5).all()


@pytest.mark.parametrize("prepend", [False, True])
def test_float64_posenc_agrees_with_the_oracle(prepend):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 9, 12, generator=gen)
    cent = torch.rand(2, 8 if prepend else 9, 2, generator=gen)
    assert (R.posenc_reference(x, cent) - O.dynamic_posenc(x, cent).double()).abs().max().item() < 4e-6
    assert (R.posenc_reference(x, None) - O.dynamic_posenc(x, None).double()).abs().max().item() < 4e-6


def test_checkerboards_have_2048_and_2049_components():
    a, b = R.checkerboard(), R.checkerboard(extra=True)
    assert a.shape == (R.BOARD_H, R.BOARD_W) and (a != b).sum() == 1
    _, na = SO.connect(a.reshape(-1), R.BOARD_H, R.BOARD_W, 0)
    _, nb = SO.connect(b.reshape(-1), R.BOARD_H, R.BOARD_W, 0)
    assert (na, nb) == (R.SLIC_MAXC, R.SLIC_MAXC + 1)
    # a cell's rows cross the chunk border
    assert a[0, R.CC_CHUNK - 1] == a[0, R.CC_CHUNK] and R.CC_CHUNK % R.CELL_W != 0


@pytest.mark.parametrize("W", R.CRAFTED_WIDTHS)
def test_crafted_maps_are_what_they_claim(W):
    H = R.CRAFTED_H
    st, nz, sp = R.crafted_batch(W)
    out, n = SO.connect(sp.reshape(-1), H, W, 0)
    assert n == 1 + H // 2                                    # label 0 is ONE component, every odd row another
    assert (out.reshape(H, W)[sp == 0] == 0).all()
    for m in (st, nz, sp):
        _, n = SO.connect(m.reshape(-1), H, W, 0)
        assert 1 < n <= R.SLIC_MAXC
    # runs cross every chunk border: same label on both sides, in the stripes' full-width bands and the serpentine's
    # even rows (at W = 257 the last chunk is the one pixel where an odd row may hold its label-0 link)
    for x in range(R.CC_CHUNK, W, R.CC_CHUNK):
        assert (st[:H // 2, x - 1] == st[:H // 2, x]).all() and (sp[0::2, x - 1] == sp[0::2, x]).all()
    _, n4 = SO.connect(nz.reshape(-1), H, W, 64)
    _, n0 = SO.connect(nz.reshape(-1), H, W, 0)
    assert 0 < n4 < n0                                         # some components are below min_size, some above


@pytest.mark.parametrize("H,W,n", [(8, 200, 16), (200, 8, 16), (5, 5, 64), (3, 4, 12), (2, 3, 64), (96, 96, 64),
                                   (41, 300, 9)])
def test_seed_grid_on_elongated_images(favit, H, W, n):
    assert favit.kernels.slic_grid(H, W, n) == SO.regular_grid_2d(H, W, n)
    ys, xs, step = SO.regular_grid_2d(H, W, n)
    assert ys and xs and step >= 1 and max(ys) < H and max(xs) < W


def test_seed_grid_takes_the_short_axis_whole():
    assert SO.regular_grid_2d(8, 200, 16)[0] == [4] and len(SO.regular_grid_2d(8, 200, 16)[1]) == 17
    assert SO.regular_grid_2d(200, 8, 16)[1] == [4]
    assert SO.regular_grid_2d(5, 5, 64) == ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 1)


@pytest.mark.parametrize("H,W,nseg,sigma,compactness,seed", R.ODD_SIZES)
def test_fp32_features_stay_within_the_device_rule_at_the_odd_sizes(H, W, nseg, sigma, compactness, seed):
    """The GPU tests allow the device's fp32 blur + CIELAB one quantisation step against the float64 oracle and ask for
    more than 95 % exact values.  A plain float32 restatement on the CPU keeps that rule at these sizes, so the
    sizes are fair to the device."""
    assert (H * W) % 4 != 0 or W % 4 != 0 or W > R.CC_CHUNK
    for i in range(3):
        img = R.smooth_image(H, W, seed * 10 + i)
        d = np.abs(R.features_f32(img, sigma).astype(np.int64) - SO.features(img, sigma).astype(np.int64))
        assert d.max() <= 1 and (d == 0).mean() > 0.95, (d.max(), (d == 0).mean())


def test_general_form_compactness_reaches_the_64_bit_kernel_without_overflow():
    ys, xs, step = SO.regular_grid_2d(96, 96, 9)
    coef = int(round((step / R.general_form_compactness(step)) ** 2))
    assert 2 ** 32 <= coef < 2 ** 32 + 2 ** 26
    assert coef * 3 * 16382 ** 2 + 2 * (16 * 2 * step + 16) ** 2 < 2 ** 63


def test_label_maps_for_the_patch_mapping():
    """The high-bit pairs are built so that merging l with l + 2^32 changes the dominant label of many patches."""
    seg = R.label_map("high_bit_pairs", 64, 8, 0)
    true = O.map_patches(seg, 64, 8)
    folded = O.map_patches(seg & 0xFFFFFFFF, 64, 8)
    dom_t, dom_f = R.mapping_tensors(true, 64)[0], R.mapping_tensors(folded, 64)[0]
    assert (dom_t != dom_f).mean() > 0.3
    assert np.unique(R.label_map("distinct", 42, 3, 1)).size == 42 * 42
    assert R.label_map("negative", 64, 8, 2).min() < -(1 << 33) and R.label_map("offset40", 64, 8, 3).min() >= 1 << 40
