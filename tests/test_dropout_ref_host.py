"""CPU checks of tests/_dropout_ref.py: the host restatement of the dropout draw behaves as common.h documents, and
the explicit-mask float64 attention references reduce, with an all-true mask and p = 0, to the formulations the suite
already trusts (oracle.favit_oracle.mhla_attention, golden-checked against the reference project, and plain
softmax(q k^T) v).  The bit-for-bit tie to the library's own draw is tests/test_gpu_dropout_masks.py."""
import numpy as np
import pytest
import torch

import _dropout_ref as R
from conftest import rel_l2
from oracle import favit_oracle as O

N = 1 << 20


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5, 0.9])
def test_keep_rate_within_five_sigma(p):
    for seed in (1, 0x123456789ABCDEF):
        rate = R.keep_mask(seed, N, p).mean()
        # p is realised to 1 / 65536: the expected rate is that of the 16-bit threshold
        want = 1.0 - R.threshold16(p) / 65536.0
        assert abs(want - (1 - p)) <= 1.0 / 65536
        assert abs(rate - want) < 5 * (p * (1 - p) / N) ** 0.5, (p, seed, rate)


def test_p_zero_keeps_everything():
    assert R.threshold16(0.0) == 0
    assert R.keep_mask(7, N, 0.0).all()
    assert R.keep_scale(0.0) == 1.0


def test_pair_elements_share_one_draw():
    """Elements 2i and 2i + 1 are decided by the low and the high half of the draw of counter i."""
    seed, p = 0x1234567800000005, 0.25
    h = R.rand_u32(seed, np.arange(N // 2))
    assert h.max() < 2 ** 32 and len(np.unique(h)) == N // 2, "an affine map and a bijective finaliser: no repeats"
    t = R.threshold16(p)
    m = R.keep_mask(seed, N, p)
    assert np.array_equal(m[0::2], (h & 0xFFFF) >= t)
    assert np.array_equal(m[1::2], (h >> 16) >= t)
    # an index array gives the mask of exactly those elements, in any shape and order
    pick = np.array([[5, 4], [N - 1, 0], [77, 76]])
    assert np.array_equal(R.keep_mask(seed, pick, p), m[pick])


def test_counter_above_32_bits_uses_the_high_word():
    seed = 99
    lo = R.rand_u32(seed, np.array([3, 4, 5]))
    hi = R.rand_u32(seed, np.array([3, 4, 5], dtype=np.uint64) + (np.uint64(1) << np.uint64(32)))
    assert not np.array_equal(lo, hi)


def test_seeds_that_differ_only_in_the_high_word_give_different_masks():
    a = R.keep_mask(0x0000000100000005, N, 0.5)
    b = R.keep_mask(0x0000000200000005, N, 0.5)
    c = R.keep_mask(0x0000000000000005, N, 0.5)
    for x, y in ((a, b), (a, c), (b, c)):
        agree = (x == y).mean()
        assert abs(agree - 0.5) < 5 * 0.5 / N ** 0.5, "independent fair masks agree on half of the elements"


def _mask(B, L, g):
    m = torch.rand(B, L, L, generator=g) > 0.4
    m |= torch.eye(L, dtype=torch.bool)
    return m.to(torch.uint8)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L,W,hd", [(5, 3, 16), (5, 7, 16), (17, 5, 32), (40, 15, 16), (33, 9, 8), (70, 7, 64)])
def test_mhla_ref_equals_the_multiplicity_bias_formulation(L, W, hd, masked):
    """All-true keep, p = 0: the window-gather core == the dense core with bias log(multiplicity) of
    oracle.favit_oracle.mhla_attention (fed identity projections, so only the attention core is compared)."""
    B, H = 2, 3
    D = H * hd
    g = torch.Generator().manual_seed(L * 31 + W)
    x = torch.randn(B, L, D, generator=g, dtype=torch.float64)
    wqkv = torch.randn(3 * D, D, generator=g, dtype=torch.float64) / D ** 0.5
    eye_h, eye_d, z = torch.eye(hd, dtype=torch.float64), torch.eye(D, dtype=torch.float64), torch.zeros
    sd = {"a.qkv.weight": wqkv, "a.qkv.bias": z(3 * D, dtype=torch.float64), "a.latent_proj.weight": eye_h,
          "a.latent_proj.bias": z(hd, dtype=torch.float64), "a.proj.weight": eye_d, "a.proj.bias": z(D, dtype=torch.float64)}
    mask = _mask(B, L, g) if masked else None
    want = O.mhla_attention(x, sd, "a.", H, W, mask).reshape(B * L, D)
    qkv = (x @ wqkv.t()).reshape(B * L, 3 * D)
    dout = torch.randn(B * L, D, generator=g, dtype=torch.float64)
    keep = torch.ones(B, H, L, W, dtype=torch.bool)
    out, dqkv, lse = R.mhla_ref(qkv, dout, B, L, H, hd, W, mask, keep, 0.0)
    assert rel_l2(out, want) < 1e-12
    out2, dqkv2, lse2 = R.mhla_ref(qkv, dout, B, L, H, hd, W, mask, None, 0.0)
    assert torch.equal(out, out2) and torch.equal(dqkv, dqkv2) and torch.equal(lse, lse2)
    # the gradient too: autograd through the oracle's formulation on the same qkv
    t = qkv.reshape(B, L, 3, H, hd).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    mult = torch.from_numpy(O.window_multiplicity(L, W)).double()
    s = (t[0] @ t[1].transpose(-2, -1)) / hd ** 0.5
    s = s + torch.where(mult > 0, torch.log(mult.clamp_min(1.0)), torch.full_like(mult, float("-inf")))
    if mask is not None:
        s = s.masked_fill(mask[:, None] == 0, float("-inf"))
    (torch.softmax(s, -1) @ t[2]).transpose(1, 2).reshape(B * L, D).backward(dout)
    assert rel_l2(dqkv, t.grad.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * D)) < 1e-12
    assert rel_l2(lse, torch.logsumexp(s.detach(), -1)) < 1e-12


def test_mhla_ref_dropout_scales_the_kept_slots():
    """One row by hand: L = 5, W = 3, row 0 has the window (0, 1, 4) -- the end pad is key L - 1."""
    B, H, L, hd, W, p = 1, 1, 5, 4, 3, 0.5
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(L, 3 * hd, generator=g, dtype=torch.float64)
    keep = torch.ones(B, H, L, W, dtype=torch.bool)
    keep[0, 0, 0] = torch.tensor([True, False, True])
    out, _, _ = R.mhla_ref(qkv, torch.zeros(L, hd, dtype=torch.float64), B, L, H, hd, W, None, keep, p)
    q, k, v = qkv[:, :hd], qkv[:, hd:2 * hd], qkv[:, 2 * hd:]
    assert list(O.window_indices(L, W)[0]) == [0, 1, 4]
    pr = torch.softmax(torch.stack([q[0] @ k[0], q[0] @ k[1], q[0] @ k[4]]) / hd ** 0.5, 0)
    assert rel_l2(out[0], (pr[0] * v[0] + pr[2] * v[4]) / (1 - p)) < 1e-12


@pytest.mark.parametrize("mask_kind", [None, "full", "keys"])
def test_sdpa_ref_equals_plain_softmax_attention(mask_kind):
    B, H, Lq, Lk, hd = 2, 3, 7, 11, 8
    g = torch.Generator().manual_seed(5)
    q, dout = (torch.randn(B, H, Lq, hd, generator=g, dtype=torch.float64) for _ in range(2))
    k, v = (torch.randn(B, H, Lk, hd, generator=g, dtype=torch.float64) for _ in range(2))
    mask = None
    if mask_kind == "full":
        mask = torch.rand(B, 1, Lq, Lk, generator=g) > 0.4
        mask[..., 0] = True
    elif mask_kind == "keys":
        mask = (torch.rand(B, 1, 1, Lk, generator=g) > 0.3)
        mask[..., 0] = True
    scale = hd ** -0.5
    keep = torch.ones(B, H, Lq, Lk, dtype=torch.bool)
    o, lse, dq, dk, dv = R.sdpa_ref(q, k, v, dout, scale, mask, keep, 0.0)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (qr @ kr.transpose(-2, -1)) * scale
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    want = torch.softmax(s, -1) @ vr
    want.backward(dout)
    for got, ref in ((o, want), (lse, torch.logsumexp(s, -1)), (dq, qr.grad), (dk, kr.grad), (dv, vr.grad)):
        assert rel_l2(got, ref) < 1e-12


def test_sdpa_ref_fully_masked_row_is_zero_and_gives_no_gradient():
    B, H, Lq, Lk, hd = 2, 2, 5, 6, 4
    g = torch.Generator().manual_seed(6)
    q, dout = (torch.randn(B, H, Lq, hd, generator=g, dtype=torch.float64) for _ in range(2))
    k, v = (torch.randn(B, H, Lk, hd, generator=g, dtype=torch.float64) for _ in range(2))
    mask = torch.rand(B, 1, Lq, Lk, generator=g) > 0.4
    mask[..., 0] = True
    mask[1, 0, 2] = False
    o, lse, dq, dk, dv = R.sdpa_ref(q, k, v, dout, 0.5, mask, None, 0.0)
    assert all(bool(torch.isfinite(t).all()) for t in (o, dq, dk, dv))
    assert bool((o[1, :, 2] == 0).all()) and bool((dq[1, :, 2] == 0).all()) and bool((lse[1, :, 2] == float("-inf")).all())
    # the other rows are what they are without that query row
    sel = [0, 1, 3, 4]
    o2, _, dq2, dk2, dv2 = R.sdpa_ref(q[1:, :, sel], k[1:], v[1:], dout[1:, :, sel], 0.5, mask[1:, :, sel], None, 0.0)
    assert rel_l2(o[1:, :, sel], o2) < 1e-12 and rel_l2(dq[1:, :, sel], dq2) < 1e-12
    assert rel_l2(dk[1:], dk2) < 1e-12 and rel_l2(dv[1:], dv2) < 1e-12
