"""The superpixel front end (csrc/slic.hip, csrc/sppp.hip) at the shapes where its kernels change path.

SLIC: rows wider than one 256-pixel chunk of the connectivity kernels, the 2048-component limit and its fallback, the
64-bit assignment kernel, images whose pixel count / width is no multiple of the four pixels a thread owns, 64
centres, elongated images, and one many-image run of the centre update that rides on the last workgroup to arrive.
SPPP: the patch mapping at its register / LDS boundary and at both limits with 64-bit and negative labels, pooling
forward AND backward of all three kinds per row against float64 with empty, dropped, one-patch and all-patch groups,
centroids across the privatised / single-copy boundary, the positional encoding in both forms, and the model with max
and attention pooling.  References: oracle/slic_oracle.py (bit-exact integer stages), oracle/favit_oracle.py (bit-exact
mapping) and the float64 restatements of tests/_superpixel_ref.py (checked on the CPU by test_superpixel_refs_host.py)."""
import functools

import numpy as np
import pytest
import torch

import _superpixel_ref as R
from conftest import rel_l2
from oracle import favit_oracle as O
from oracle import slic_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID, UNSUPPORTED = r"\(code -1\)", r"\(code -2\)"


@pytest.fixture(scope="module")
def K(favit):
    return favit.kernels


# ----------------------------------------------------------------------------------------------------------------
# SLIC stage 3 on crafted cluster maps
# ----------------------------------------------------------------------------------------------------------------
def _connect(favit, labels, min_size):
    """favit_slic_connect on uint8 maps [B, H, W] with the buffers kernels.slic sets up.  Returns (out, n_regions)."""
    K = favit.kernels
    B, H, W = labels.shape
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(DEV).reshape(B, H * W)
    ws = torch.empty((2, B, H * W), dtype=torch.int32, device=DEV)
    out = torch.empty((B, H, W), dtype=torch.int64, device=DEV)
    nreg = torch.empty(B, dtype=torch.int32, device=DEV)
    favit._abi.check(favit._abi.lib().favit_slic_connect(K._p(lab), K._p(ws[0]), K._p(ws[1]), K._p(out), K._p(nreg), B, H, W,
                                                         int(min_size), K._st()), "favit_slic_connect")
    torch.cuda.synchronize()
    return out.cpu().numpy(), nreg.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _crafted_reference(W, min_size):
    return [SO.connect(m.reshape(-1), R.CRAFTED_H, W, min_size) for m in R.crafted_batch(W)]


@pytest.mark.parametrize("min_size", [0, 4, 64])
@pytest.mark.parametrize("W", R.CRAFTED_WIDTHS)
def test_connectivity_on_rows_wider_than_one_chunk(favit, W, min_size):
    """cc_runs_kernel / cc_merge_kernel beyond 256 pixels per row: runs restart at chunk borders and are re-joined by
    unions.  Three different maps in one batch (full-width and diagonal stripes, blocky noise, one serpentine component
    of deep union chains); components below min_size merge into a neighbour of their first pixel.  Bit for bit."""
    maps = R.crafted_batch(W)
    out, nreg = _connect(favit, maps, min_size)
    for b, (ref_o, ref_n) in enumerate(_crafted_reference(W, min_size)):
        assert int(nreg[b]) == ref_n, (b, int(nreg[b]), ref_n)
        np.testing.assert_array_equal(out[b].reshape(-1), ref_o, err_msg=f"image {b}")


def test_component_count_limit_and_fallback(favit):
    """2048 components are relabelled like any image; 2049 make n_regions = -1 and out = the cluster map
    (include/favit.h).  Both in one batch, the overfull board between two full ones: its fallback stays its own."""
    full, over = R.checkerboard(), R.checkerboard(extra=True)
    maps = np.stack([full, over, full])
    out, nreg = _connect(favit, maps, 0)
    ref_o, ref_n = SO.connect(full.reshape(-1), R.BOARD_H, R.BOARD_W, 0)
    assert ref_n == R.SLIC_MAXC
    assert nreg.tolist() == [R.SLIC_MAXC, -1, R.SLIC_MAXC]
    for b in (0, 2):
        np.testing.assert_array_equal(out[b].reshape(-1), ref_o, err_msg=f"image {b}")
    np.testing.assert_array_equal(out[1], over.astype(np.int64))
    # small components of the full board merge as the oracle merges them (every cell is below 16 pixels)
    out, nreg = _connect(favit, maps[[0, 2]], 16)
    ref_o, ref_n = SO.connect(full.reshape(-1), R.BOARD_H, R.BOARD_W, 16)
    assert nreg.tolist() == [ref_n, ref_n]
    np.testing.assert_array_equal(out[0].reshape(-1), ref_o)
    np.testing.assert_array_equal(out[1].reshape(-1), ref_o)


# ----------------------------------------------------------------------------------------------------------------
# SLIC stage by stage against the oracle
# ----------------------------------------------------------------------------------------------------------------
def _check_stages(K, imgs, nseg, sigma, compactness, floor):
    """tests/test_slic.py's stage test: float stage within one quantisation step of the float64 oracle with more than
    `floor` of the values exact, integer stages bit-exact from the device's own features."""
    B, _, H, W = imgs.shape
    out, feat, lab, nreg = K.slic(torch.from_numpy(imgs).to(DEV), n_segments=nseg, compactness=compactness, sigma=sigma,
                                  stages=True)
    torch.cuda.synchronize()
    ys, xs, step = SO.regular_grid_2d(H, W, nseg)
    assert K.slic_grid(H, W, nseg) == (ys, xs, step)
    coef = int(round((step / float(compactness)) ** 2))
    min_size = int(0.5 * (H * W / float(len(ys) * len(xs))))
    feat, lab, out, nreg = feat.cpu().numpy(), lab.cpu().numpy(), out.cpu().numpy(), nreg.cpu().numpy()
    for b in range(B):
        ref_f = SO.features(imgs[b], sigma)
        diff = np.abs(feat[b, :, :3].astype(np.int64) - ref_f.astype(np.int64))
        assert diff.max() <= 1 and (diff == 0).mean() > floor, (b, diff.max(), (diff == 0).mean())
        assert (feat[b, :, 3] == 0).all()
        ref_l = SO.cluster(feat[b, :, :3], H, W, ys, xs, step, coef, iters=10)
        np.testing.assert_array_equal(lab[b].reshape(-1), ref_l, err_msg=f"cluster labels, image {b}")
        ref_o, ref_n = SO.connect(lab[b].reshape(-1), H, W, min_size)
        assert 0 <= ref_n
        np.testing.assert_array_equal(out[b].reshape(-1), ref_o, err_msg=f"regions, image {b}")
        assert int(nreg[b]) == ref_n
    return step, coef


def _images(H, W, seed, n=3):
    return np.stack([R.smooth_image(H, W, seed * 10 + i) for i in range(n)])


def test_general_64_bit_assignment(K):
    """slic_assign_kernel<false>: coef >= 2^32 sends the call to the 64-bit form.  The compactness comes from the step;
    neither the oracle's int64 nor the kernel's 64-bit distance can wrap (features within +-8191, window of 2 steps)."""
    H = W = 96
    ys, xs, step = SO.regular_grid_2d(H, W, 9)
    compactness = R.general_form_compactness(step)
    coef = int(round((step / float(compactness)) ** 2))
    assert coef >= 2 ** 32
    assert coef * 3 * 16382 ** 2 + 2 * (16 * 2 * step + 16) ** 2 < 2 ** 63
    assert _check_stages(K, _images(H, W, 50), 9, 1.0, compactness, 0.95) == (step, coef)


@pytest.mark.parametrize("H,W,nseg,sigma,compactness,seed", R.ODD_SIZES)
def test_odd_image_sizes(K, H, W, nseg, sigma, compactness, seed):
    """H*W % 4 != 0 (the last thread's four pixels run past the image), W % 4 != 0 (a thread's pixels straddle a row
    end), W > 256 (chunked connectivity on real cluster maps)."""
    assert (H * W) % 4 != 0 or W % 4 != 0 or W > 256
    _check_stages(K, _images(H, W, seed), nseg, sigma, compactness, 0.95)


def test_centre_count_limits(K):
    """K = 64 centres (the limit) bit-exact; a seed grid of more than 64 is refused; a blur radius above 32 is
    unsupported; an 8 x 200 image (shorter than the step: the short axis gets one row of seeds) matches the oracle."""
    ys, xs, _ = SO.regular_grid_2d(96, 96, 64)
    assert len(ys) * len(xs) == 64
    _check_stages(K, _images(96, 96, 34), 64, 1.0, 1.0, 0.95)
    ys, xs, _ = SO.regular_grid_2d(96, 96, 100)
    assert len(ys) * len(xs) > 64
    img = torch.from_numpy(_images(96, 96, 34, n=1)).to(DEV)
    with pytest.raises(ValueError, match="at most 64 seed centres"):
        K.slic(img, n_segments=100)
    assert int(4.0 * 8.2 + 0.5) == 33
    with pytest.raises(RuntimeError, match="favit_slic_features.*" + UNSUPPORTED):
        K.slic(img, n_segments=9, sigma=8.2)
    K.slic(img, n_segments=9, sigma=8.1)                      # radius 32 runs
    ys, xs, step = SO.regular_grid_2d(8, 200, 16)
    assert len(ys) == 1 and min(8, 200) < step
    _check_stages(K, _images(8, 200, 35), 16, 1.0, 1.0, 0.95)


def test_many_images_across_the_chip(K):
    """The centre update of an iteration is done by the last assignment workgroup of an image to arrive (no fence
    between its neighbours' atomics and their tickets).  64 images of 192 x 192 -- 36 workgroups of 1024 pixels per
    image, 2304 in all, on every XCD at once, ten iterations -- built from 8 distinct images repeated 8 times in
    shuffled positions: every copy must give its source image's oracle result in all four stages.  One run."""
    H = W = 192
    nseg, compactness, sigma = 16, 10.0, 1.0
    src = _images(H, W, 60, n=8)
    order = np.random.RandomState(6).permutation(64)
    which = order % 8                                           # batch position -> source image
    assert np.bincount(which).tolist() == [8] * 8 and (which[:8] != np.arange(8)).any()
    imgs = src[which]
    out, feat, lab, nreg = K.slic(torch.from_numpy(imgs).to(DEV), n_segments=nseg, compactness=compactness, sigma=sigma,
                                  stages=True)
    torch.cuda.synchronize()
    feat, lab, out, nreg = feat.cpu().numpy(), lab.cpu().numpy(), out.cpu().numpy(), nreg.cpu().numpy()
    ys, xs, step = SO.regular_grid_2d(H, W, nseg)
    coef = int(round((step / compactness) ** 2))
    min_size = int(0.5 * (H * W / float(len(ys) * len(xs))))
    bad = []
    for s in range(8):
        pos = np.nonzero(which == s)[0]
        ref_f = SO.features(src[s], sigma)
        diff = np.abs(feat[pos[0], :, :3].astype(np.int64) - ref_f.astype(np.int64))
        assert diff.max() <= 1 and (diff == 0).mean() > 0.95, (s, diff.max(), (diff == 0).mean())
        ref_l = SO.cluster(feat[pos[0], :, :3], H, W, ys, xs, step, coef, iters=10)
        ref_o, ref_n = SO.connect(ref_l, H, W, min_size)
        for b in pos:
            ok = (np.array_equal(feat[b], feat[pos[0]]) and np.array_equal(lab[b].reshape(-1), ref_l)
                  and np.array_equal(out[b].reshape(-1), ref_o) and int(nreg[b]) == ref_n)
            if not ok:
                bad.append((int(b), s, int((lab[b].reshape(-1) != ref_l).sum())))
    assert not bad, f"(batch position, source image, wrong cluster labels): {bad}"


# ----------------------------------------------------------------------------------------------------------------
# SPPP: patch -> superpixel mapping
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _map_case(HW, P, kind, image):
    seg = R.label_map(kind, HW, P, seed=1000 * HW + 10 * P + image)
    return seg, R.mapping_tensors(O.map_patches(seg, HW, P), (HW // P) ** 2)


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("HW,P", [(64, 32), (80, 40), (128, 64), (128, 2), (42, 3)])
def test_patch_mapping_sweep(K, HW, P, B):
    """dominant_label_kernel at n = P*P = 1024 (the last register-path size), 1600 (LDS path), 4096 (limit), rank_kernel at
    N = 4096 (48 KiB of LDS, its limit), an odd small shape; b > 0; labels that are all distinct, beyond 2^40, equal in
    their low 32 bits, negative.  Dominant label, rank, token count, perm and offs bit for bit."""
    N = (HW // P) ** 2
    for kind in R.MAP_KINDS:
        cases = [_map_case(HW, P, kind, i) for i in range(B)]
        seg = torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV)
        rank, ntok, perm, offs, dom = (t.cpu().numpy() for t in K.sppp_map_patches(seg, P))
        for b, (_, (rdom, rrank, rperm, roffs, rn)) in enumerate(cases):
            np.testing.assert_array_equal(dom[b], rdom, err_msg=f"{kind}: dominant label, image {b}")
            np.testing.assert_array_equal(rank[b], rrank, err_msg=f"{kind}: rank, image {b}")
            assert int(ntok[b]) == rn, (kind, b)
            np.testing.assert_array_equal(offs[b], roffs, err_msg=f"{kind}: offs, image {b}")
            np.testing.assert_array_equal(perm[b], rperm, err_msg=f"{kind}: perm, image {b}")
            assert offs[b, N] == N and offs[b, 0] == 0 and sorted(perm[b].tolist()) == list(range(N))


def test_patch_mapping_limits(K):
    seg = torch.zeros((1, 130, 130), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        K.sppp_map_patches(seg, 2)                            # N = 65 * 65 = 4225 patches
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        K.sppp_map_patches(seg, 65)                           # 4225 pixels per patch
    with pytest.raises(RuntimeError, match=INVALID):
        K.sppp_map_patches(seg[:, :64, :64].contiguous(), 5)


# ----------------------------------------------------------------------------------------------------------------
# SPPP: pooling
# ----------------------------------------------------------------------------------------------------------------
POOL_HW, POOL_P = 32, 4


@functools.lru_cache(maxsize=None)
def _pool_maps():
    """Three images with different token counts: ONE group of all 64 patches; blocky noise with groups of one patch;
    four quadrants."""
    rs = np.random.RandomState(11)
    one = np.full((POOL_HW, POOL_HW), 3, dtype=np.int64)
    many = np.kron(rs.randint(0, 40, size=(8, 8)), np.ones((4, 4), dtype=np.int64))
    ar = np.arange(POOL_HW)
    quad = ((ar[:, None] >= 16) * 2 + (ar[None, :] >= 16)).astype(np.int64)
    segs = np.stack([one, many, quad])
    groups = [R.groups_of_mapping(O.map_patches(s, POOL_HW, POOL_P)) for s in segs]
    counts = [len(g) for g in groups]
    assert counts[0] == 1 and len(groups[0][0]) == 64 and counts[2] == 4 and counts[1] > 8
    assert min(len(g) for g in groups[1]) == 1
    return segs, groups


def _pool_device(K, emb, perm, offs, kind, Rt, gout):
    e = emb.to(DEV).contiguous()
    out, argmax = K.sppp_pool_fwd(e, perm, offs, kind, Rt)
    demb = K.sppp_pool_bwd(gout.to(DEV).contiguous(), e, perm, offs, argmax, kind, Rt)
    torch.cuda.synchronize()
    return out.cpu(), demb.cpu()


def _pool_fp32_restatement(emb, groups, kname, Rt, gout):
    """O.pool and its autograd in fp32 on the CPU, image by image (zero rows for missing groups)."""
    e = emb.clone().requires_grad_(True)
    rows = []
    for b in range(emb.shape[0]):
        g = groups[b][:Rt]
        o = O.pool(e[b], dict(enumerate(g)), kname)
        rows.append(torch.cat([o, o.new_zeros(Rt - len(g), emb.shape[2])]))
    out = torch.stack(rows)
    out.backward(gout)
    return out.detach(), e.grad


@pytest.mark.parametrize("D", [32, 192, 260, 384])
@pytest.mark.parametrize("kname", R.POOL_KINDS)
def test_pooling_forward_and_backward_per_row(K, kname, D):
    """favit_sppp_pool_fwd / _bwd against float64, B = 3 images of 1, many and 4 tokens.  R = the largest count: the
    other images' surplus tokens are empty groups (zero rows forward, nothing backward).  R = the largest count - 3:
    the dropped groups' patches get zero gradient (what assume_num_tokens relies on).  D = 260 and 384 take the
    channel loop past 256 threads.

    Whole tensors: rel_l2 < 2e-5.  Per token row forward and per patch row backward: error / (row norm + 1e-3 * mean row
    norm) at most 4 x the worst such error of the fp32 CPU restatement (O.pool and its autograd) on the same inputs
    -- measured in the test, per kind, width and R.  Measured for these inputs (smallest .. largest over the widths
    and both R): mean 8.7e-8 .. 1.06e-7 forward, 2.5e-8 .. 2.8e-8 backward; attention 1.6e-7 .. 9.2e-7 forward,
    8.1e-7 .. 3.7e-6 backward; max pooling 0 both ways, where the kernel must then be exact as well.  The factor 4
    allows for the kernel's other summation order (and its 1 / count multiplication where autograd divides)."""
    kind = R.POOL_KINDS.index(kname)
    segs, groups = _pool_maps()
    N = (POOL_HW // POOL_P) ** 2
    _, ntok, perm, offs, _ = K.sppp_map_patches(torch.from_numpy(segs).to(DEV), POOL_P)
    assert ntok.tolist() == [len(g) for g in groups]
    for b in range(3):
        assert R.groups_of_perm_offs(perm[b].cpu(), offs[b].cpu()) == groups[b]
    gen = torch.Generator().manual_seed(D)
    emb = torch.randn(3, N, D, generator=gen) * 0.3
    Rmax = max(len(g) for g in groups)
    for Rt in (Rmax, Rmax - 3):
        gout = torch.randn(3, Rt, D, generator=gen)
        ref_o, ref_d = R.pool_reference(emb, groups, kname, Rt, gout)
        got_o, got_d = _pool_device(K, emb, perm, offs, kind, Rt, gout)
        cpu_o, cpu_d = _pool_fp32_restatement(emb, groups, kname, Rt, gout)
        assert rel_l2(got_o, ref_o) < 2e-5 and rel_l2(got_d, ref_d) < 2e-5, (kname, Rt)
        for what, got, cpu, ref in (("forward", got_o, cpu_o, ref_o), ("backward", got_d, cpu_d, ref_d)):
            measured = R.row_errors(cpu, ref).max().item()
            err = R.row_errors(got, ref)
            print(f"pool {kname} D={D} R={Rt} {what}: fp32 restatement {measured:.3e}, kernel {err.max().item():.3e}")
            assert err.max().item() <= 4 * measured, (kname, Rt, what, int(err.argmax()), err.max().item(), measured)
        # empty groups: zero rows; dropped or absent groups: no gradient
        for b in range(3):
            n = min(len(groups[b]), Rt)
            assert (got_o[b, n:] == 0).all(), (b, "rows of empty groups")
            gone = [p for g in groups[b][Rt:] for p in g]
            assert (got_d[b, gone] == 0).all(), (b, "patches of dropped groups")
        if kname == "max":
            assert torch.equal(got_o.double(), ref_o), "the maximum is one of the inputs: bit-equal"


def test_max_pooling_with_ties(K):
    """Embeddings rounded to a few values, so that most groups hold their maximum several times: the forward is still
    the exact maximum; backward, for every (image, token, channel), exactly ONE patch of the group receives go[d],
    that patch holds the maximum, every other patch receives 0."""
    segs, groups = _pool_maps()
    N, D = (POOL_HW // POOL_P) ** 2, 260
    _, _, perm, offs, _ = K.sppp_map_patches(torch.from_numpy(segs).to(DEV), POOL_P)
    gen = torch.Generator().manual_seed(1)
    emb = torch.round(torch.randn(3, N, D, generator=gen))
    Rt = max(len(g) for g in groups)
    gout = torch.randn(3, Rt, D, generator=gen)
    gout = gout + torch.sign(gout) * 0.25                       # no zero in go: a receiving patch is recognisable
    assert (gout != 0).all()
    got_o, got_d = _pool_device(K, emb, perm, offs, 1, Rt, gout)
    ref_o = R.pool_forward(emb.double(), groups, "max", Rt)
    assert torch.equal(got_o.double(), ref_o)
    tied = 0
    for b in range(3):
        for r, g in enumerate(groups[b]):
            e, d = emb[b, g], got_d[b, g]                       # [n, D]
            hit = d != 0
            assert (hit.sum(0) == 1).all(), (b, r, "one receiving patch per channel")
            assert torch.equal(d.sum(0), gout[b, r]), (b, r, "it receives go[d] unchanged")
            assert torch.equal((e * hit).sum(0), got_o[b, r] * hit.any(0)), (b, r, "the receiving patch holds the maximum")
            tied += int(((e == got_o[b, r]).sum(0) > 1).sum())
    assert tied > 1000


# ----------------------------------------------------------------------------------------------------------------
# SPPP: centroids
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [64, 50])
@pytest.mark.parametrize("S", [16, 64, 65, 196, 2048])
def test_centroids_across_the_privatisation_boundary(K, S, HW):
    """centroid_kernel: 16 privatised LDS tables up to S = 64, one above (65, 196), the limit 2048; HW = 50: the pixel
    count is no multiple of the 8192 a pass loads.  Labels >= S and negative labels are ignored, labels without pixels
    give 0.5.  The kernel sums integers exactly and divides once in double: at most 1 fp32 ulp from the float64 quotient."""
    rs = np.random.RandomState(S + HW)
    a = rs.randint(-3, S + 5, size=(HW, HW))
    b = 2 * rs.randint(0, max(1, S // 2), size=(HW, HW))                       # odd labels stay empty
    c = np.kron(rs.randint(0, S, size=((HW + 4) // 5, (HW + 4) // 5)), np.ones((5, 5), dtype=np.int64))[:HW, :HW]
    segs = np.stack([a, b, c]).astype(np.int64)
    ref = R.centroids_reference(segs, S)
    assert (segs[0] >= S).any() and (segs[0] < 0).any() and (ref[1, 1::2] == 0.5).all()
    got = K.sppp_centroids(torch.from_numpy(segs).to(DEV), S).cpu().numpy()
    assert got.shape == (3, S, 2) and got.dtype == np.float32
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= ulp).all(), (np.unravel_index(np.argmax(err / ulp), err.shape), (err / ulp).max())
    if S == 2048:
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            K.sppp_centroids(torch.from_numpy(segs).to(DEV), S + 1)


# ----------------------------------------------------------------------------------------------------------------
# SPPP: positional encoding
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prepend", [False, True])
@pytest.mark.parametrize("L", [5, 17, 197])
@pytest.mark.parametrize("D", [6, 64, 384])
def test_positional_encoding_both_forms(K, D, L, prepend):
    """favit_sppp_posenc_fwd with one centroid per token (n_cent = L) and with the class token at (0.5, 0.5) in front
    (n_cent = L - 1), different centroids per image, against float64.  Absolute bound: 4 x the worst error of the
    oracle's own fp32 dynamic_posenc against float64 on the same inputs, measured here per case (1.3e-7 .. 3.0e-7 over
    the eighteen cases: one rounding of |x + pe| < 8 plus the fp32 sine / exponential)."""
    gen = torch.Generator().manual_seed(100 * D + L)
    x = torch.randn(3, L, D, generator=gen)
    cent = torch.rand(3, L - 1 if prepend else L, 2, generator=gen)
    ref = R.posenc_reference(x, cent)
    measured = (O.dynamic_posenc(x, cent).double() - ref).abs().max().item()
    got = K.sppp_posenc_fwd(x.to(DEV), cent.to(DEV).contiguous()).cpu().double()
    err = (got - ref).abs().max().item()
    print(f"posenc D={D} L={L} prepend={prepend}: oracle fp32 {measured:.3e}, kernel {err:.3e}")
    assert err <= 4 * measured, (err, measured)


def test_positional_encoding_rejects_what_the_reference_rejects(K):
    x = torch.zeros(3, 5, 7, device=DEV)
    with pytest.raises(RuntimeError, match=INVALID):
        K.sppp_posenc_fwd(x, torch.zeros(3, 5, 2, device=DEV))              # odd D
    x = torch.zeros(3, 5, 8, device=DEV)
    for n in (3, 6):
        with pytest.raises(RuntimeError, match=INVALID):
            K.sppp_posenc_fwd(x, torch.zeros(3, n, 2, device=DEV))          # n_cent outside {L, L - 1}


# ----------------------------------------------------------------------------------------------------------------
# the model with max and attention pooling
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", ["max", "attention"])
def test_sppp_model_with_max_and_attention_pooling(favit, kname):
    """SPPPViTMHLA (embed_dim 64, depth 1, B = 3, three different maps of four superpixels) in fp32 mode: logits and
    every parameter gradient against O.sppp_vit_mhla_forward and its autograd, rel_l2 < 1e-3 as in
    test_gpu_modules.test_sppp_model_logits."""
    favit.set_compute_dtype("fp32")
    torch.manual_seed(31)
    S = 64
    m = favit.models.sppp_mhla.SPPPViTMHLA(img_size=S, patch_size=8, num_classes=10, embed_dim=64, depth=1, num_heads=4,
                                          num_superpixels=4, pooling_type=kname, window_size=3, use_mhla=True).to(DEV).eval()
    ar = torch.arange(S)
    quad = (ar[:, None] >= S // 2).long() * 2 + (ar[None, :] >= S // 2).long()
    other = (ar[:, None] >= S // 4).long() * 2 + (ar[None, :] >= 3 * S // 4).long()
    diag = (ar[:, None] + ar[None, :] >= S).long() * 2 + (ar[:, None] >= ar[None, :]).long()
    maps = torch.stack([quad, other, diag]).contiguous()
    x = torch.randn(3, 3, S, S)
    gout = torch.randn(3, 10)
    m.segmentation.set_label_maps(maps.to(DEV))
    try:
        y = m(x.to(DEV))
        (y * gout.to(DEV)).sum().backward()
    finally:
        m.segmentation.set_label_maps(None)
    sd = {k: v.detach().float().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = O.sppp_vit_mhla_forward(x, maps.numpy(), sd, 8, 4, 3, True, S=4, kind=kname)
    (want * gout).sum().backward()
    assert rel_l2(y, want) < 1e-3
    for k, p in m.named_parameters():
        ref = sd[k].grad
        assert ref is not None and p.grad is not None, k
        assert ref.abs().max().item() > 1e-6, k
        assert rel_l2(p.grad, ref) < 1e-3, (k, rel_l2(p.grad, ref))
