"""Float64 references and crafted label maps for the superpixel front end (csrc/slic.hip stage 3, csrc/sppp.hip).

The pooling, centroid and positional-encoding kernels are compared with plain float64 restatements written here (the
golden-checked oracle works in fp32 and per image; these are batched, take the grouping as (perm, offs) the way the
kernels do, and know about empty and dropped groups).  The label maps are built so that a given branch of the
connectivity kernels must run: rows wider than one 256-pixel chunk, runs that cross a chunk border, exactly
2048 / 2049 components, one component that winds through the whole image.

numpy / torch only; runs on the CPU.  tests/test_superpixel_refs_host.py ties this module to the oracle;
tests/test_gpu_superpixel_front_end.py leans on it."""
import math

import numpy as np
import torch

POOL_KINDS = ("mean", "max", "attention")          # the kernel's kind = the index here (include/favit.h)
SLIC_MAXC = 2048                                   # components per image that favit_slic_connect relabels
CC_CHUNK = 256                                     # pixels of a row that cc_runs_kernel scans at a time


# ----------------------------------------------------------------------------------------------------------------
# grouping
# ----------------------------------------------------------------------------------------------------------------
def groups_of_mapping(mapping):
    """oracle.favit_oracle.map_patches' dict -> [[patch, ...], ...] in token order."""
    return [list(v) for v in mapping.values()]


def groups_of_perm_offs(perm, offs):
    """One image's (perm [N], offs [N+1]) -> every non-empty group in token order."""
    perm, offs = np.asarray(perm).tolist(), np.asarray(offs).tolist()
    out = []
    for r in range(len(offs) - 1):
        if offs[r + 1] > offs[r]:
            out.append(perm[offs[r]:offs[r + 1]])
    return out


def mapping_tensors(mapping, N):
    """What favit_sppp_map_patches must return for one image whose oracle mapping is `mapping`:
    (dom [N], rank [N], perm [N], offs [N+1], n_tokens).  Groups in first-appearance order, raster order inside a
    group, offs[r] = N for every r past the last group."""
    dom = np.zeros(N, dtype=np.int64)
    rank = np.full(N, -1, dtype=np.int64)
    perm, offs = [], [0]
    for r, (label, idx) in enumerate(mapping.items()):
        assert list(idx) == sorted(idx)
        dom[idx] = label
        rank[idx] = r
        perm += list(idx)
        offs.append(len(perm))
    assert len(perm) == N and (rank >= 0).all()
    offs += [N] * (N + 1 - len(offs))
    return dom, rank, np.asarray(perm, dtype=np.int64), np.asarray(offs, dtype=np.int64), len(mapping)


# ----------------------------------------------------------------------------------------------------------------
# pooling
# ----------------------------------------------------------------------------------------------------------------
def pool_forward(emb, groups, kind, R):
    """emb [B, N, D] (any float dtype; float64 for the reference), groups[b] = that image's groups in token order.
    Returns [B, R, D]: token r of image b pools groups[b][r]; a token past the image's last group is a zero row and a
    group past R is dropped (what the kernels do for offs[r] == offs[r + 1] and for a grid of R tokens)."""
    B, _, D = emb.shape
    rows = []
    for b in range(B):
        for r in range(R):
            if r >= len(groups[b]):
                rows.append(emb.new_zeros(D))
                continue
            e = emb[b, groups[b][r], :]
            if kind == "mean":
                rows.append(e.sum(dim=0) / e.shape[0])
            elif kind == "max":
                rows.append(e.max(dim=0)[0])
            elif kind == "attention":
                s = e.sum(dim=-1)
                w = torch.exp(s - s.max())
                rows.append(((w / w.sum())[:, None] * e).sum(dim=0))
            else:
                raise ValueError(kind)
    return torch.stack(rows).reshape(B, R, D)


def pool_reference(emb, groups, kind, R, gout):
    """float64 forward and backward (autograd over pool_forward): (out [B, R, D], demb [B, N, D])."""
    e = emb.detach().double().clone().requires_grad_(True)
    out = pool_forward(e, groups, kind, R)
    out.backward(gout.double())
    return out.detach(), e.grad


def row_errors(got, ref):
    """Per-row relative error ||got - ref|| / (||ref|| + 1e-3 * mean row norm of ref) over the last axis, float64."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    n = ref.norm(dim=-1)
    return (got - ref).norm(dim=-1) / (n + 1e-3 * n.mean())


# ----------------------------------------------------------------------------------------------------------------
# centroids, positional encoding
# ----------------------------------------------------------------------------------------------------------------
def centroids_reference(segmaps, S):
    """segmaps int64 [B, H, W] -> float64 [B, S, 2] (x, y): per label 0 <= s < S exact integer sums of the pixel
    coordinates, then ONE float64 division by (extent * count); a label without pixels gets (0.5, 0.5)."""
    segmaps = np.asarray(segmaps, dtype=np.int64)
    B, H, W = segmaps.shape
    yy, xx = np.divmod(np.arange(H * W, dtype=np.int64), W)
    out = np.full((B, S, 2), 0.5, dtype=np.float64)
    for b in range(B):
        lab = segmaps[b].reshape(-1)
        ok = (lab >= 0) & (lab < S)
        cnt = np.zeros(S, dtype=np.int64)
        sx = np.zeros(S, dtype=np.int64)
        sy = np.zeros(S, dtype=np.int64)
        np.add.at(cnt, lab[ok], 1)
        np.add.at(sx, lab[ok], xx[ok])
        np.add.at(sy, lab[ok], yy[ok])
        has = cnt > 0
        out[b, has, 0] = sx[has].astype(np.float64) / (float(W) * cnt[has].astype(np.float64))
        out[b, has, 1] = sy[has].astype(np.float64) / (float(H) * cnt[has].astype(np.float64))
    return out


def posenc_reference(x, cent):
    """float64 restatement of favit_sppp_posenc_fwd.  x [B, L, D]; cent [B, n, 2] with n == L (one centroid per token)
    or n == L - 1 (token 0 is the class token and sits at (0.5, 0.5)): first half of the channels sin(cx * f_i), second
    half cos(cy * f_i), f_i = 10000^(-i / (D/2)).  cent = None: the index sinusoid (sin on even, cos on odd channels)."""
    x = torch.as_tensor(x).double()
    B, L, D = x.shape
    if cent is None:
        pos = torch.arange(L, dtype=torch.float64)[:, None]
        div = torch.exp(torch.arange(0, D, 2, dtype=torch.float64) * (-math.log(10000.0) / D))
        pe = torch.zeros(L, D, dtype=torch.float64)
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        return x + pe[None]
    c = torch.as_tensor(cent).double()
    if c.shape[1] == L - 1:
        c = torch.cat([torch.full((B, 1, 2), 0.5, dtype=torch.float64), c], dim=1)
    assert c.shape[1] == L
    half = D // 2
    f = torch.exp(torch.arange(half, dtype=torch.float64) * (-math.log(10000.0) / half))
    return x + torch.cat([torch.sin(c[:, :, 0:1] * f), torch.cos(c[:, :, 1:2] * f)], dim=-1)


# ----------------------------------------------------------------------------------------------------------------
# crafted cluster maps for the connectivity stage (uint8 [H, W])
# ----------------------------------------------------------------------------------------------------------------
BOARD_H, BOARD_W, CELL_H, CELL_W = 96, 320, 3, 5


def checkerboard(extra=False):
    """96 x 320, cells 3 tall x 5 wide of labels 0 / 1: 32 x 64 = 2048 components, exactly what stage 3 holds.  The
    chunk border at x = 256 falls inside a cell (256 = 51 * 5 + 1), so the cell's rows are runs that cross it.
    extra: the centre pixel of one cell (the one the chunk border cuts) becomes label 2 -- the rest of the cell is a
    ring and stays one component -- which makes 2049."""
    yy, xx = np.mgrid[0:BOARD_H, 0:BOARD_W]
    lab = ((yy // CELL_H + xx // CELL_W) % 2).astype(np.uint8)
    if extra:
        cy, cx = 16 * CELL_H + CELL_H // 2, (CC_CHUNK // CELL_W) * CELL_W + CELL_W // 2
        lab[cy, cx] = 2
    return lab


def serpentine(H, W):
    """Even rows: label 0 over the full width.  Odd rows: label 1 but for one label-0 pixel, at the right end after
    rows 0, 4, 8, ... and at the left end after rows 2, 6, ...: label 0 is ONE component that winds through the image
    (root = pixel 0, every row hangs off the one above through a single pixel: deep union chains), every odd row is a
    component of its own of W - 1 pixels."""
    lab = np.zeros((H, W), dtype=np.uint8)
    for y in range(1, H, 2):
        lab[y, :] = 1
        lab[y, W - 1 if (y // 2) % 2 == 0 else 0] = 0
    return lab


def stripes(H, W):
    """Top half: horizontal bands two rows tall (full-width runs: every chunk border of a wide row lies inside one);
    bottom half: diagonal bands seven pixels wide of three labels (runs start at a different x in every row)."""
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.where(yy < H // 2, (yy // 2) % 2, 2 + ((xx + yy) // 7) % 3)
    return lab.astype(np.uint8)


def noise(H, W, seed, cell=(2, 3), n_labels=3):
    """Blocky noise: cells of `cell` pixels with a random label each (many components of 6, 12, ... pixels, some
    below and some above any min_size in use, touching in every way)."""
    rs = np.random.RandomState(seed)
    ch, cw = cell
    base = rs.randint(0, n_labels, size=((H + ch - 1) // ch, (W + cw - 1) // cw))
    return np.kron(base, np.ones((ch, cw), dtype=np.int64))[:H, :W].astype(np.uint8)


CRAFTED_H = 40
CRAFTED_WIDTHS = (257, 300, 520)       # one chunk border with a last chunk of ONE pixel; one border; two borders


def crafted_batch(W):
    """The three maps of one width, one per image of a batch: stripes, noise, serpentine."""
    return np.stack([stripes(CRAFTED_H, W), noise(CRAFTED_H, W, seed=W), serpentine(CRAFTED_H, W)])


# ----------------------------------------------------------------------------------------------------------------
# SLIC inputs
# ----------------------------------------------------------------------------------------------------------------
def smooth_image(H, W, seed):
    """Soft colour gradients: a 6 x 6 random colour field upsampled bicubically (as in tests/test_slic.py)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 3, 6, 6, generator=g)
    return torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)[0].clamp(0, 1).numpy()


def features_f32(img, sigma):
    """oracle.slic_oracle.features (rescale=True) restated in float32 the way the device orders the work (blur along x,
    then along y, then the min-max rescale, then sRGB -> CIELAB): how far fp32 alone moves the quantised features."""
    f = np.float32
    img = np.asarray(img, dtype=f)
    _, H, W = img.shape
    lo, hi = img.min(), img.max()
    r = int(4.0 * sigma + 0.5) if sigma > 0 else 0
    if r > 0:
        k = np.exp(-0.5 * (np.arange(-r, r + 1) ** 2) / (sigma * sigma))
        k = (k / k.sum()).astype(f)

        def refl(i, n):
            while i < 0 or i >= n:
                i = -i - 1 if i < 0 else 2 * n - 1 - i
            return i
        ix = np.array([[refl(x + d, W) for d in range(-r, r + 1)] for x in range(W)])
        iy = np.array([[refl(y + d, H) for d in range(-r, r + 1)] for y in range(H)])
        tmp = np.zeros_like(img)
        for j in range(2 * r + 1):
            tmp = tmp + k[j] * img[:, :, ix[:, j]]
        img = np.zeros_like(tmp)
        for j in range(2 * r + 1):
            img = img + k[j] * tmp[:, iy[:, j], :]
    img = img - lo
    if hi != lo:
        img = img / (hi - lo)
    lin = np.where(img > f(0.04045), np.abs((img + f(0.055)) / f(1.055)) ** f(2.4), img / f(12.92)).astype(f)
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], dtype=f)
    xyz = np.einsum("ij,jyx->iyx", M, lin).astype(f) / np.array([0.95047, 1.0, 1.08883], dtype=f)[:, None, None]
    t = np.where(xyz > f(0.008856), np.cbrt(xyz), f(7.787) * xyz + f(16.0 / 116.0)).astype(f)
    lab = np.stack([f(116.0) * t[1] - f(16.0), f(500.0) * (t[0] - t[1]), f(200.0) * (t[1] - t[2])], -1)
    return np.clip(np.rint(lab * f(16.0)), -8191, 8191).astype(np.int16).reshape(H * W, 3)


# the stage tests of the GPU file: (H, W, n_segments, sigma, compactness or None = chosen from the step, image seed)
ODD_SIZES = ((37, 53, 12, 1.0, 1.0, 31), (50, 70, 16, 1.0, 1.0, 32), (41, 300, 9, 1.0, 1.0, 33))


def general_form_compactness(step):
    """A compactness whose coef = round((step / compactness)^2) lies just above 2^32 (the 64-bit assignment kernel)."""
    return step / (65536.0 * 1.001)


# ----------------------------------------------------------------------------------------------------------------
# label maps for the patch mapping (int64 [HW, HW])
# ----------------------------------------------------------------------------------------------------------------
MAP_KINDS = ("blocky", "distinct", "offset40", "high_bit_pairs", "negative")


def label_map(kind, HW, P, seed):
    rs = np.random.RandomState(seed)
    cell = int(rs.choice([1, 2, max(1, P // 2), P, 2 * P]))
    n = (HW + cell - 1) // cell
    blocky = np.kron(rs.randint(0, 12, size=(n, n)), np.ones((cell, cell), dtype=np.int64))[:HW, :HW].astype(np.int64)
    if kind == "blocky":
        return blocky
    if kind == "distinct":                 # every count is 1: the smallest label of the patch wins
        return rs.permutation(HW * HW).astype(np.int64).reshape(HW, HW)
    if kind == "offset40":
        return blocky + (1 << 40)
    if kind == "high_bit_pairs":           # l and l + 2^32 share their low word: counted together they outvote a third label
        low = rs.randint(0, 3, size=(HW, HW)).astype(np.int64)
        high = (rs.randint(0, 2, size=(HW, HW)).astype(np.int64) * (low < 2)) << 32
        return low + high
    if kind == "negative":
        return np.where(blocky % 3 == 0, -blocky - (1 << 33), blocky - 6)
    raise ValueError(kind)
