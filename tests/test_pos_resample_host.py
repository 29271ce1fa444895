"""functional.pos_resample_matrix and the tables made of it, on the host: the matrix against torch's own bicubic
interpolation in float64 for both antialias modes, the identity for equal grids, rows that sum to one, and the
compressed-row tables (the matrix's and its transpose's) against the dense fp32 matrix."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

PAIRS = [(14, 24), (14, 10), (3, 5), (5, 3), (1, 4), (4, 1), (2, 2), (7, 7), (24, 14), (14, 37)]


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("g_in,g_out", PAIRS)
def test_matrix_is_torchs_bicubic(favit, g_in, g_out, antialias):
    M = favit.functional.pos_resample_matrix(g_in, g_out, antialias)
    assert M.dtype == torch.float64 and tuple(M.shape) == (g_out, g_in)
    x = torch.randn(2, 3, g_in, g_in, dtype=torch.float64, generator=torch.Generator().manual_seed(g_in * 100 + g_out))
    ref = TF.interpolate(x, size=(g_out, g_out), mode="bicubic", align_corners=False, antialias=antialias)
    got = torch.einsum("ai,bj,ncij->ncab", M, M, x)
    assert (got - ref).abs().max().item() < 1e-12
    assert (M.sum(dim=1) - 1.0).abs().max().item() < 1e-12
    if g_in == g_out:
        assert torch.equal(M, torch.eye(g_in, dtype=torch.float64))
    taps = int((M != 0).sum(dim=1).max())
    assert taps <= (int(np.ceil(4 * max(g_in / g_out, 1.0))) + 1 if antialias else 4)
    assert M.abs().sum(dim=1).max().item() <= 1.375 + 1e-12


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("g_in,g_out", [(14, 24), (24, 14), (1, 4), (4, 1), (7, 7), (30, 3)])
def test_compressed_rows_hold_the_fp32_matrix_and_its_transpose(favit, g_in, g_out, antialias):
    K = favit.kernels
    M32 = K.pos_resample_matrix(g_in, g_out, antialias).numpy().astype(np.float32)
    for mat in (M32, np.ascontiguousarray(M32.T)):
        rowptr, cols, vals = K._csr(mat)
        assert rowptr.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.float32
        assert rowptr[0] == 0 and rowptr[-1] == len(cols) == len(vals) and len(rowptr) == mat.shape[0] + 1
        dense = np.zeros_like(mat)
        for r in range(mat.shape[0]):
            c = cols[rowptr[r]:rowptr[r + 1]]
            assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 0 and c[-1] < mat.shape[1]))
            assert np.all(vals[rowptr[r]:rowptr[r + 1]] != 0)
            dense[r, c] = vals[rowptr[r]:rowptr[r + 1]]
        assert np.array_equal(dense, mat)


def test_bad_sides_are_refused(favit):
    with pytest.raises(ValueError, match="grid sides"):
        favit.functional.pos_resample_matrix(0, 4, True)
    with pytest.raises(ValueError, match="not a square grid"):
        favit.functional.pos_resample(torch.zeros(1, 16, 8), 4)


def test_models_carry_a_plain_antialias_switch(favit):
    M = favit.models
    kw = dict(img_size=16, patch_size=4, num_classes=5, embed_dim=32, depth=1, num_heads=4)
    for m in (M.vit.VisionTransformer(**kw), M.vit_mhla.VisionTransformerMHLA(window_size=7, use_mhla=True, **kw),
              M.mhla_models.PretrainedViTWithMHLA(window_size=3, **kw)):
        assert m.pos_antialias is True
        keys = set(m.state_dict())
        assert m.set_pos_antialias(False) is m and m.pos_antialias is False
        assert set(m.state_dict()) == keys and not any("antialias" in k for k in keys)
        assert not any("antialias" in n for n, _ in list(m.named_parameters()) + list(m.named_buffers()))
