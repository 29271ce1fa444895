"""The mean-pooled head on the host: set_global_pool on every model class (validation, defaults, no new state), the
closed-form backward the kernels compute against float64 autograd of the reference, and the importer's fc_norm rule."""
import pytest
import torch

import _head_pool_ref as R
import _pretrained_ref as S

SMALL = dict(img_size=16, patch_size=4, num_classes=5, embed_dim=32, depth=2, num_heads=2)


def _models(favit):
    M = favit.models
    sp = dict(num_superpixels=4)
    return [
        M.vit.VisionTransformer(**SMALL),
        M.vit_mhla.VisionTransformerMHLA(window_size=3, use_mhla=True, **SMALL),
        M.mhla_models.PretrainedViTWithMHLA(window_size=3, **SMALL),
        M.mhla_models.PretrainedSPPPViTWithMHLA(window_size=3, **sp, **SMALL),
        M.sppp.SPPPViT(**sp, **SMALL),
        M.sppp_mhla.SPPPViTMHLA(window_size=3, use_mhla=True, **sp, **SMALL),
        M.attention.CrossAttentionViT(**SMALL),
        M.attention.CrossAttentionSPPPViT(**sp, **SMALL),
    ]


@pytest.fixture(scope="module")
def models(favit):
    return _models(favit)


def test_every_model_class_has_the_method_and_the_token_default(favit, models):
    assert len({type(m) for m in models}) == 8
    for m in models:
        assert (m.global_pool, m.pool_norm) == ("token", "before"), type(m).__name__
        assert type(m).set_global_pool is favit.models.vit.set_global_pool


def test_set_global_pool_validates_and_returns_the_model(favit, models):
    m = models[0]
    for pool, norm in (("max", "before"), ("avg", "both"), ("cls", "after"), (None, "before"), ("avg", None)):
        with pytest.raises(ValueError):
            m.set_global_pool(pool, norm)
        assert (m.global_pool, m.pool_norm) == ("token", "before"), "a refused call changes nothing"
    assert m.set_global_pool("avg", "after") is m and (m.global_pool, m.pool_norm) == ("avg", "after")
    assert m.set_global_pool("avg") is m and (m.global_pool, m.pool_norm) == ("avg", "before")
    assert m.set_global_pool() is m and (m.global_pool, m.pool_norm) == ("token", "before")
    assert favit.models.vit.set_global_pool(m, "avg").global_pool == "avg"
    m.set_global_pool()


def test_pooling_adds_no_parameter_buffer_or_state_dict_key(models):
    for m in models:
        keys, n_par, n_buf = list(m.state_dict()), sum(p.numel() for p in m.parameters()), len(list(m.buffers()))
        names = [k for k, _ in m.named_parameters()]
        for pool, norm in (("avg", "before"), ("avg", "after"), ("token", "before")):
            m.set_global_pool(pool, norm)
            assert list(m.state_dict()) == keys, type(m).__name__
            assert sum(p.numel() for p in m.parameters()) == n_par and len(list(m.buffers())) == n_buf
            assert [k for k, _ in m.named_parameters()] == names
        assert not any("pool" in k for k in keys)


@pytest.mark.parametrize("norm_first", [True, False])
@pytest.mark.parametrize("B,L,D,first", [(3, 9, 16, 1), (2, 2, 8, 1), (2, 7, 12, 0), (2, 6, 8, 2)])
def test_closed_form_backward_matches_float64_autograd(norm_first, B, L, D, first):
    g = torch.Generator().manual_seed(B * 100 + L)
    x = torch.randn(B, L, D, dtype=torch.float64, generator=g) * 1.7 + 0.3
    gamma = 1 + 0.2 * torch.randn(D, dtype=torch.float64, generator=g)
    beta = 0.3 * torch.randn(D, dtype=torch.float64, generator=g)
    dy = torch.randn(B, D, dtype=torch.float64, generator=g)
    _, dx, dg, db = R.head_pool_grads(x, gamma, beta, dy, norm_first, first)
    cdx, cdg, cdb = R.closed_form_backward(x, gamma, dy, norm_first, first)
    assert (cdx - dx).abs().max().item() < 1e-12
    assert (cdg - dg).abs().max().item() < 1e-12 and (cdb - db).abs().max().item() < 1e-12
    assert torch.equal(cdx[:, :first], torch.zeros(B, first, D, dtype=torch.float64))
    assert torch.equal(dx[:, :first], torch.zeros(B, first, D, dtype=torch.float64)), "the head does not read these rows"
    if norm_first:       # dgamma = sum_b dy[b] * s[b]: the affine map commutes with the mean
        xh = torch.nn.functional.layer_norm(x[:, first:], (D,))
        assert ((dy * xh.mean(1)).sum(0) - dg).abs().max().item() < 1e-12
        y = R.head_pool(x, gamma, beta, True, first)
        assert (gamma * xh.mean(1) + beta - y).abs().max().item() < 1e-12


# ---- importer ---------------------------------------------------------------------------------------------------

KW = dict(img_size=S.IMG, patch_size=S.P, num_classes=S.CLASSES, embed_dim=S.D, depth=S.DEPTH, num_heads=S.H)


@pytest.fixture(scope="module")
def timm_sd():
    sd = S.as_timm({k: v.detach().clone() for k, v in S.source_model(seed=11).state_dict().items()})
    assert "norm.weight" in sd and "norm.bias" in sd and "patch_embed.proj.weight" in sd
    return sd


def _fresh(favit):
    return favit.models.vit.VisionTransformer(**KW)


def test_fc_norm_loads_into_norm_and_hints_avg_after(favit, timm_sd):
    src = dict(timm_sd)
    src["fc_norm.weight"], src["fc_norm.bias"] = src.pop("norm.weight") * 1.5, src.pop("norm.bias") + 0.25
    model = _fresh(favit)
    rep = favit.pretrained.load_pretrained(model, src)
    assert rep["pool_hint"] == ("avg", "after")
    assert "norm.weight" in rep["loaded"] and "norm.bias" in rep["loaded"]
    assert not rep["unused"] and not rep["missing"]
    assert torch.equal(model.norm.weight.detach().double(), src["fc_norm.weight"].double().float().double())
    assert torch.equal(model.norm.bias.detach().double(), src["fc_norm.bias"].double().float().double())
    assert (model.global_pool, model.pool_norm) == ("token", "before"), "loading never changes the model's pooling"
    assert "fc_norm" in rep.summary() and "'avg', 'after'" in rep.summary()


def test_norm_wins_over_fc_norm(favit, timm_sd):
    src = dict(timm_sd)
    src["fc_norm.weight"], src["fc_norm.bias"] = src["norm.weight"] * 3.0, src["norm.bias"] - 1.0
    model = _fresh(favit)
    rep = favit.pretrained.load_pretrained(model, src)
    assert rep["pool_hint"] is None
    assert torch.equal(model.norm.weight.detach(), src["norm.weight"].float())
    assert torch.equal(model.norm.bias.detach(), src["norm.bias"].float())
    assert len(rep["unused"]) == 2
    for leaf in ("weight", "bias"):
        line = [u for u in rep["unused"] if u.startswith(f"fc_norm.{leaf}")]
        assert len(line) == 1 and "norm.*" in line[0], rep["unused"]


def test_plain_norm_gives_no_hint(favit, timm_sd):
    rep = favit.pretrained.load_pretrained(_fresh(favit), dict(timm_sd))
    assert rep["pool_hint"] is None and not rep["unused"]
    assert "fc_norm" not in rep.summary()
    conv, rep2 = favit.pretrained.convert_state_dict(dict(timm_sd), _fresh(favit))
    assert rep2["pool_hint"] is None


def test_a_refused_fc_norm_load_leaves_the_model_untouched(favit, timm_sd):
    src = dict(timm_sd)
    src.pop("norm.weight"), src.pop("norm.bias")
    src["fc_norm.weight"], src["fc_norm.bias"] = torch.ones(S.D + 1), torch.zeros(S.D + 1)
    model = _fresh(favit)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with pytest.raises(ValueError, match="norm.weight"):
        favit.pretrained.load_pretrained(model, src)
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
