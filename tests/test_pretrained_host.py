"""Checkpoint import on the host (pretrained.convert_state_dict / load_pretrained): the torchvision, timm and both
Hugging Face key layouts converted and run through the float64 oracle against the source model's own logits, the
target names of every model family, the refusals (which leave the model untouched) and the project's own flat .npz."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _pretrained_ref as S
from oracle import favit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(img_size=S.IMG, patch_size=S.P, num_classes=S.CLASSES, embed_dim=S.D, depth=S.DEPTH, num_heads=S.H)


@pytest.fixture(scope="module")
def source():
    """(source model, its state dict, an input batch, its float64 logits): computed once, never modified."""
    m = S.source_model(seed=3)
    x = torch.randn(3, S.C, S.IMG, S.IMG, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        logits = m(x)
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}, x, logits


def _dense(favit, **over):
    return favit.models.vit.VisionTransformer(**{**KW, **over})


def _snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)


def test_torchvision_layout_reproduces_the_source_logits(favit, source):
    _, sd, x, logits = source
    model = _dense(favit)
    conv, rep = favit.pretrained.convert_state_dict(sd, model)
    assert rep["layout"] == "torchvision" and rep["source_grid"] == 4 and rep["model_grid"] == 4
    assert sorted(conv) == sorted(model.state_dict()) == rep["loaded"]
    assert not rep["skipped"] and not rep["unused"] and not rep["missing"]
    assert all(v.dtype == torch.float64 for v in conv.values())
    assert (O.vit_forward(x, conv, S.P, S.H) - logits).abs().max().item() < 1e-12
    # the test bites: the convolution weight flattened without the permutation is far off
    wrong = dict(conv)
    wrong["patch_embed.projection.1.weight"] = sd["conv_proj.weight"].reshape(S.D, -1)
    assert (O.vit_forward(x, wrong, S.P, S.H) - logits).abs().max().item() > 1e-3


def test_older_torchvision_mlp_names(favit):
    m = S.source_model(seed=5, old_mlp_names=True)
    assert any(".mlp.linear_1." in k for k in m.state_dict())
    x = torch.randn(2, S.C, S.IMG, S.IMG, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    conv, rep = favit.pretrained.convert_state_dict(m.state_dict(), _dense(favit))
    assert not rep["unused"] and not rep["missing"]
    with torch.no_grad():
        assert (O.vit_forward(x, conv, S.P, S.H) - m(x)).abs().max().item() < 1e-12


@pytest.mark.parametrize("layout", ["timm", "hf", "hf5", "hf_bare", "hf5_bare"])
def test_other_layouts_reproduce_the_source_logits(favit, source, layout):
    _, sd, x, logits = source
    if layout == "timm":
        src = S.as_timm(sd)
    else:
        src = S.as_hf(sd, in_memory=layout.startswith("hf5"), prefix="" if layout.endswith("_bare") else "vit.")
        src["vit.pooler.dense.weight"] = torch.zeros(S.D, S.D, dtype=torch.float64)
    assert not set(src) & set(sd)
    model = _dense(favit)
    conv, rep = favit.pretrained.convert_state_dict(src, model)
    assert rep["layout"] == layout.replace("_bare", "")
    assert sorted(conv) == sorted(model.state_dict()) and not rep["missing"] and not rep["skipped"]
    assert rep["unused"] == ([] if layout == "timm" else ["vit.pooler.dense.weight"])
    assert (O.vit_forward(x, conv, S.P, S.H) - logits).abs().max().item() < 1e-12
    ref, _ = favit.pretrained.convert_state_dict(sd, model)            # and bit for bit what the torchvision spelling gives
    assert _same(conv, ref)


def test_multihead_attention_containers_get_their_own_names(favit, source):
    _, sd, x, logits = source
    model = favit.models.vit_mhla.VisionTransformerMHLA(window_size=7, use_mhla=False, **KW)
    conv, rep = favit.pretrained.convert_state_dict(S.as_hf(sd, in_memory=False), model)
    for i in range(S.DEPTH):
        for leaf in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
            assert f"blocks.{i}.attn.{leaf}" in conv
    assert not any(".attn.qkv." in k or ".attn.proj." in k for k in conv) and not rep["missing"]
    assert (O.vit_mhla_forward(x, conv, S.P, S.H, 7, False) - logits).abs().max().item() < 1e-12


def test_mhla_targets_keep_latent_proj_and_take_sequential_mlp_names(favit, source):
    _, sd, _, _ = source
    model = favit.models.mhla_models.PretrainedViTWithMHLA(window_size=3, **KW)
    conv, rep = favit.pretrained.convert_state_dict(S.as_timm(sd), model)
    assert "blocks.1.mlp.0.weight" in conv and "blocks.1.mlp.3.bias" in conv and "blocks.0.attn.qkv.weight" in conv
    assert rep["missing"] == sorted(k for k in model.state_dict() if "latent_proj" in k) and len(rep["missing"]) == 2 * S.DEPTH
    before = _snapshot(model)
    rep = favit.pretrained.load_pretrained(model, sd)
    after = model.state_dict()
    assert rep["pos_embed"] == "copied"
    for k in after:
        if "latent_proj" in k:
            assert torch.equal(after[k], before[k])
        else:
            assert torch.equal(after[k], conv[k].to(after[k].dtype)), k


def test_hugging_face_directory_and_in_memory_keys_agree(favit, tmp_path):
    tr = pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    torch.manual_seed(7)
    cfg = tr.ViTConfig(hidden_size=S.D, num_hidden_layers=S.DEPTH, num_attention_heads=S.H, intermediate_size=4 * S.D,
                       image_size=S.IMG, patch_size=S.P, num_channels=S.C, layer_norm_eps=1e-5, num_labels=S.CLASSES,
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hf = tr.ViTForImageClassification(cfg).eval()
    with torch.no_grad():
        for p in hf.parameters():
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() > 1 else 0.5))
    hf.save_pretrained(str(tmp_path / "ckpt"))
    model = _dense(favit)
    on_disk, eps = favit.pretrained.read_state_dict(str(tmp_path / "ckpt"))
    assert eps == 1e-5
    a, ra = favit.pretrained.convert_state_dict(on_disk, model)
    b, rb = favit.pretrained.convert_state_dict(hf.state_dict(), model)
    assert sorted(a) == sorted(model.state_dict()) and _same(a, b)
    assert {ra["layout"], rb["layout"]} <= {"hf", "hf5"} and not ra["missing"] and not rb["missing"]
    x = torch.randn(2, S.C, S.IMG, S.IMG, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        want = hf.double()(x).logits
    assert (O.vit_forward(x, {k: v.double() for k, v in a.items()}, S.P, S.H) - want).abs().max().item() < 1e-12
    rep = favit.pretrained.load_pretrained(model, str(tmp_path / "ckpt"))
    assert rep["layer_norm_eps"] == 1e-5 and "1e-05" in rep.summary()
    assert _same(dict(model.state_dict()), {k: v.float() for k, v in a.items()})


@pytest.mark.parametrize("ext", [".pt", ".pth", ".bin", ".npz", ".safetensors"])
def test_file_formats(favit, source, tmp_path, ext):
    _, sd, _, _ = source
    path = str(tmp_path / ("ckpt" + ext))
    if ext == ".npz":
        np.savez(path, **{k: v.numpy() for k, v in sd.items()})
    elif ext == ".safetensors":
        pytest.importorskip("safetensors")
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, path)
    else:
        torch.save({"state_dict": sd} if ext == ".pth" else {"model": sd} if ext == ".bin" else sd, path)
    got, eps = favit.pretrained.read_state_dict(path)
    assert eps is None and _same(got, sd)
    with pytest.raises(ValueError, match="unknown checkpoint format"):
        favit.pretrained.read_state_dict(str(tmp_path / "ckpt.h5"))


@pytest.mark.parametrize("over,named", [
    ({"patch_size": 8}, r"patch_embed\.projection\.1\.weight.*\(32, 3, 4, 4\).*\(32, 192\)"),
    ({"embed_dim": 64}, r"\(32, 3, 4, 4\).*\(64, 48\)"),
    ({"depth": 3}, r"depth differs: the source has 2 blocks.*the model 3"),
])
def test_another_patch_size_width_or_depth_is_refused(favit, source, over, named):
    _, sd, _, _ = source
    model = _dense(favit, **over)
    before = _snapshot(model)
    with pytest.raises(ValueError, match=named):
        favit.pretrained.load_pretrained(model, sd)
    assert _same(before, dict(model.state_dict()))


def test_width_mismatch_names_key_and_shapes_without_a_patch_weight(favit, source):
    _, sd, _, _ = source
    src = {k: v for k, v in S.as_timm(sd).items() if not k.startswith("patch_embed.")}
    src["patch_embed.proj.weight"] = S.as_timm(sd)["patch_embed.proj.weight"]
    src["blocks.0.norm1.weight"] = torch.ones(48, dtype=torch.float64)
    model = _dense(favit)
    before = _snapshot(model)
    with pytest.raises(ValueError, match=r"blocks\.0\.norm1\.weight.*\(48,\).*\(32,\)"):
        favit.pretrained.load_pretrained(model, src)
    assert _same(before, dict(model.state_dict()))


def test_pos_embed_refusals_and_unknown_layout(favit, source):
    _, sd, _, _ = source
    model = _dense(favit, img_size=32)                         # an 8 x 8 grid against the source's 4 x 4
    before = _snapshot(model)
    with pytest.raises(ValueError, match=r"pos_embed.*4x4.*8x8.*strict"):
        favit.pretrained.load_pretrained(model, sd, pos_embed="strict")
    assert _same(before, dict(model.state_dict()))
    odd = dict(sd)
    odd["encoder.pos_embedding"] = torch.zeros(1, 16, S.D, dtype=torch.float64)       # 15 grid rows
    with pytest.raises(ValueError, match=r"pos_embed.*16 rows.*square grid"):
        favit.pretrained.load_pretrained(model, odd)
    assert _same(before, dict(model.state_dict()))
    with pytest.raises(ValueError, match="unknown checkpoint layout"):
        favit.pretrained.load_pretrained(model, {"backbone.stem.weight": torch.zeros(3), "fc.bias": torch.zeros(2)})
    with pytest.raises(ValueError, match="not a state dict"):
        favit.pretrained.load_pretrained(model, {"epoch": 3})
    with pytest.raises(ValueError, match="'resample' or 'strict'"):
        favit.pretrained.load_pretrained(model, sd, pos_embed="bilinear")
    assert _same(before, dict(model.state_dict()))


def test_a_head_of_another_shape_is_skipped_and_reported(favit, source):
    _, sd, _, _ = source
    model = _dense(favit, num_classes=7)
    before = _snapshot(model)
    rep = favit.pretrained.load_pretrained(model, sd)
    after = model.state_dict()
    assert set(rep["skipped"]) == {"head.weight", "head.bias"} and "(5, 32)" in rep["skipped"]["head.weight"]
    assert "head.weight" not in rep["loaded"] and "head.weight" not in rep["missing"]
    assert torch.equal(after["head.weight"], before["head.weight"]) and torch.equal(after["head.bias"], before["head.bias"])
    assert torch.equal(after["norm.weight"], sd["encoder.ln.weight"].float())
    assert "skipped head.weight" in rep.summary()


def test_flat_npz_in_the_projects_own_keys_loads_what_load_flat_weights_loads(favit, tmp_path):
    spec = importlib.util.spec_from_file_location("favit_run_experiment_pretrained",
                                                  os.path.join(ROOT, "tools", "run_experiment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    torch.manual_seed(9)
    donor = favit.models.vit_mhla.VisionTransformerMHLA(window_size=7, use_mhla=True, **KW)
    keep = [k for k in donor.state_dict() if "latent_proj" not in k and not k.startswith("head.")]
    path = str(tmp_path / "flat.npz")
    np.savez(path, not_a_model_key=np.zeros(3, np.float32), **{k: donor.state_dict()[k].numpy() for k in keep})

    def fresh():
        torch.manual_seed(10)
        return favit.models.vit_mhla.VisionTransformerMHLA(window_size=7, use_mhla=True, **KW)
    a, b = fresh(), fresh()
    loaded = []
    sd = a.state_dict()                                        # what load_flat_weights did before this module existed
    with np.load(path, allow_pickle=False) as arc:
        for k in arc.files:
            if k in sd:
                with torch.no_grad():
                    sd[k].copy_(torch.from_numpy(arc[k]))
                loaded.append(k)
    rep = favit.pretrained.load_pretrained(b, path)
    assert rep["layout"] == "native" and rep["loaded"] == sorted(loaded) == sorted(keep)
    assert rep["unused"] == ["not_a_model_key"] and _same(dict(a.state_dict()), dict(b.state_dict()))
    c = fresh()
    assert sorted(tool.load_flat_weights(c, path)) == sorted(keep) and _same(dict(a.state_dict()), dict(c.state_dict()))
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, **{"norm.weight": np.zeros(7, np.float32)})
    with pytest.raises(ValueError, match=r"norm\.weight.*\(7,\).*\(32,\)"):
        tool.load_flat_weights(c, bad)
