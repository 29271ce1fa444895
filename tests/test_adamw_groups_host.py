"""Host-side tests of the fine-tuning parameter groups (train.param_groups: layer-wise learning-rate decay, weight-decay
exemptions), of the one-arena layout of train.FusedAdamW(fuse_groups=True) and of the segmented AdamW entry point's
declarations.  Nothing here launches a kernel."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch


def _vit(favit, seed=3):
    torch.manual_seed(seed)
    return favit.models.vit_mhla.VisionTransformerMHLA(img_size=32, patch_size=4, embed_dim=64, depth=2, num_heads=4,
                                                       use_mhla=True)


def _pairs(groups, model):
    """{name: (rate, weight decay or None)} from a group list."""
    names = {id(p): n for n, p in model.named_parameters()}
    return {names[id(p)]: (g["lr"], g.get("weight_decay")) for g in groups for p in g["params"]}


def _layer_id(name, depth):
    m = re.match(r"^blocks\.(\d+)\.", name)
    if m:
        return int(m.group(1)) + 1
    if "head" in name or name.startswith("norm."):
        return depth + 1
    return 0


def test_default_arguments_give_the_three_name_based_groups(favit):
    model = _vit(favit)
    dict(model.named_parameters())["patch_embed.projection.1.bias"].requires_grad_(False)      # (frozen: skipped)
    base, lat, head = [], [], []
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (head if "head" in n else lat if "latent_proj" in n else base).append(p)
    want = [g for g in ({"params": base, "lr": 1e-4}, {"params": lat, "lr": 1e-4 * 5.0}, {"params": head, "lr": 1e-3})
            if g["params"]]
    got = favit.train.param_groups(model, lr=1e-4, head_lr=1e-3)
    assert [sorted(g) for g in got] == [sorted(g) for g in want]
    for a, b in zip(got, want):
        assert a["lr"] == b["lr"] and [id(p) for p in a["params"]] == [id(p) for p in b["params"]]
    assert len(got) == 3


def test_layer_decay_and_exemptions_follow_the_formula(favit):
    model = _vit(favit)
    model.blocks[0].norm1.weight.requires_grad_(False)
    d, lr, head_lr, depth = 0.5, 1e-4, 1e-3, 2
    groups = favit.train.param_groups(model, lr=lr, head_lr=head_lr, layer_decay=d, no_weight_decay="auto")
    got = _pairs(groups, model)
    want = {}
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        cat = head_lr if "head" in n else lr * 5.0 if "latent_proj" in n else lr
        exempt = p.ndim <= 1 or n.split(".")[-1] in ("cls_token", "pos_embed")
        want[n] = (cat * d ** (depth + 1 - _layer_id(n, depth)), 0.0 if exempt else None)
    assert got == want
    assert "blocks.0.norm1.weight" not in got
    # the examples of the recipe, spelled out
    assert got["blocks.0.mlp.fc1.weight"] == (pytest.approx(2.5e-5, rel=1e-12), None)
    lat_bias = [n for n in got if n.startswith("blocks.1.") and n.endswith("latent_proj.bias")]
    assert lat_bias and all(got[n] == (pytest.approx(2.5e-4, rel=1e-12), 0.0) for n in lat_bias)
    assert got["head.weight"] == (pytest.approx(1e-3, rel=1e-12), None)
    assert got["pos_embed"] == (pytest.approx(1.25e-5, rel=1e-12), 0.0)
    # no (rate, weight decay) pair twice; exempt groups carry the key, the others do not
    keys = [(g["lr"], g.get("weight_decay")) for g in groups]
    assert len(set(keys)) == len(keys)
    assert all(g.get("weight_decay", 0.0) == 0.0 for g in groups)
    # descending layer order
    names = {id(p): n for n, p in model.named_parameters()}
    tops = [max(_layer_id(names[id(p)], depth) for p in g["params"]) for g in groups]
    assert tops == sorted(tops, reverse=True) and tops[0] == depth + 1 and tops[-1] == 0


def test_exemption_by_name_and_alone(favit):
    model = _vit(favit)
    groups = favit.train.param_groups(model, lr=1e-4, head_lr=1e-3, no_weight_decay=["bias", "pos_embed"])
    for n, (rate, wd) in _pairs(groups, model).items():
        assert wd == (0.0 if ("bias" in n or "pos_embed" in n) else None), n
        assert rate == (1e-3 if "head" in n else 5e-4 if "latent_proj" in n else 1e-4)
    with pytest.raises(ValueError):
        favit.train.param_groups(model, lr=1e-4, no_weight_decay="norm")
    with pytest.raises(ValueError):
        favit.train.param_groups(model, lr=1e-4, layer_decay=1.5)


def test_layer_decay_needs_blocks(favit):
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    with pytest.raises(ValueError, match="blocks"):
        favit.train.param_groups(model, lr=1e-4, layer_decay=0.5)
    assert favit.train.param_groups(model, lr=1e-4, no_weight_decay="auto")      # exemptions alone need none


def _recipe(favit, model, d=0.75):
    return favit.train.param_groups(model, lr=1e-4, head_lr=1e-3, layer_decay=d, no_weight_decay="auto")


def test_fused_layout_on_cpu_parameters(favit):
    T, K = favit.train, favit.kernels
    model = _vit(favit)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    groups = _recipe(favit, model)
    assert len(groups) > 3
    opt = T.FusedAdamW(groups, lr=1e-4, weight_decay=0.05, distributed=False, fuse_groups=True)
    align = K.ADAMW_SEG_ALIGN
    assert align == 256 and K.ADAMW_MAX_SEGMENTS == 64
    arena_p, arena_g = opt._arena["p"], opt._arena["g"]
    at = 0
    for g, src in zip(opt.groups, groups):
        f = g["flat"]
        start = (f.flat_p.data_ptr() - arena_p.data_ptr()) // 4
        assert start == at and start % align == 0 and f.numel % align == 0
        assert f.numel - favit.dp.FlatBuffers.size_of(src["params"]) < align
        assert (f.flat_g.data_ptr() - arena_g.data_ptr()) // 4 == start
        for key in ("m", "v"):
            assert g[key].numel() == f.numel and (g[key].data_ptr() - opt._arena[key].data_ptr()) // 4 == start
        assert f.params == [p for p in reversed(src["params"])]           # reverse registration order, as per group
        assert all(o % 4 == 0 for o in f.offsets)
        for p, o in zip(f.params, f.offsets):
            assert p.data.data_ptr() == arena_p.data_ptr() + 4 * (start + o)
            assert p.grad.data_ptr() == arena_g.data_ptr() + 4 * (start + o)
        assert g["sync"] is None and g["lr"] == src["lr"]
        assert g["weight_decay"] == src.get("weight_decay", 0.05)
        at += f.numel
    assert at == arena_p.numel()
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    # everything outside the parameters is padding and zero
    used = torch.zeros(at, dtype=torch.bool)
    for g in opt.groups:
        s = (g["flat"].flat_p.data_ptr() - arena_p.data_ptr()) // 4
        for p, o in zip(g["flat"].params, g["flat"].offsets):
            used[s + o:s + o + p.numel()] = True
    assert not arena_p[~used].any()
    # zero_grad re-attaches dropped gradients to the arena
    model.head.weight.grad = None
    opt.zero_grad()
    assert arena_g.data_ptr() <= model.head.weight.grad.data_ptr() < arena_g.data_ptr() + 4 * at


def test_fused_state_round_trips_into_a_per_group_optimizer(favit):
    T = favit.train
    m1, m2 = _vit(favit, 5), _vit(favit, 6)
    fused = T.FusedAdamW(_recipe(favit, m1), lr=1e-4, weight_decay=0.05, distributed=False, fuse_groups=True)
    plain = T.FusedAdamW(_recipe(favit, m2), lr=1e-4, weight_decay=0.05, distributed=False)
    gen = torch.Generator().manual_seed(1)
    for g in fused.groups:
        for p, o in zip(g["flat"].params, g["flat"].offsets):         # (the padding stays zero)
            g["m"][o:o + p.numel()].copy_(torch.randn(p.numel(), generator=gen))
            g["v"][o:o + p.numel()].copy_(torch.rand(p.numel(), generator=gen))
    fused.steps = 9
    state = fused.state_dict(m1)
    plain.load_state_dict(state, m2)
    back = plain.state_dict(m2)
    assert plain.steps == 9 and back["groups"] == state["groups"]
    assert sorted(back["state"]) == sorted(state["state"]) == sorted(n for n, _ in m1.named_parameters())
    for k, st in state["state"].items():
        assert torch.equal(st["m"], back["state"][k]["m"]) and torch.equal(st["v"], back["state"][k]["v"])
        assert st["m"].abs().sum() > 0
    # and the other way round, into a fresh fused optimizer
    m3 = _vit(favit, 7)
    again = T.FusedAdamW(_recipe(favit, m3), lr=1e-4, weight_decay=0.05, distributed=False, fuse_groups=True)
    again.load_state_dict(back, m3)
    for k, st in again.state_dict(m3)["state"].items():
        assert torch.equal(st["m"], state["state"][k]["m"]) and torch.equal(st["v"], state["state"][k]["v"])
    # a schedule sees the groups it always saw
    sched = T.WarmupCosine(again, 2, 10)
    assert len(sched.base_lrs) == len(again.groups) and again.groups[0]["lr"] == sched.base_lrs[0] * 0.5


def test_fused_groups_share_betas_and_eps(favit):
    T = favit.train
    model = _vit(favit)
    groups = _recipe(favit, model)
    groups[1]["betas"] = (0.8, 0.999)
    with pytest.raises(ValueError, match="betas"):
        T.FusedAdamW(groups, distributed=False, fuse_groups=True)
    groups = _recipe(favit, _vit(favit))
    groups[-1]["eps"] = 1e-6
    with pytest.raises(ValueError, match="eps"):
        T.FusedAdamW(groups, distributed=False, fuse_groups=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.FusedAdamW(_recipe(favit, _vit(favit)), distributed=False, fuse_groups=True, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.FusedAdamW(_recipe(favit, _vit(favit)), distributed=False, fuse_groups=True, max_grad_norm=1.0)


def test_flat_buffers_over_caller_storage(favit):
    FB = favit.dp.FlatBuffers
    lin = torch.nn.Linear(5, 3)
    w, b = lin.weight.detach().clone(), lin.bias.detach().clone()
    assert FB.size_of(lin.parameters()) == 16 + 4
    store_p, store_g = torch.zeros(256), torch.zeros(256)
    f = FB(lin.parameters(), store_p, store_g)
    assert f.numel == 256 and f.flat_p is store_p and f.flat_g is store_g and f.offsets == [0, 4]
    assert torch.equal(lin.weight.detach(), w) and torch.equal(store_p[:3], b) and not store_p[20:].any()
    with pytest.raises(ValueError):
        FB(torch.nn.Linear(5, 3).parameters(), torch.zeros(16), torch.zeros(16))
    with pytest.raises(ValueError):
        FB(torch.nn.Linear(5, 3).parameters(), torch.zeros(64))


def test_kernel_wrapper_refuses_cpu_tensors(favit):
    K = favit.kernels
    t = torch.zeros(256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.adamw_multi(t, t.clone(), t.clone(), t.clone(), [256], [1e-3], [0.0], 0.9, 0.999, 1e-8, 1)


def test_entry_points_are_declared_exported_and_bound(favit):
    A = favit._abi
    lib, sig, declared = A.lib(), A._SIGS, A.declared_symbols()
    with open(A.HEADER_PATH) as f:
        header = f.read()
    for name in ("favit_adamw_multi", "favit_adamw_multi_max_segments", "favit_adamw_multi_align"):
        assert name in declared, f"{name} is not declared in include/favit.h"
        assert name in sig, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"libfavit.so does not export {name}"
    assert lib.favit_abi_version() == 8, "the additions are additive: the ABI version stays"
    assert re.search(r"\bint\s+favit_adamw_multi\s*\(\s*const\s+favit_adamw_multi_t\s*\*\s*d\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    mx = int(re.search(r"#define\s+FAVIT_ADAMW_MAX_SEGMENTS\s+(\d+)", header).group(1))
    al = int(re.search(r"#define\s+FAVIT_ADAMW_SEG_ALIGN\s+(\d+)", header).group(1))
    assert (mx, al) == (64, 256) == (lib.favit_adamw_multi_max_segments(), lib.favit_adamw_multi_align())
    assert (A.ADAMW_MAX_SEGMENTS, A.ADAMW_SEG_ALIGN) == (mx, al)
    # the mirror has the header's fields in the header's order, and the C layout that follows from them
    body = re.search(r"typedef struct favit_adamw_multi \{(.*?)\} favit_adamw_multi_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            head, *more = decl.split(",")
            fields += [re.search(r"(\w+)\s*(\[\w+\])?$", head.strip()).group(1)] + [re.sub(r"\W", "", x) for x in more]
    assert fields == [f[0] for f in A.AdamwMulti._fields_]
    assert ctypes.sizeof(A.AdamwMulti) == 6 * 8 + 8 + 4 + 4 + 64 * 8 + 64 * 4 + 64 * 4 + 7 * 4 + 4 + 8
    assert A.AdamwMulti.end.offset == 64 and A.AdamwMulti.coef.offset % 8 == 0
    # a refused table never reaches the device: the library answers before it launches anything
    d = A.AdamwMulti()
    assert lib.favit_adamw_multi(ctypes.byref(d), None) == A.ERR_INVALID


def test_experiment_tool_flags_default_to_off():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("favit_run_experiment_groups", os.path.join(root, "tools", "run_experiment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--experiment", "mhla"])
    assert a.layer_decay is None and a.no_wd_norm_bias is False and a.fuse_groups is False
    b = tool.parse_args(["--experiment", "mhla", "--layer_decay", "0.75", "--no_wd_norm_bias", "--fuse_groups"])
    assert (b.layer_decay, b.no_wd_norm_bias, b.fuse_groups) == (0.75, True, True)
