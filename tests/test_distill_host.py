"""Knowledge distillation without a GPU: the float64 reference against torch's own losses and against the closed-form
gradient the header states, the argument checks of train.Distill and the kernels wrappers, the ABI table against the
header, and the runner's flags."""
import importlib.util
import os
import re

import pytest
import torch

import _distill_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_ = torch.nn.functional


def _case(B, Cn, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cn, generator=g, dtype=torch.float64) * 3
    z = torch.randn(B, Cn, generator=g, dtype=torch.float64) * 3
    if B > 1:
        x[0] = 80.0 * (1 - 2 * (torch.arange(Cn) % 2))
        z[1] = 80.0 * (1 - 2 * (torch.arange(Cn) % 2))
    y = torch.randint(0, Cn, (B,), generator=g)
    lam = torch.tensor([(0.0, 0.3, 1.0, 0.75)[b % 4] for b in range(B)])
    return x, z, y, lam


@pytest.mark.parametrize("tau", [1.0, 3.0])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("B,Cn", [(1, 1), (5, 2), (7, 65)])
def test_soft_reference_is_hintons_loss(B, Cn, alpha, tau):
    x, z, y, _ = _case(B, Cn)
    ref = R.reference(x, z, y, None, 0.1, alpha, tau, "soft")
    kl = F_.kl_div(torch.log_softmax(x / tau, 1), torch.log_softmax(z / tau, 1), reduction="batchmean",
                   log_target=True) * tau * tau
    want = (1 - alpha) * F_.cross_entropy(x, y, label_smoothing=0.1) + alpha * kl
    assert abs(ref["kd"] - kl.item()) < 1e-12 * max(1.0, abs(kl.item()))
    assert abs(ref["loss"] - want.item()) < 1e-12 * max(1.0, abs(want.item()))


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("B,Cn", [(1, 1), (5, 2), (7, 65)])
def test_hard_reference_is_cross_entropy_against_the_teachers_argmax(B, Cn, alpha):
    x, z, y, _ = _case(B, Cn)
    ref = R.reference(x, z, y, None, 0.0, alpha, 1.0, "hard")
    kd = F_.cross_entropy(x, z.argmax(1))          # (random rows have no ties; the +-80 row's first maximum is class 0)
    want = (1 - alpha) * F_.cross_entropy(x, y) + alpha * kd
    assert abs(ref["kd"] - kd.item()) < 1e-12 * max(1.0, abs(kd.item()))
    assert abs(ref["loss"] - want.item()) < 1e-12 * max(1.0, abs(want.item()))


def test_lowest_argmax_breaks_ties_downwards():
    z = torch.zeros(3, 70, dtype=torch.float64)
    z[1, 3] = z[1, 64] = 2.0
    z[2, 69] = 1.0
    assert R.lowest_argmax(z).tolist() == [0, 3, 69]


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kind,tau", [("soft", 1.0), ("soft", 3.0), ("hard", 1.0)])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_autograd_gradient_is_the_headers_closed_form(eps, alpha, kind, tau, mixed):
    for B, Cn in ((1, 1), (5, 2), (7, 65)):
        x, z, y, lam = _case(B, Cn, seed=3)
        lam = lam if mixed else None
        ref = R.reference(x, z, y, lam, eps, alpha, tau, kind)
        closed = R.closed_form_grad(x, z, y, lam, eps, alpha, tau, kind, 1.0 / B)
        assert (ref["grad"] - closed).abs().max().item() < 1e-12, (B, Cn)


def test_distill_validates_on_construction(favit):
    D = favit.train.Distill
    d = D(0.5, 3.0, "hard")
    assert (d.alpha, d.tau, d.kind, d.hard) == (0.5, 3.0, "hard", True) and not D(1.0).hard and D(0.0).tau == 1.0
    for bad in (dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=0.5, tau=0.0), dict(alpha=0.5, tau=float("nan")),
                dict(alpha=0.5, tau=float("inf")), dict(alpha=0.5, kind="medium"), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            D(**bad)
    T = favit.train
    with pytest.raises(ValueError):
        T._check_teacher(torch.nn.Linear(2, 2), None)
    with pytest.raises(ValueError):
        T._check_teacher(None, D(0.5))
    with pytest.raises(TypeError):
        T._check_teacher(torch.nn.Linear(2, 2), 0.5)


def test_kernels_argument_checks_raise_before_any_library_call(favit, monkeypatch):
    K = favit.kernels

    def no_library():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(favit._abi, "lib", no_library)
    x, y, z = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3)
    for kw, err in ((dict(distill_alpha=-0.1), ValueError), (dict(distill_alpha=1.1), ValueError),
                    (dict(distill_alpha=0.5, distill_tau=0.0), ValueError),
                    (dict(distill_alpha=0.5, distill_tau=float("nan")), ValueError)):
        with pytest.raises(err):
            K.cross_entropy(x, y, teacher=z, **kw)
    for t in (torch.zeros(2, 4), torch.zeros(3, 3), torch.zeros(6), torch.zeros(2, 3, dtype=torch.float64),
              torch.zeros(3, 2).t(), [[0.0] * 3] * 2):
        with pytest.raises(TypeError):
            K.cross_entropy(x, y, teacher=t, distill_alpha=0.5)
    with pytest.raises(ValueError, match="meta"):                    # another device than the logits'
        K.cross_entropy(x, y, teacher=torch.zeros(2, 3, device="meta"), distill_alpha=0.5)
    with pytest.raises(ValueError):                                  # a weight without a teacher
        K.cross_entropy(x, y, distill_alpha=0.5)
    with pytest.raises(ValueError):
        K.cross_entropy_distill(x, z, y, alpha=1.5)
    with pytest.raises(ValueError):
        K.cross_entropy_distill(x, z, y, alpha=0.5, label_smoothing=1.0)
    # a hard teacher does not use tau
    with pytest.raises(RuntimeError):                                # (past the checks: CPU tensors are refused)
        K.cross_entropy(x, y, teacher=z, distill_alpha=0.5, distill_tau=0.0, distill_hard=True)


def test_entry_point_is_declared_and_bound_with_one_arity(favit):
    sig = favit._abi._SIGS
    name = "favit_cross_entropy_distill"
    assert name in favit._abi.declared_symbols(), f"{name} is not declared in include/favit.h"
    with open(favit._abi.HEADER_PATH) as f:
        header = f.read()
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, "no declaration found"
    args = [a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert len(args) == 15 and len(sig[name][0]) == 15
    # logits, teacher, labels, lam, loss_rows, kd_rows, dlogits are pointers; then B, C; four floats; hard; the stream
    want = ["*"] * 7 + ["int32_t"] * 2 + ["float"] * 4 + ["int32_t", "*"]
    for a, w in zip(args, want):
        assert w in a and (w == "*" or "*" not in a), (a, w)
    import ctypes as C
    assert sig[name][0] == [C.c_void_p] * 7 + [C.c_int32] * 2 + [C.c_float] * 4 + [C.c_int32, C.c_void_p]
    assert sig[name][1] is C.c_int


def _runner():
    spec = importlib.util.spec_from_file_location("favit_run_experiment_distill",
                                                  os.path.join(ROOT, "tools", "run_experiment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_runner_flags(capsys):
    tool = _runner()
    a = tool.parse_args(["--experiment", "mhla"])
    assert a.teacher_experiment is None and a.teacher_weights is None and a.distill_alpha == 0.0
    assert a.distill_tau == 1.0 and a.distill_type == "soft"
    a = tool.parse_args(["--experiment", "mhla_pretrained", "--weights", "w.npz", "--teacher_experiment", "traditional",
                         "--teacher_weights", "w.npz", "--distill_alpha", "0.5", "--distill_tau", "3",
                         "--distill_type", "hard"])
    assert (a.teacher_experiment, a.teacher_weights, a.distill_alpha, a.distill_tau, a.distill_type) == \
        ("traditional", "w.npz", 0.5, 3.0, "hard")
    for bad in (["--distill_alpha", "0.5"], ["--distill_alpha", "1.5", "--teacher_experiment", "mhla"],
                ["--teacher_experiment", "sppp_mhla"], ["--teacher_experiment", "mhla", "--distill_tau", "0"],
                ["--teacher_experiment", "mhla", "--distill_type", "firm"], ["--teacher_weights", "w.npz"]):
        with pytest.raises(SystemExit):
            tool.parse_args(["--experiment", "mhla"] + bad)
    capsys.readouterr()


def test_runner_builds_a_frozen_teacher_of_the_students_size(favit, tmp_path, capsys):
    import numpy as np
    tool = _runner()
    a = tool.parse_args(["--experiment", "mhla", "--img_size", "32", "--patch_size", "4", "--embed_dim", "64", "--depth",
                         "2", "--num_heads", "4", "--dropout", "0.1", "--drop_path", "0.1", "--teacher_experiment",
                         "traditional", "--distill_alpha", "0.5"])
    torch.manual_seed(0)
    donor = tool.build_teacher(favit, a, 10)
    path = str(tmp_path / "w.npz")
    np.savez(path, **{k: v.numpy() for k, v in donor.state_dict().items()})
    a.teacher_weights = path
    torch.manual_seed(1)
    teacher = tool.build_teacher(favit, a, 10)
    assert isinstance(teacher, favit.models.vit.VisionTransformer) and not teacher.training
    assert all(not p.requires_grad for p in teacher.parameters())
    assert all(m.p == 0 for m in teacher.modules() if isinstance(m, torch.nn.Dropout))
    assert all(float(getattr(m, "drop_path", 0.0) or 0.0) == 0.0 for m in teacher.modules())
    for (k, v), (_, w) in zip(sorted(teacher.state_dict().items()), sorted(donor.state_dict().items())):
        assert torch.equal(v, w), k
    student = tool.build_model(favit, a, 10)
    assert student.head.weight.shape == teacher.head.weight.shape
    capsys.readouterr()
