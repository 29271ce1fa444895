"""Host side of the encoder backward's queue (functional._BackwardQueue): WHEN the collected weight gradients are
launched, what an exception leaves behind, the order of the deferred folds and of the gradient-ready calls, and the
zero pool.  No GPU: functional._gt returns None for CPU tensors, so lin_bwd_w allocates and queues, and the launches
are replaced with recorders.  A schedule is the list of launches per block, then those at close; ("grouped", 48) is one
grouped launch of 48 problems.  The expected schedules were recorded with this driver before the queue became a class."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, HD = 64, 256
SHAPES = ((D, HD), (HD, D), (D, D), (3 * D, D))          # (N, K) of a block's four weight-gradient problems


def record(F, setattr_, events, decline=()):
    """Replace the launches the queue issues with recorders that append (kind, problems) to events.  decline: the
    kinds among "ragged" / "grouped" that answer False, as the library does for a list it cannot take."""
    def launch(kind):
        def f(probs, *a, **kw):
            ok = kind not in decline
            events.append((kind if ok else kind + " declined", len(probs)))
            return ok
        return f
    K = F.K
    setattr_(K, "gemm_grouped_tn", launch("grouped"))
    setattr_(K, "gemm_grouped_tn_ragged", launch("ragged"))
    setattr_(K, "gemm", lambda *a, **kw: events.append(("gemm", 1)))
    setattr_(K, "reduce_rows_multi", launch("reduce"))
    setattr_(K, "mhla_fold_bwd_multi", launch("fold"))


def queue_block(F, rows):
    M = 2 * rows
    for N, Kd in SHAPES:
        F.lin_bwd_w(torch.zeros(M, N, dtype=torch.bfloat16), torch.zeros(M, Kd, dtype=torch.bfloat16), M, N, Kd)


def drive(F, rows, per_block, events):
    sched = []
    with F._BackwardQueue(per_block=per_block) as q:
        for i, r in enumerate(rows):
            n0 = len(events)
            queue_block(F, r)
            q.end_block((2 * r, 2 * rows[i + 1]) if i + 1 < len(rows) else None)
            sched.append(events[n0:])
        n0 = len(events)
    sched.append(events[n0:])
    return sched


@pytest.fixture
def rec(favit, monkeypatch):
    """(functional, events): the launches are recorders, no ready hook, no FAVIT_WGRAD_PER_BLOCK."""
    F, ev = favit.functional, []
    record(F, monkeypatch.setattr, ev)
    monkeypatch.setitem(F._STATE, "grad_ready", None)
    monkeypatch.delenv("FAVIT_WGRAD_PER_BLOCK", raising=False)
    return F, ev


RAGGED_ROWS = list(range(5, 72, 6)) + [71, 71]           # 5, 11, ..., 71, 71, 71: 14 blocks
HOLD_ROWS = [64 << i for i in range(6)]                  # 64, 128, ..., 2048


def test_uniform_blocks_launch_every_twelve(rec):
    F, ev = rec
    assert F.K.GROUP_MAX == 48
    want = [[]] * 11 + [[("grouped", 48)]] + [[]] * 2 + [[("grouped", 8)]]
    assert drive(F, [8] * 14, False, ev) == want


def test_ragged_blocks_launch_every_twelve(rec):
    F, ev = rec
    want = [[]] * 11 + [[("ragged", 48)]] + [[]] * 2 + [[("ragged", 8)]]
    assert drive(F, RAGGED_ROWS, True, ev) == want


@pytest.mark.parametrize("per_block", [False, True])
def test_a_ready_hook_means_four_blocks_per_launch(rec, monkeypatch, per_block):
    F, ev = rec
    monkeypatch.setitem(F._STATE, "grad_ready", lambda p: None)
    kind = "ragged" if per_block else "grouped"
    rows = [5, 11, 17, 23, 29, 35] if per_block else [8] * 6
    assert drive(F, rows, per_block, ev) == [[], [], [], [(kind, 16)], [], [], [(kind, 8)]]


def test_declined_ragged_list_goes_block_by_block(rec, monkeypatch):
    F, ev = rec
    record(F, monkeypatch.setattr, ev, decline=("ragged",))
    assert drive(F, [5, 11, 17], True, ev) == [[], [], [], [("ragged declined", 12)] + [("grouped", 4)] * 3]


def test_declined_grouped_launch_goes_gemm_by_gemm(rec, monkeypatch):
    F, ev = rec
    record(F, monkeypatch.setattr, ev, decline=("ragged", "grouped"))
    block = [("grouped declined", 4)] + [("gemm", 1)] * 4
    assert drive(F, [5, 11], True, ev) == [[], [], [("ragged declined", 8)] + block * 2]


def _child(case):
    """Runs in a child process (the hold limit is read from the environment at import): prints the schedule."""
    sys.path.insert(0, ROOT)
    F = importlib.import_module("focused-attention-vit_amd").functional
    ev = []
    record(F, setattr, ev)
    F._STATE["grad_ready"] = None
    rows, per_block = (HOLD_ROWS, True) if case == "ragged" else ([512] * 6, False)
    print(json.dumps(drive(F, rows, per_block, ev)))


@pytest.mark.parametrize("case,hold_mb,want", [
    ("uniform", None, [[]] * 6 + [[["grouped", 24]]]),            # six blocks of 2 MB under the default 384 MB
    ("uniform", "1", [[["grouped", 4]]] * 6 + [[]]),
    ("ragged", "1", [[], [["ragged", 8]]] + [[["ragged", 4]]] * 4 + [[]]),
])
def test_hold_limit(case, hold_mb, want):
    env = {k: v for k, v in os.environ.items() if k not in ("FAVIT_WGRAD_PER_BLOCK", "FAVIT_WGRAD_HOLD_MB")}
    if hold_mb:
        env["FAVIT_WGRAD_HOLD_MB"] = hold_mb
    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), case], env=env, text=True)
    assert json.loads(out.strip().splitlines()[-1]) == want


def test_per_block_switch(rec, monkeypatch):
    F, ev = rec
    monkeypatch.setenv("FAVIT_WGRAD_PER_BLOCK", "1")
    for rows, per_block in (([8] * 5, False), ([5, 11, 17, 23, 29], True)):
        assert drive(F, rows, per_block, ev) == [[("grouped", 4)]] * 5 + [[]]


def test_exception_drops_the_queue_without_launching(rec):
    F, ev = rec
    with pytest.raises(RuntimeError, match="boom"):
        with F._BackwardQueue() as q:
            queue_block(F, 8)
            q.end_block()
            queue_block(F, 8)
            F._SIDE["pending"].append(object())
            raise RuntimeError("boom")
    assert ev == [] and F._QUEUE is None and F._SIDE["pending"] == []
    queue_block(F, 8)                                     # no queue is open: every problem launches at once
    assert ev == [("gemm", 1)] * 4


def _param(*shape, grad=True):
    p = torch.nn.Parameter(torch.zeros(*shape))
    if grad:
        p.grad = torch.zeros(*shape)
    return p


def test_folds_wait_for_weight_gradients_and_ready_calls_follow_launches(rec, monkeypatch):
    """Two blocks, each: a Linear with gradient buffers, a Linear with a buffer for its weight only, a Linear with
    none, the folded qkv projection of an MHLA chain and a LayerNorm backward.  The hook hears of exactly the
    parameters whose buffers a launch wrote, after that launch, in queue order."""
    F, ev = rec
    monkeypatch.setattr(F, "_gt", lambda p: None if p is None or not p.requires_grad else p.grad)

    def layernorm_bwd(dy, x, ldx, gamma, mean, rstd, rows, Dn, *, dg_out, db_out, defer, **kw):
        defer.append((torch.zeros(2, 1, Dn), dg_out, db_out))         # the defer= contract of kernels.layernorm_bwd
        return x, None, None, None
    monkeypatch.setattr(F.K, "layernorm_bwd", layernorm_bwd)
    names = {}
    monkeypatch.setitem(F._STATE, "grad_ready", lambda p: ev.append(("ready", names[id(p)])))

    def named(tag, p):
        names[id(p)] = tag
        return p
    chain = F.MHLAChain(2, 7)
    M, bf = 16, torch.bfloat16
    want_w, want_d = [], []
    with F._BackwardQueue(zero_floats=2 * (3 * D + 4)) as q:
        for b in "ab":
            w1, b1 = named(b + ".w1", _param(D, D)), named(b + ".b1", _param(D))
            w2, b2 = named(b + ".w2", _param(D, D)), named(b + ".b2", _param(D, grad=False))
            w3, b3 = _param(D, D, grad=False), _param(D, grad=False)
            for w, c in ((w1, b1), (w2, b2), (w3, b3)):
                F.lin_bwd_w(torch.zeros(M, D, dtype=bf), torch.zeros(M, D, dtype=bf), M, D, D, wp=w, bp=c)
            prm = [named(b + "." + n, _param(*s)) for n, s in
                   (("wqkv", (3 * D, D)), ("bqkv", (3 * D,)), ("wl", (D // 2, D // 2)), ("bl", (D // 2,)))]
            assert chain.qkv_grads(torch.zeros(M, 3 * D, dtype=bf), torch.zeros(M, D, dtype=bf), prm + [None, None]) == [None] * 4
            gam, bet = named(b + ".gamma", _param(D)), named(b + ".beta", _param(D))
            F.EncoderOp._ln_bwd(torch.zeros(M, D), torch.zeros(M, D), (gam, bet), None, None, None, (0.0, 0))
            assert ev == [], "nothing is launched inside a block"
            want_w += [("ready", b + ".w1"), ("ready", b + ".b1"), ("ready", b + ".w2")]
            want_d.append([("ready", b + ".gamma"), ("ready", b + ".beta")])
            want_d.append([("ready", b + "." + n) for n in ("wqkv", "bqkv", "wl", "bl")])
        with pytest.raises(AssertionError, match="not been launched"):
            q.flush_deferred()                            # four weight gradients per block are still waiting
        assert ev == [] and len(q.wgrads) == 8 and len(q.folds) == 2 and len(q.ln_folds) == 2
        assert isinstance(q.wgrads[0], F._WGrad) and isinstance(q.folds[0], F._Fold) and isinstance(q.ln_folds[0], F._LNFold)
        assert q.end_block() is False and ev == []
    assert ev == ([("grouped", 8)] + want_w + [("reduce", 2)] + want_d[0] + want_d[2] + [("fold", 2)] + want_d[1] + want_d[3])


def test_zero_pool(favit):
    F = favit.functional
    cpu = torch.device("cpu")
    with F._BackwardQueue(zero_floats=24, device=cpu) as q:
        base = q.zeros.data_ptr()
        vs = [F._zero_vec(n, cpu) for n in (5, 6, 7)]
        assert [tuple(v.shape) for v in vs] == [(5,), (6,), (7,)]
        assert [v.data_ptr() - base for v in vs] == [0, 32, 64], "16-byte boundaries, no overlap"
        assert all(v.data_ptr() % 16 == 0 and v.dtype == torch.float32 and not v.any() for v in vs)
        spill = F._zero_vec(1, cpu)                       # 24 floats are taken: a fresh tensor
        assert spill.untyped_storage().data_ptr() != q.zeros.untyped_storage().data_ptr() and not spill.any()
        other = F._zero_vec(4, torch.device("meta"))      # another device than the pool's
        assert other.device.type == "meta" and q.zero_off == 24
    assert F._QUEUE is None
    fresh = F._zero_vec(3, cpu)                           # no queue: fresh zeros
    assert tuple(fresh.shape) == (3,) and not fresh.any()
    with F._BackwardQueue() as q:                         # a queue without a pool
        assert q.zeros is None and not F._zero_vec(3, cpu).any()


if __name__ == "__main__":
    _child(sys.argv[1])
