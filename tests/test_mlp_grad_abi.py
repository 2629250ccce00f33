"""mms_mlp_grad / mms_mlp_grad_rop per output tensor on the CPU build, and the proof of the harness that test_mlp_grad_abi_gpu.py runs
on the HIP build: the closed form against float64 double backward, every case through the ABI with the gates of mlp_grad_check.py,
and mutations of the evaluation that the gates must catch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mlp_grad_check as mc  # noqa: E402
from massive_marl_benchmark_amd import _lib  # noqa: E402

_REF = {}


def _case(name):
    """(inputs, (truth, yardstick, scale)) of a case, computed once and left unchanged."""
    if name not in _REF:
        inp = mc.case_inputs(name)
        _REF[name] = (inp, mc.reference(inp))
    return _REF[name]


def test_closed_form_against_double_backward():
    """The closed form in float64 equals torch's float64 double backward of the same network (h kept in float64, unrounded: autograd's
    own forward), within 1e-12 of the scale: float64 roundoff times the term count.  The reference is not a copy of the kernel's
    comments."""
    inp = mc.case_inputs("ragged", round_h=False)
    dims, L = inp["dims"], len(inp["dims"]) - 1
    W = [t.double().requires_grad_(True) for t in inp["W"]]
    b = [t.double().requires_grad_(True) for t in inp["b"]]
    g = inp["g"].double().requires_grad_(True)
    hs, as_, cur = [], [], inp["x"].double()
    for l in range(1, L + 1):
        a = cur @ W[l - 1].t() + b[l - 1]
        as_.append(a)
        if l < L:
            cur = torch.where(a > 0, a, torch.expm1(a))
            hs.append(cur)
    mu = as_[-1]
    for mine, theirs in zip(inp["h"], hs):
        assert torch.equal(mine, theirs.detach())
    params = [t for pair in zip(W, b) for t in pair]
    grads = torch.autograd.grad(mu, params, g, create_graph=True)
    de = torch.autograd.grad(mu, as_[:-1] + hs, g, retain_graph=True)
    s = sum((gr * v.double()).sum() for gr, v in zip(grads, [t for pair in zip(inp["V"], inp["C"]) for t in pair]))
    second = torch.autograd.grad(s, params + [g], allow_unused=True)
    auto = {"rmu": second[-1]}
    for l in range(1, L + 1):
        auto["dw_%d" % l], auto["db_%d" % l] = grads[2 * l - 2].detach(), grads[2 * l - 1].detach()
        auto["rdw_%d" % l] = second[2 * l - 2]
        auto["rdb_%d" % l] = second[2 * l - 1] if second[2 * l - 1] is not None else torch.zeros(dims[l], dtype=torch.float64)
        if l < L:
            auto["d_%d" % l], auto["e_%d" % l] = de[l - 1], de[L - 1 + l - 1]
    assert second[2 * L - 1] is None                                  # b_L: nothing of the first gradient depends on it
    a = (dims, inp["x"], inp["h"], inp["W"], inp["g"], inp["V"], inp["C"])
    mine, scale = mc.closed_form(*a, torch.float64), mc.closed_form(*a, torch.float64, absolute=True)
    assert sorted(mine) == sorted(auto)
    for k in mine:
        assert mine[k].shape == auto[k].shape, k
        excess = float(((mine[k] - auto[k]).abs() - 1e-12 * scale[k]).max())
        assert excess <= 0, (k, excess)


def test_cases_reach_their_regimes():
    """The inputs hit the branches of the operand they are meant for."""
    inp, (truth, _, scale) = _case("regimes")
    h1, h2, h3 = inp["h"][:3]
    assert bool((h1[:4] == 0).all()) and bool((h1[4:] != 0).any())
    assert bool((h2 > 0).all())
    share = float((h3 == -1).float().mean())
    print("regimes: share of h_3 == -1 exactly: %.3f" % share)
    assert 0.01 < share < 0.2 and bool((h3 > 0).any()) and bool(((h3 < 0) & (h3 > -1)).any())
    inp, (truth, _, scale) = _case("dead")
    assert bool((inp["h"][1] == -1).all())
    for k in ("d_2", "e_1", "d_1", "dw_1", "db_1", "dw_2", "db_2"):
        assert bool((scale[k] == 0).all()) and bool((truth[k] == 0).all()), k
    assert bool((scale["dw_3"] != 0).any()) and bool((scale["rdw_1"] == 0).all())


@pytest.mark.parametrize("name", list(mc.CASES))
def test_cpu_build_per_tensor(name):
    inp, (truth, yard, scale) = _case(name)
    L = len(inp["dims"]) - 1
    r = mc.run_abi(_lib.lib_cpu(), -1, None, inp, fill=0xFF)
    stats = {}
    fails = mc.gates(r["out"], truth, yard, scale, L, stats)
    print(name, stats)
    mc.record(name, stats, prefix="cpu")
    assert fails == []
    assert r["guards"] and r["ws_outside"] and r["bytes"] == (0, 0)
    # the fp32 yardstick itself passes (b): the per-element bound is one a plain fp32 evaluation meets
    ystats = {}
    assert mc.gates(yard, truth, yard, scale, L, ystats) == []
    print(name, "yardstick (b):", ystats["b"])


def test_gradients_alone():
    """d_out = e_out = NULL: the same dW and db, and nothing else is written."""
    inp, _ = _case("ragged")
    full = mc.run_abi(_lib.lib_cpu(), -1, None, inp)
    bare = mc.run_abi(_lib.lib_cpu(), -1, None, inp, save=False)
    assert bare["guards"] and bare["untouched"] and sorted(bare["out"]) == sorted(k for k in full["out"] if k.startswith(("dw_", "db_")))
    for k, t in bare["out"].items():
        assert torch.equal(t, full["out"][k]), k


def _mutant(inp, **changed):
    m = dict(inp, **{k: v for k, v in changed.items() if k != "fpp"})
    return mc.closed_form(m["dims"], m["x"], m["h"], m["W"], m["g"], m["V"], m["C"], torch.float64, fpp=changed.get("fpp", True))


def _two_planes(w):
    hi = w.bfloat16().float()
    return hi + (w - hi).bfloat16().float()


@pytest.mark.parametrize("name", ["ragged", "wide", "regimes"])
def test_gates_catch_mutations(name):
    """A float64 evaluation with one defect, in place of the output: each must fail the gates."""
    inp, (truth, yard, scale) = _case(name)
    L = len(inp["dims"]) - 1
    assert mc.gates(truth, truth, yard, scale, L) == []
    g = inp["g"].clone()
    g[-1] = 0.0                                                        # a dropped batch row
    wl = inp["W"][-1].clone()
    wl[:, -1] = 0.0                                                    # a dropped k
    mutants = {"row": _mutant(inp, g=g), "k": _mutant(inp, W=inp["W"][:-1] + [wl]),
               "plane": _mutant(inp, W=[_two_planes(w) for w in inp["W"]])}      # a lost third bf16 plane
    if name == "regimes":
        mutants["fpp"] = _mutant(inp, fpp=False)                       # the f'' term left out
    for what, out in mutants.items():
        fails = mc.gates(out, truth, yard, scale, L)
        print(name, what, len(fails), sorted({f[0] for f in fails}))
        assert fails, (name, what)
    hit = {f[0] for f in mc.gates(mutants["row"], truth, yard, scale, L)}
    assert {"dw_%d" % L, "db_%d" % L} <= hit                           # per tensor: the small ones are seen on their own
    if name == "regimes":
        assert all(f[0].startswith(("rdw", "rdb")) for f in mc.gates(mutants["fpp"], truth, yard, scale, L))


def test_guards_and_workspace_bookkeeping():
    """The harness's own detectors: a write into a guard or outside the workspace slice is reported."""
    o = mc.Guarded((3, 5), "cpu")
    assert o.guards_nan() and o.all_nan() and o.t.data_ptr() == o.buf.data_ptr() + 4 * mc.GUARD
    o.t.zero_()
    assert o.guards_nan() and not o.all_nan()
    o.buf[mc.GUARD + 15] = 0.0
    assert not o.guards_nan()
    w = mc.Workspace(1000, 0xFF, "cpu")
    assert w.ptr().value % 256 == 0 and w.n == 1000 and w.outside_untouched()
    w.buf[w.off:w.off + w.n] = 0
    assert w.outside_untouched()
    w.buf[w.off + w.n] = 0
    assert not w.outside_untouched()
