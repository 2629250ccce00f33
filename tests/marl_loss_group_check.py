"""Checks of mms_marl_ppo_loss_group (include/mms.h, csrc/marl_loss_kernels.hip, csrc/cpu/mms_cpu.cpp) and loss.marl_ppo_loss_group, shared
by the CPU-build tests (test_marl_loss_group.py) and the GPU tests (test_marl_loss_group_gpu.py).

The entry's rule is one sentence -- group g's outputs are the single entry's bits on group g's arguments -- so the yardstick of every
check here is mms_marl_ppo_loss itself (marl_loss_check.run) on the same tensors, compared with `same`; the float64 comparison goes
through marl_loss_check.gates with its constants, this file has no tolerance of its own.

A group is a spec: {"pr": the problem (or, with indices, the storage), "indices", "dense": (mu, value) of an indexed call, "grads",
"row_logp", "pitches", "views": stored fields replacing the problem's}.  Shapes (test files): groups 1, 2, 3 and 32; M = 1, one row
less than, exactly and one more than the rows kernel's rows per workgroup (rows_per_workgroup: kMlThreads of the kernel file over the
lanes per row at that A), and 1000; A = 1, 8, 80, 128."""
import ctypes
import os
import re

import torch

import marl_loss_check as mc
from massive_marl_benchmark_amd import _lib
from massive_marl_benchmark_amd.model import MmsMarlLossGroup
from ppo_loss_check import Guarded, Workspace, same

MAX_GROUPS = 32
OUTPUTS = ("out", "dmu", "dstd", "dvalue", "row_logp")
ALL = mc.cfg(huber=1, clipped=1, pm=1, vm=1, norm=1, factor=1)
KERNELS = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "marl_loss_kernels.hip")


def rows_per_workgroup(A):
    """Rows one step of a rows-kernel workgroup holds at this A: kMlThreads (read from the kernel file) over S, the power of two that
    holds ceil(A / 4) lanes."""
    with open(KERNELS) as f:
        threads = int(re.search(r"constexpr int kMlThreads = (\d+);", f.read()).group(1))
    s = 1
    while 4 * s < A:
        s *= 2
    return threads // s


def shapes():
    """(groups, M, A): every value of the module docstring at least once, with the corners {32 groups, A = 128} and {M = 1}."""
    r8, r128, r1 = rows_per_workgroup(8), rows_per_workgroup(128), rows_per_workgroup(1)
    return [(1, 1, 1), (32, 1, 8), (2, r8 - 1, 8), (3, r8, 8), (3, r8 + 1, 8), (2, r1 + 1, 1), (2, 1000, 80), (32, r128 + 1, 128), (3, 1000, 8), (1, r128 - 1, 80)]


def spec(pr, **kw):
    s = dict(pr=pr, indices=None, dense=None, grads=True, row_logp=True, pitches=None, views=None, drop=())
    s.update(kw)
    return s


def _rows(s):
    return s["dense"][0].shape[0] if s["dense"] is not None else s["pr"]["M"]


def _stored(s):
    return dict(s["pr"], **(s["views"] or {}))


def query(L, device, stream, groups, M, A):
    n = ctypes.c_int64(-1)
    rc = L.mms_marl_ppo_loss_group(device, groups, M, A, None, mc.CLIP, 1.0, 0.0, mc.DELTA, 1, 1, 0, 0, 0, None, ctypes.byref(n), stream)
    return rc, int(n.value)


def table_of(specs, c, outs):
    """The host table over the specs' tensors and the outputs outs[g] = {name: tensor or None}; returns it with what must stay alive."""
    table = (MmsMarlLossGroup * max(len(specs), 1))()
    for t, s, o in zip(table, specs, outs):
        pr = _stored(s)
        mu, value = s["dense"] if s["dense"] is not None else (pr["mu"], pr["value"])
        ptr = lambda x: None if x is None else x.data_ptr()
        t.mu, t.std, t.value, t.indices = ptr(mu), ptr(pr["std"]), ptr(value), ptr(s["indices"])
        t.fields = mc.fields_struct(pr, c, s["pitches"], s["drop"])
        if c["norm"]:
            t.norm_mean, t.norm_var = ptr(pr["norm_mean"]), ptr(pr["norm_var"])
        t.out, t.dmu, t.dstd, t.dvalue, t.row_logp = (ptr(o[k]) for k in OUTPUTS)
    return table


def raw(L, device, stream, groups, M, A, table, c, ws, nbytes):
    n = ctypes.c_int64(nbytes)
    return L.mms_marl_ppo_loss_group(device, groups, M, A, None if table is None else ctypes.addressof(table), c["clip"], c["value_coef"], c["entropy_coef"],
                                     c["delta"], c["huber"], c["clipped"], c["pm"], c["vm"], c["norm"], ws, ctypes.byref(n), stream)


def guarded(specs, dev):
    M, A = _rows(specs[0]), specs[0]["pr"]["A"]
    return [{"out": Guarded((5,), dev), "dmu": Guarded((M, A), dev), "dstd": Guarded((A,), dev), "dvalue": Guarded((M,), dev), "row_logp": Guarded((M,), dev)}
            for _ in specs]


def _on(s, k):
    return k == "out" or (k == "row_logp" and s["row_logp"]) or (k in ("dmu", "dstd", "dvalue") and s["grads"])


def run_group(L, device, stream, specs, c, fill=0x00):
    """One grouped call on guarded outputs and an exactly sized workspace slice; per group what marl_loss_check.run returns."""
    dev = specs[0]["pr"]["mu"].device
    M, A, G = _rows(specs[0]), specs[0]["pr"]["A"], len(specs)
    assert all(_rows(s) == M and s["pr"]["A"] == A for s in specs)
    rc, need = query(L, device, stream, G, M, A)
    _lib.check(rc, None, "mms_marl_ppo_loss_group size query", L)
    assert need % 256 == 0 and (need > 0) == (device >= 0), need
    g = guarded(specs, dev)
    ws = Workspace(need, fill, dev)
    table = table_of(specs, c, [{k: (x.t if _on(s, k) else None) for k, x in gg.items()} for s, gg in zip(specs, g)])
    _lib.check(raw(L, device, stream, G, M, A, table, c, ws.ptr(), need), None, "mms_marl_ppo_loss_group", L)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    results = []
    for s, gg in zip(specs, g):
        res = {k: gg["out"].t[i] for i, k in enumerate(mc.SCALARS)}
        res.update({k: gg[k].t for k in gg if k != "out" and _on(s, k)})
        results.append({"out": res, "guards": all(x.guards_nan() for x in gg.values()), "untouched": all(gg[k].all_nan() for k in gg if not _on(s, k))})
    assert ws.outside_untouched(), "a write outside the workspace slice"
    return results


def run_single(L, device, stream, s, c, fill=0x00):
    """The single entry on one spec's arguments (marl_loss_check.run)."""
    return mc.run(L, device, stream, _stored(s), c, indices=s["indices"], grads=s["grads"], row_logp=s["row_logp"], fill=fill, dense=s["dense"],
                  pitches=s["pitches"])


def equals_single(L, device, stream, specs, c):
    """Every group bit for bit the single entry's result on its arguments, guards intact, what was not asked for untouched; a second
    call (another workspace fill) gives the same bits.  Returns the grouped results."""
    first = run_group(L, device, stream, specs, c, fill=0x00)
    again = run_group(L, device, stream, specs, c, fill=0xFF)
    for g, (s, a, b) in enumerate(zip(specs, first, again)):
        one = run_single(L, device, stream, s, c)
        assert a["guards"] and a["untouched"] and b["guards"] and b["untouched"], ("a write outside an output", g)
        assert same(a["out"], one["out"]), ("group differs from the single entry", g, len(specs))
        assert same(a["out"], b["out"]), ("results depend on the run or on the workspace's content", g)
    return first


def device_name(device):
    return "cpu" if device < 0 else "cuda:%d" % device


def clean_problem(M, A, seed, dev):
    """marl_loss_check.problem at the first of seed, seed + 100, .. whose forced rows lie in no band either (problem draws only the free
    rows again), so that the gates compare the sums of every group"""
    for k in range(20):
        pr = mc.problem(M, A, seed=seed + 100 * k, device=dev)
        in_r, in_v = mc.bands(pr)
        if not bool((in_r | in_v).any()):
            return pr
    raise AssertionError("no problem without a row in a band")


def check_shape(L, device, stream, G, M, A, c=None):
    """G problems of one shape: the single entry's bits, and float64 through marl_loss_check.gates (every group up to three, else the
    first, a middle and the last)."""
    c = c or ALL
    dev = device_name(device)
    specs = [spec(clean_problem(M, A, 11 + g, dev)) for g in range(G)]
    res = equals_single(L, device, stream, specs, c)
    for g in sorted(set(range(G)) if G <= 3 else {0, G // 2, G - 1}):
        fails = mc.gates(specs[g]["pr"], res[g]["out"], c)
        assert not fails, (g, fails)


def independence(L, device, stream, M=300, A=8):
    """Group 1's bits do not move when every other group's inputs are overwritten by different large finite values; per-group mask sums
    (one group nearly all zero) and per-group normaliser statistics each give the single entry's bits."""
    dev = device_name(device)
    prs = [mc.problem(M, A, seed=21 + g, device=dev) for g in range(3)]
    for g, pr in enumerate(prs):
        pr["norm_mean"], pr["norm_var"] = torch.tensor([0.1 + 0.7 * g], device=dev), torch.tensor([1.3 + 2.0 * g], device=dev)
    prs[2]["active_masks"] = torch.zeros(M, device=dev)
    prs[2]["active_masks"][M // 2] = 1.0                              # nearly all zero: a shared mask sum would show here
    assert len({float(pr["active_masks"].sum()) for pr in prs}) == 3
    specs = [spec(pr) for pr in prs]
    before = equals_single(L, device, stream, specs, ALL)
    for g in (0, 2):
        for k in ("mu", "value", "actions", "adv", "value_preds", "returns", "factor", "norm_mean"):
            prs[g][k].mul_(-37.0).add_(1.0e3)
        prs[g]["norm_var"].mul_(50.0)
        prs[g]["old_logp"].add_(0.5)
    after = run_group(L, device, stream, specs, ALL)
    assert same(before[1]["out"], after[1]["out"]), "a group's results depend on another group's inputs"
    assert not same(before[0]["out"], after[0]["out"])


def shared_views(T, N, agents, A, seed, device):
    """Every agent's views of ONE shared [T, N, agents, A] / [T+1, N, agents(, 1)] block (marl_loss_check.shared_block builds one agent's):
    (problems, views per agent, pitches); the bases of two agents' wide fields lie A floats apart."""
    M = T * N
    prs = [mc.problem(M, A, seed + 17 * j, device) for j in range(agents)]
    wide = lambda name: torch.stack([p[name].view(T, N, A) for p in prs], 2).contiguous()
    tall = lambda name: torch.cat([torch.stack([p[name].view(T, N) for p in prs], 2), torch.full((1, N, agents), 7.0, device=device)], 0).contiguous()
    short = lambda name: torch.stack([p[name].view(T, N) for p in prs], 2).contiguous()
    block = {"actions": wide("actions"), "old_logp": wide("old_logp"), "value_preds": tall("value_preds"), "returns": tall("returns"),
             "active_masks": tall("active_masks").unsqueeze(-1), "factor": short("factor").unsqueeze(-1)}
    views = [{"actions": block["actions"][:, :, k], "old_logp": block["old_logp"][:, :, k], "value_preds": block["value_preds"][:, :, k:k + 1],
              "returns": block["returns"][:, :, k:k + 1], "active_masks": block["active_masks"][:, :, k], "factor": block["factor"][:, :, k],
              "adv": prs[k]["adv"].view(T, N, 1).clone()} for k in range(agents)]
    assert views[1]["actions"].data_ptr() - views[0]["actions"].data_ptr() == 4 * A
    pitches = {"actions": agents * A, "old_logp": agents * A, "value_preds": agents, "returns": agents, "active_masks": agents, "factor": agents, "adv": 1}
    return prs, views, pitches


def mixed_options(L, device, stream, T=6, N=25, agents=5, A=8):
    """One call whose groups differ in everything a group may choose: indices given or NULL, row_logp or not, gradients or not, over the
    agents' views of one shared block."""
    dev = device_name(device)
    prs, views, pitches = shared_views(T, N, agents, A, 5, dev)
    M = T * N
    specs = []
    for k in range(agents):
        idx = dense = None
        if k % 2 == 0:                                                # an indexed group: a permutation of its own rows, mu and value gathered
            idx = torch.randperm(M, generator=torch.Generator().manual_seed(k)).to(dev)
            dense = (prs[k]["mu"][idx].contiguous(), prs[k]["value"][idx].contiguous())
        specs.append(spec(prs[k], indices=idx, dense=dense, grads=k not in (1, 2), row_logp=k not in (2, 3), views=views[k], pitches=pitches))
    res = equals_single(L, device, stream, specs, ALL)
    assert "dmu" not in res[1]["out"] and "row_logp" not in res[3]["out"] and set(res[2]["out"]) == set(mc.SCALARS)
    # no group asks for gradients: the finish pass has no column blocks at all
    equals_single(L, device, stream, [spec(prs[k], grads=False, views=views[k], pitches=pitches) for k in range(2)], ALL)
    # a misaligned mu in one group only: that group takes the scalar loads, its neighbours the wide ones
    shifted = torch.zeros(M * A + 1, device=dev)[1:].view(M, A)
    shifted.copy_(prs[1]["mu"])
    equals_single(L, device, stream, [spec(prs[0]), spec(dict(prs[1], mu=shifted)), spec(prs[2])], mc.cfg(**mc.SHIPPED))


def check_error_paths(L, device, stream, messages=None):
    """Every refused call returns non-zero with a message and writes nothing for any group."""
    dev = device_name(device)
    M, A, G = 40, 8, 3
    prs = [mc.problem(M, A, 5 + g, dev) for g in range(G)]
    specs = [spec(pr) for pr in prs]
    rc, need = query(L, device, stream, G, M, A)
    assert rc == 0
    g = guarded(specs, dev)
    ws = Workspace(max(need, 256), 0x5A, dev)
    outs = lambda none=(): [{k: (None if (i, k) in none else x.t) for k, x in gg.items()} for i, gg in enumerate(g)]

    def go(groups=G, table="good", nbytes=need, shift=0, none=(), c=ALL, last=None, pitches=None, drop=(), M=M, A=A):
        sp = list(specs)
        if last is not None or pitches is not None or drop:
            sp[-1] = spec(dict(prs[-1], **(last or {})), pitches=pitches, drop=drop)
        t = None if table is None else table_of(sp, c, outs(none))
        if table == "many":                                           # 33 entries behind the pointer: groups = 33 must be refused, not read
            t = (MmsMarlLossGroup * 33)(*([t[0]] * 33))
        return raw(L, device, stream, groups, M, A, t, c, ws.ptr(shift), nbytes)

    last = G - 1
    bad = [("groups = 0", dict(groups=0), "groups must be 1..%d" % MAX_GROUPS), ("groups = 33", dict(groups=33, table="many"), "groups must be 1..%d" % MAX_GROUPS),
           ("a NULL table", dict(table=None), "table is NULL"), ("M = 0", dict(M=0), "M must be in"), ("A above the limit", dict(A=mc.MAX_A + 1), "A must be in"),
           ("two of the three gradients in one group", dict(none=((1, "dstd"),)), "group 1: mms_marl_ppo_loss: dmu, dstd and dvalue go together"),
           ("a short workspace", dict(nbytes=need - 1), "workspace too small"), ("a misaligned workspace", dict(shift=64), "256-byte aligned"),
           ("NULL mu in the last group", dict(last=dict(mu=None)), "group %d: mms_marl_ppo_loss: null pointer" % last),
           ("NULL out in the last group", dict(none=((last, "out"),)), "group %d: mms_marl_ppo_loss: null pointer" % last),
           ("a mask flag without masks in the last group", dict(drop=("active_masks",)), "active_masks is NULL"),
           ("use_norm without a mean in the last group", dict(last=dict(norm_mean=None)), "use_norm needs"),
           ("an actions pitch below A in the last group", dict(pitches={"actions": A - 1}), "at least A"),
           ("a returns pitch of 0 in the last group", dict(pitches={"returns": 0}), "at least 1")]
    if device < 0:
        bad = [b for b in bad if b[0] != "a short workspace"]        # (the CPU build needs no bytes)
    for label, kw, contains in bad:
        rc = go(**kw)
        msg = _lib.last_error(None, L)
        assert rc != 0 and msg, (label, rc, msg)
        assert contains in msg, (label, msg)
        if messages is not None:
            messages.append((label, msg))
        if dev != "cpu":
            torch.cuda.synchronize()
        assert all(x.all_nan() for gg in g for x in gg.values()) and ws.outside_untouched() and bool((ws.buf == 0x5A).all()), label
    assert L.mms_marl_ppo_loss_group(device, G, M, A, None, mc.CLIP, 1.0, 0.0, mc.DELTA, 1, 1, 0, 0, 0, None, None, stream) != 0
    assert "ws_bytes" in _lib.last_error(None, L)
    assert go() == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    assert not any(bool(torch.isnan(x.t).any()) for gg in g for x in gg.values()) and all(x.guards_nan() for gg in g for x in gg.values())


def counting(L, calls):
    """Counts the calls of the grouped symbol (marl_loss_check.counting counts the single one's); returns the function that restores it."""
    real = L.mms_marl_ppo_loss_group
    L.mms_marl_ppo_loss_group = lambda *a: (calls.append(1), real(*a))[1]

    def restore():
        L.mms_marl_ppo_loss_group = real
    return restore


def python_layer(device, G=3, M=200, A=6, c=None):
    """loss.marl_ppo_loss_group against loss.marl_ppo_loss per agent: objectives, info, row_logp and the gradients with respect to every
    agent's mu, std and value bit for bit (incoming gradients 1, 4, 16 ..: each objective's own, exactly); an agent with mu and std
    detached gets none for them; the single entry is not called, the grouped one twice per 32 agents (size query and launch)."""
    from massive_marl_benchmark_amd.algorithms.marl import loss as loss_mod
    c = c or ALL
    prs = [mc.problem(M, A, seed=31 + g, device=device) for g in range(G)]
    for g, pr in enumerate(prs):
        pr["norm_mean"] = pr["norm_mean"] + 0.25 * g
    idx = [None if g % 2 else torch.randperm(M, generator=torch.Generator().manual_seed(g)).to(device) for g in range(G)]
    fields = [tuple(pr[k] for k in mc.FIELDS[:5]) + (pr["active_masks"], pr["factor"] if c["factor"] else None) for pr in prs]
    kw = mc.loss_kwargs(c)

    def leaves(detach):
        out = []
        for g, pr in enumerate(prs):
            rows = slice(None) if idx[g] is None else idx[g]
            mu, std, v = pr["mu"][rows].clone().requires_grad_(True), pr["std"].clone().requires_grad_(True), pr["value"][rows].clone().view(-1, 1).requires_grad_(True)
            out.append((mu, std, v, g == detach))
        return out

    def ins(leaf):
        mu, std, v, det = leaf
        return (mu.detach(), std.detach(), v) if det else (mu, std, v)

    calls_one, calls_group = [], []
    L, _, _ = _lib.for_device(device)
    restore_one, restore_group = mc.counting(L, calls_one), counting(L, calls_group)
    try:
        lv = leaves(detach=1)
        norms = [(pr["norm_mean"], pr["norm_var"]) for pr in prs] if c["norm"] else None
        objs, info = loss_mod.marl_ppo_loss_group([ins(l)[0] for l in lv], [ins(l)[1] for l in lv], [ins(l)[2] for l in lv], fields, norms=norms, indices=idx,
                                                  row_logp=True, **kw)
        assert not calls_one and len(calls_group) == 2 * ((G + 31) // 32)
        assert len(objs) == G and all(t.shape == (G,) and not t.requires_grad for k, t in info.items() if k != "row_logp")
        sum(4.0 ** g * o for g, o in enumerate(objs)).backward()
    finally:
        restore_one()
        restore_group()
    ref = leaves(detach=1)
    for g, (pr, leaf) in enumerate(zip(prs, ref)):
        more = dict(norm_mean=pr["norm_mean"], norm_var=pr["norm_var"]) if c["norm"] else {}
        o, i = loss_mod.marl_ppo_loss(*ins(leaf), *fields[g], indices=idx[g], row_logp=True, **kw, **more)
        (4.0 ** g * o).backward()
        assert torch.equal(o.detach(), objs[g].detach()), g
        for k in ("policy_loss", "value_loss", "dist_entropy", "ratio"):
            assert torch.equal(i[k], info[k][g]), (g, k)
        assert torch.equal(i["row_logp"], info["row_logp"][g]), g
        for a, b in zip(leaf[:3], lv[g][:3]):
            assert (a.grad is None) == (b.grad is None) and (a.grad is None or torch.equal(a.grad, b.grad)), g
        assert (lv[g][0].grad is None) == (g == 1) and lv[g][2].grad is not None
