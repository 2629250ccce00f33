"""The policy head fused into the step (mms_bind_policy_head; csrc/head_block.h: ppo_head_block with SWAVES > 0 and the staging waves'
ppo_head_stage_values) at the critic widths VH and head widths H the module-level tests never reach -- one check list for both builds:
tests/test_head_shapes.py runs it on libmms_cpu.so, tests/test_head_shapes_gpu.py on libmms.so.

The C ABI is driven directly with an MmsPolicyHead (ActorCritic ties VH to a network).  Two TenAnt engines with the same seed:
A steps with the head bound, B with mms_ppo_heads_act into its "actions" tensor and then mms_step.  After reset_all and one zero-action
step every case is ONE more step on the same pair (the pair's state must stay bit-equal, so it is reused).  Three gates per case:
  (a) ppo_rollout_check.gate_sample on what the fused step left, with the 8-wave split of the step kernel: mu, value, draw and logp
      against float64 within that file's derived bounds, and its exact parts.  No bound is stated here.
  (b) every slot and the counters bit for bit what ppo_rollout_check.sample_run's stand-alone call leaves on the same operands;
  (c) the engine state of A and B bit for bit after the step.
Poison: every destination is an `Out` (NaN-filled, guarded); hidden, vhidden, vweight and the tiled weight copy each carry a tail of
TAIL NaN floats behind their last element, so a read past the end that enters a sum makes a mean or a value NaN and fails (a).  The
staged loop's second load from a clamped address and the rows clamped to N - 1 read inside the arrays and must not reach a result.
With `mutation` a case corrupts its own truth (gate_sample's hooks) and only returns the ratios."""
import numpy as np
import torch

import ppo_rollout_check as pc
from massive_marl_benchmark_amd.engine import Engine
from massive_marl_benchmark_amd.model import MmsPolicyHead

A = 80
TAIL = 512
ENGINE = ("root_states", "dof_state", "obs", "obs_clipped", "rew", "actions", "reset", "progress", "reset_count", "prev")
SEED = 0x9E3779B97F4A7C15                                            # (a seed with a high word)
# VH against the staged loop's lane map (lane l: floats 4 l .. 4 l + 3 of a 256-float trip, two trips per pass of 512):
#   4 only lane 0 works; 252 the last lane idle; 256 a first trip on every lane, no second; 260 / 508 the second trip on lane 0 only / on
#   all lanes but the last; 512 one whole pass; 516 / 768 / 772 a second pass with no / every / one lane on its second trip; 1024 two
#   whole passes; 1284 a third pass
VHS = (4, 252, 256, 260, 508, 512, 516, 768, 772, 1024, 1284)


def _cases():
    """name -> dict(N, H, VH, tiles, ref_scale, counters, row_offset, flags, dests).  The arguments that are not the default are spread
    over the cases, not multiplied through them: reference_scale alternates, the counters follow ppo_rollout_check.check_heads' pattern
    (one row at 2^32 in every third case), row_offset is 3 or 3 + 2^33, reset flags are raised by hand in the first and the last block
    in two cases.  dests: the slots handed over (None: all six)."""
    out = {}
    shapes = [(48, 512, VH) for VH in VHS] + [(N, 1024, VH) for VH in (260, 1024) for N in (16, 48)]
    for i, (N, H, VH) in enumerate(shapes):
        for tiles in (True, False):
            k = 2 * i + int(tiles)
            out["N%d_H%d_VH%d_%s" % (N, H, VH, "tiles" if tiles else "rows")] = dict(
                N=N, H=H, VH=VH, tiles=tiles, ref_scale=(i + int(tiles)) % 2, counters=k % 3, row_offset=3 + (2 ** 33 if k % 4 == 1 else 0),
                flags=(N == 48 and VH in (260, 1284) and tiles), dests=None)
    base = dict(N=48, H=512, tiles=True, ref_scale=1, counters=1, row_offset=3, flags=False)
    out["N48_H512_VH772_no_actions_out"] = dict(base, VH=772, dests=tuple(d for d in pc.DESTS if d != "actions_out"))
    out["N48_H512_VH260_act_and_value_only"] = dict(base, VH=260, dests=("act_slot", "value_slot"))
    return out


CASES = _cases()


def _counters(N, kind):
    """kind 0: zeros; 1: check_heads' pattern; 2: the same with row 1 at 2^32"""
    c = np.zeros(N, np.int64) if kind == 0 else (np.arange(N, dtype=np.int64) * 7) % 5
    if kind == 2:
        c[1] += 2 ** 32
    return c


def _poisoned(a, tdev):
    """`a` on the device with TAIL NaN floats behind its last element"""
    buf = torch.full((a.size + TAIL,), float("nan"), dtype=torch.float32, device=tdev)
    buf[:a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(tdev)
    assert buf.data_ptr() % 16 == 0
    return buf[:a.size].view(a.shape)


def weight_tiles(w):
    """the layout of mms_policy_head.weight_tiles (include/mms.h): element ((ct (H / 4) + k / 4) 16 + i) 4 + k % 4 = weight[16 ct + i][k],
    zero rows for outputs >= A"""
    n, H = w.shape
    nct = (n + 15) // 16
    pad = np.zeros((nct * 16, H), np.float32)
    pad[:n] = w
    return np.ascontiguousarray(pad.reshape(nct, 16, H // 4, 4).transpose(0, 2, 1, 3)).reshape(-1)


class Pair:
    """Engines A (takes the bound head) and B (mms_ppo_heads_act + mms_step) of N envs, same seed, one zero-action step behind them."""

    def __init__(self, env, N, monkeypatch):
        monkeypatch.setenv("MMS_STEP_BLOCK16", "1")                  # the <768, 16> layout at these sizes, for both engines (read per launch)
        self.env, self.N = env, N
        tdev = torch.device(env[3])
        self.engines = [Engine("TenAnt", num_envs=N, device=0 if tdev.type == "cuda" else "cpu", seed=11, clip_obs=5.0) for _ in range(2)]
        for e in self.engines:
            assert e.takes_policy_head(), "the engine does not take a bound policy head at this size"
            assert e.num_actions == A
            e.reset_all()
            e.tensor("actions").zero_()
            e.step()
        pc._sync(env[3])
        self.assert_same_state("warm-up")

    def assert_same_state(self, what, skip=()):
        a, b = self.engines
        bad = [k for k in ENGINE if k not in skip and not torch.equal(a.tensor(k), b.tensor(k))]
        assert not bad, "%s: the engine with the bound head and the one stepped by mms_ppo_heads_act + mms_step differ in %s" % (what, bad)

    def close(self):
        for e in self.engines:
            e.close()


def pair_for(pairs, env, N, monkeypatch):
    """the pair of N envs in the runner's cache `pairs`, opened at its first use"""
    if N not in pairs:
        pairs[N] = Pair(env, N, monkeypatch)
    return pairs[N]


def run_case(pair, name, monkeypatch, mutation=None):
    """One step of `pair` at CASES[name]: the three gates (module docstring); returns gate_sample's ratios.  With `mutation` the truth of
    gate (a) is corrupted and nothing of (a) is asserted."""
    monkeypatch.setenv("MMS_STEP_BLOCK16", "1")
    c = CASES[name]
    env = pair.env
    L, di, stream, tdev = env
    N, H, VH = c["N"], c["H"], c["VH"]
    assert N == pair.N
    dests = pc.DESTS if c["dests"] is None else c["dests"]
    eng_a, eng_b = pair.engines
    pr = pc.heads_data(N, H, A, VH, 1000 * H + 10 * VH + N + int(c["tiles"]))
    d = {k: _poisoned(pr[k], tdev) for k in ("hidden", "vhidden", "vweight")}
    d.update({k: pc._up(pr[k], tdev) for k in ("weight", "bias", "vbias", "log_std", "value")})
    pr["_dev_%s" % tdev] = d                                           # (sample_run's stand-alone call reads the same buffers)
    tiles = _poisoned(weight_tiles(pr["weight"]), tdev) if c["tiles"] else None
    ctr = _counters(N, c["counters"])
    seed = SEED + c["ref_scale"]
    kw = dict(ref_scale=c["ref_scale"], seed=seed, row_offset=c["row_offset"], counters=ctr)
    flagged = torch.tensor(sorted({1, 5, N - 1}), device=tdev)
    if c["flags"]:                                                   # envs reset under a bound head, first and last block
        for e in pair.engines:
            e.tensor("reset")[flagged] = 1

    # A: the head bound, one step
    shapes = dict(actions_out=(N, A), act_slot=(N, A), logp_slot=(N,), value_slot=(N,), mu_slot=(N, A), sigma_slot=(N, A))
    o = {k: pc.Out(shapes[k], tdev) for k in dests if k != "actions_out"}
    cnt_a = pc._up(ctr, tdev)
    p = lambda t: None if t is None else t.data_ptr()
    head = MmsPolicyHead(hidden=p(d["hidden"]), weight=p(d["weight"]), bias=p(d["bias"]), vhidden=p(d["vhidden"]), vweight=p(d["vweight"]), vbias=p(d["vbias"]),
                         log_std=p(d["log_std"]), counters=p(cnt_a), actions_out=p(eng_a.tensor("actions")) if "actions_out" in dests else None,
                         seed=seed, row_offset=c["row_offset"], H=H, VH=VH, A=A, reference_scale=c["ref_scale"], weight_tiles=p(tiles),
                         **{k: p(v.buf) for k, v in o.items()})
    if "actions_out" in dests:
        eng_a.tensor("actions").fill_(float("nan"))
    eng_a.bind_policy_head(head)
    eng_a.step()
    pc._sync(tdev)
    fused = {k: (o[k].get() if k in o else None) for k in pc.DESTS}
    if "actions_out" in dests:
        fused["actions_out"] = eng_a.tensor("actions").cpu().numpy().copy()
    fused["counters"] = cnt_a.cpu().numpy()
    fused["value_in"] = None

    # (b) the stand-alone call on the same operands
    alone = pc.sample_run(env, pr, "heads", value=None, dests=dests, **kw)
    for k in dests:
        assert pc.same_bits(fused[k], alone[k]), (name, "the fused step and mms_ppo_heads_act differ in", k)
    assert (fused["counters"] == alone["counters"]).all(), (name, "counters")

    # B: the stand-alone call into its own action tensor (actions_out = NULL in A: A's act_slot instead), then the step
    if "actions_out" in dests:
        cnt_b = pc._up(ctr, tdev)
        q = pc._p
        pc._ok(L, L.mms_ppo_heads_act(di, q(d["hidden"]), q(d["weight"]), q(d["bias"]), H, None, q(d["vhidden"]), q(d["vweight"]), q(d["vbias"]), VH, q(d["log_std"]),
                                      seed, q(cnt_b), c["row_offset"], c["ref_scale"], q(eng_b.tensor("actions")), None, None, None, None, None, N, A, stream),
               "mms_ppo_heads_act")
        skip = ()
    else:
        eng_b.tensor("actions").copy_(o["act_slot"].t)
        skip = ("actions",)                                          # (unspecified in A with actions_out = NULL: include/mms.h)
    eng_b.step()
    pc._sync(tdev)
    # (c)
    pair.assert_same_state(name, skip=skip)
    if c["flags"]:
        assert int(eng_a.tensor("progress")[flagged].max()) == 0, (name, "a hand-raised reset flag was not seen")

    # (a) the fused step's outputs against float64.  A slot the case leaves NULL is taken from the stand-alone call (which (b) has just
    # shown equal in every slot that IS given); actions_out = NULL: the exact part "actions_out = act_slot" has nothing to compare.
    seen = dict(fused)
    if len(dests) < len(pc.DESTS):
        full = pc.sample_run(env, pr, "heads", value=None, **kw)
        for k in dests:
            assert pc.same_bits(fused[k], full[k]), (name, k)
        for k in pc.DESTS:
            if seen[k] is None:
                seen[k] = seen["act_slot"] if k == "actions_out" else full[k]
    r = pc.gate_sample(pr, seen, "heads", N=N, waves=8, mutation=mutation, **kw)
    if mutation is None:
        pc.report(tdev, name, group="head_shapes", **r)
        assert max(r.values()) <= 1.0, (name, r)
    return r
