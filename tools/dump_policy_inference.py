"""SHA-256 digests of everything GroupedPolicyInference returns, over every route it has: the A/B proof of a change that must not move
a bit (profiles/policy_inference_refactor_*.json).

    python tools/dump_policy_inference.py --device cpu|cuda [--module-file FILE] [--out FILE]

prints ONE JSON object, digest per "<case>/<call>/<output>" (and the route names where a call reports one).  Two versions of
algorithms/marl/policy_inference.py compare by running this once per version -- `--module-file` loads the class from another file of
the same package layout -- on the same build of the library: byte-identical output = bit-identical results.

Feed-forward cases (tests/marl_modules.py networks: obs 46, share_obs 388, 8 actions, layer_N 2; n 3, M 128, hidden 128 unless named):
f16x2 (default), bf16x3, fp32fold (split_layers=False), plain (fold_layernorm=False), small (M 24, hidden 64), chunks (n 20, M 24,
hidden 64, share_obs 1100), sobs390 (n 2, share_obs 390: no folded first critic layer), strided (observations as rows of an
[M, n, 46] block), obs4 (n 2, obs 4, split_layers=False: get_actions must not fold, get_values folds).  Each records get_actions
deterministic, sampled, sampled again into `out=` views of [M, n, .] slots with the draw counters, with one share_obs for all critics,
get_values, evaluate_actions over all agents and over agents [n - 1, 0] with old_logp and factor.
Recurrent cases (tests/marl_rnn_check.py make_agents / make_inputs: n 3, recurrent_N 2): rnn_format fp32 at (M 24, hidden 64) and
(M 128, hidden 128), f16x2 at (M 128, hidden 128); each records get_actions sampled, deterministic with rnn_out into
[M, n, 2, hidden] slots, get_values.
collect: two steps of collect_into and values_into over the tensors of SharedRolloutBuffers, feed-forward (the cached split plan at
128 envs, the generic one at 24) and recurrent (fp32 at 24 envs, f16x2 at 128)."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import marl_modules as mm  # noqa: E402
import marl_rnn_check as rc  # noqa: E402

ACT = 8


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def load_class(module_file):
    if not module_file:
        from massive_marl_benchmark_amd.algorithms.marl.policy_inference import GroupedPolicyInference
        return GroupedPolicyInference
    import massive_marl_benchmark_amd.algorithms.marl  # noqa: F401  (the package the file's relative imports resolve in)
    spec = importlib.util.spec_from_file_location("massive_marl_benchmark_amd.algorithms.marl._policy_inference_ab", module_file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.GroupedPolicyInference


def put(res, case, call, **outs):
    for name, v in outs.items():
        key = "%s/%s/%s" % (case, call, name)
        assert key not in res, key
        if v is None or isinstance(v, str):
            res[key] = v
        else:
            res[key] = digest(torch.stack(list(v)) if isinstance(v, (list, tuple)) else v)


def leaves(g):
    return [g] if g._chunks is None else g._chunks


def feed_forward(cls, res, case, device, n=3, M=128, hidden=128, obs_dim=46, sobs_dim=388, strided=False, **kw):
    gen = torch.Generator().manual_seed(9)
    actors, critics = [], []
    for i in range(n):
        torch.manual_seed(20 + i)
        a, c = mm.Actor(obs_dim, ACT, hidden, 2), mm.Critic(sobs_dim, hidden, 2)
        mm.randomize(a, gen)
        mm.randomize(c, gen)
        actors.append(a.to(device))
        critics.append(c.to(device))
    rn = lambda *s: (torch.randn(*s, generator=gen) * 2).to(device)
    obs = [rn(M, obs_dim) for _ in range(n)]
    if strided:
        block = torch.stack(obs, 1).contiguous()
        obs = [block[:, k] for k in range(n)]
    sobs = [rn(M, sobs_dim) for _ in range(n)]
    g = cls(actors, critics, seed=1, **kw)
    values, actions, none = g.get_actions(sobs, obs, deterministic=True)
    assert none is None
    put(res, case, "deterministic", values=values, actions=actions)
    values, actions, logp = g.get_actions(sobs, obs)
    put(res, case, "sampled", values=values, actions=actions, logp=logp)
    given, old = [t.clone() for t in actions], [t.clone() for t in logp]
    slots = [torch.full((M, n, w), float("nan"), device=device) for w in (1, ACT, ACT)]
    g.get_actions(sobs, obs, out=tuple([s[:, k] for k in range(n)] for s in slots))
    put(res, case, "sampled_out", values=slots[0], actions=slots[1], logp=slots[2], counters=torch.cat([c.counters for c in leaves(g)]))
    values, actions, _ = g.get_actions([sobs[0]] * n, obs, deterministic=True)
    put(res, case, "shared_share_obs", values=values, actions=actions)
    put(res, case, "get_values", values=g.get_values(sobs))
    put(res, case, "evaluate", logp=g.evaluate_actions(obs, given), eval_route=g.eval_route)
    sel = [n - 1, 0]
    factor = [torch.full((M, 1), 1.0 + 0.25 * i, device=device) for i in range(2)]
    lp = g.evaluate_actions([obs[k] for k in sel], [given[k] for k in sel], agents=sel, old_logp=[old[k] * 0.99 for k in sel], factor=factor)
    put(res, case, "evaluate_factor", logp=lp, factor=factor, eval_route=g.eval_route)


def recurrent(cls, res, case, device, M, hidden, rnn_format, n=3, recurrent_N=2):
    actors, critics = rc.make_agents(n, hidden, recurrent_N, device, seed=hidden + 7 * recurrent_N + M)
    x = rc.make_inputs(n, M, hidden, recurrent_N, device, seed=M + hidden)
    g = cls(actors, critics, seed=3, rnn_format=rnn_format)
    kw = dict(rnn_states=x["rs"], rnn_states_critic=x["rsc"], masks=x["masks"])
    values, actions, logp, new_a, new_c = g.get_actions(x["sobs"], x["obs"], **kw)
    put(res, case, "sampled", values=values, actions=actions, logp=logp, rnn_states=new_a, rnn_states_critic=new_c, rnn_route=g.rnn_route,
        counters=g.counters)
    slots = [torch.full((M, n, recurrent_N, hidden), float("nan"), device=device) for _ in range(2)]
    values, actions, none, new_a, new_c = g.get_actions(x["sobs"], x["obs"], deterministic=True, rnn_out=tuple([s[:, k] for k in range(n)] for s in slots), **kw)
    assert none is None and new_a[0].data_ptr() == slots[0].data_ptr()
    put(res, case, "deterministic_rnn_out", values=values, actions=actions, rnn_states=slots[0], rnn_states_critic=slots[1], rnn_route=g.rnn_route)
    put(res, case, "get_values", values=g.get_values(x["sobs"], rnn_states_critic=x["rsc"], masks=x["masks"]), rnn_route=g.rnn_route)


def collect(cls, res, case, device, envs, hidden, recurrent_N=0, rnn_format="fp32", n=3, T=2):
    if recurrent_N:
        actors, critics = rc.make_agents(n, hidden, recurrent_N, device, seed=31)
    else:
        gen = torch.Generator().manual_seed(31)
        actors, critics = [mm.Actor(rc.OBS, ACT, hidden, 2) for _ in range(n)], [mm.Critic(rc.SOBS, hidden, 2) for _ in range(n)]
        for m in actors + critics:
            mm.randomize(m, gen)
            m.to(device)
    sh = rc.shared_tensors(n, T, envs, hidden, max(recurrent_N, 1), device, seed=32)
    g = cls(actors, critics, seed=7, rnn_format=rnn_format)
    for s in range(T):
        sh.step = s
        acts = g.collect_into(sh)
        assert acts.data_ptr() == sh.actions[s].data_ptr()
    sh.step = 0
    g.collect_into(sh)                                               # a second rollout: the cached operands of slot 0, a new draw
    dst = torch.full((envs, n), float("nan"), device=device)
    g.values_into(sh, dst)
    put(res, case, "rollout", actions=sh.actions, logp=sh.action_log_probs, values=sh.value_preds[:T], rnn_states=sh.rnn_states,
        rnn_states_critic=sh.rnn_states_critic, counters=g.counters, bootstrap_values=dst, rnn_route=g.rnn_route)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    ap.add_argument("--module-file", default="", help="load GroupedPolicyInference from this copy of policy_inference.py instead")
    ap.add_argument("--out", default="", help="also write the JSON object to this file")
    a = ap.parse_args()
    cls, dev, res = load_class(a.module_file), a.device, {}
    with torch.no_grad():
        feed_forward(cls, res, "f16x2", dev)
        feed_forward(cls, res, "bf16x3", dev, split_format="bf16x3")
        feed_forward(cls, res, "fp32fold", dev, split_layers=False)
        feed_forward(cls, res, "plain", dev, fold_layernorm=False)
        feed_forward(cls, res, "small", dev, M=24, hidden=64)
        feed_forward(cls, res, "chunks", dev, n=20, M=24, hidden=64, sobs_dim=1100)
        feed_forward(cls, res, "sobs390", dev, n=2, sobs_dim=390)
        feed_forward(cls, res, "strided", dev, strided=True)
        feed_forward(cls, res, "obs4", dev, n=2, obs_dim=4, split_layers=False)
        recurrent(cls, res, "rnn_fp32_M24_H64", dev, 24, 64, "fp32")
        recurrent(cls, res, "rnn_fp32_M128_H128", dev, 128, 128, "fp32")
        recurrent(cls, res, "rnn_f16x2_M128_H128", dev, 128, 128, "f16x2")
        collect(cls, res, "collect_ff_split", dev, 128, 128)
        collect(cls, res, "collect_ff_generic", dev, 24, 64)
        collect(cls, res, "collect_rnn_fp32", dev, 24, 64, recurrent_N=2)
        collect(cls, res, "collect_rnn_f16x2", dev, 128, 128, recurrent_N=2, rnn_format="f16x2")
    if dev == "cuda":
        torch.cuda.synchronize()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
