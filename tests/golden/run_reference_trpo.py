#!/usr/bin/env python3
"""Drop-in proof for TRPO: the REFERENCE's agents/algorithms/rl/trpo/trpo.py `TRPO.run` (:99-175 rollout + update, :258-351 the update),
imported in place and left unmodified, driven over this build's VecTaskPython on the CPU build of the engine (device_type="cpu"), for
2 iterations on OneAnt with 64 envs -- once with the reference's own RolloutStorage / ActorCritic, once with this build's
(massive_marl_benchmark_amd.algorithms.rl.trpo) patched into the reference module, with fused_grad=True so that the actor's gradient
and every kl_hessian_times_vector go through mms_mlp_grad / mms_mlp_grad_rop.  Each run logs its losses and the number of
line_search calls (noptepochs x nminibatches per iteration) and of failed line searches, and -- under run_reference_learners.py's
StoredIsSeen recorder -- for how many steps the stored observation is the one `act` was given; tests/test_trpo_dropin_log.py checks the log.

Runs only where the reference tree exists; the import plumbing (name-only stubs, nothing copied) is run_reference_learners.py's.
Writes tests/golden/reference_trpo_dropin.log.

    python tests/golden/run_reference_trpo.py
"""
import contextlib
import functools
import io
import os
import re
import sys
import tempfile
import types

import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import run_reference_learners as rrl  # noqa: E402


def run_trpo(tmp):
    from massive_marl_benchmark_amd.model import default_cfg
    from massive_marl_benchmark_amd.tasks.agent_base.vec_task import VecTaskPython
    from massive_marl_benchmark_amd.tasks.one_ant import OneAnt
    pkg = types.ModuleType("agents.algorithms.rl.trpo")
    pkg.__path__ = [os.path.join(rrl.REF, "agents/algorithms/rl/trpo")]
    sys.modules["agents.algorithms.rl.trpo"] = pkg
    ref_storage = rrl.load("agents.algorithms.rl.trpo.storage", "agents/algorithms/rl/trpo/storage.py")
    ref_module = rrl.load("agents.algorithms.rl.trpo.module", "agents/algorithms/rl/trpo/module.py")
    pkg.RolloutStorage, pkg.ActorCritic = ref_storage.RolloutStorage, ref_module.ActorCritic
    trpo = rrl.load("agents.algorithms.rl.trpo.trpo", "agents/algorithms/rl/trpo/trpo.py")
    cfg_train = yaml.safe_load(open(os.path.join(rrl.REF, "cfg", "trpo", "config.yaml")))
    cfg_train["policy"]["pi_hid_sizes"] = cfg_train["policy"]["vf_hid_sizes"] = [64, 64]     # small networks: a plumbing run
    from massive_marl_benchmark_amd.algorithms.rl import trpo as ours
    for label, storage_cls, module_cls in (("reference RolloutStorage + ActorCritic", ref_storage.RolloutStorage, ref_module.ActorCritic),
                                           ("this build's RolloutStorage + ActorCritic(fused_grad=True)", ours.RolloutStorage,
                                            functools.partial(ours.ActorCritic, fused_grad=True))):
        trpo.RolloutStorage, trpo.ActorCritic = storage_cls, module_cls
        cfg = default_cfg("OneAnt")
        cfg["env"]["numEnvs"] = 64
        cfg["seed"] = 1
        task = OneAnt(cfg, None, "physx", "cpu", 0, True)
        env = VecTaskPython(task, "cpu", cfg_train["clip_observations"], cfg_train["clip_actions"])
        torch.manual_seed(1)
        os.makedirs(os.path.join(tmp, "trpo"), exist_ok=True)
        learner = trpo.TRPO(vec_env=env, cfg_train=cfg_train, device="cpu", sampler=cfg_train["learn"].get("sampler", "sequential"),
                            log_dir=os.path.join(tmp, "trpo"), is_testing=False, print_log=True, apply_reset=False, asymmetric=False)
        calls = [0]
        inner = learner.line_search

        def counted(*a, **k):
            calls[0] += 1
            return inner(*a, **k)
        learner.line_search = counted
        fused = getattr(learner.actor_critic, "_grad_path_qualifies", None)
        fused = bool(fused and fused(torch.zeros(8, env.observation_space.shape[0])))
        rec = rrl.StoredIsSeen(learner, off_policy=False)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            learner.run(num_learning_iterations=2, log_interval=1)
        out = buf.getvalue()
        assert "Learning iteration 1/2" in out, out[-2000:]
        assert all(bool(torch.isfinite(p).all()) for p in learner.actor_critic.parameters())
        losses = [float(x) for x in re.findall(r"(?:Value function|Surrogate) loss:\s*(\S+)", out)]
        rrl.say("TRPO.run (reference agents/algorithms/rl/trpo/trpo.py, unmodified) x 2 iterations on OneAnt 64 envs, CPU build, %s: ok" % label)
        rrl.say("    line_search calls: %d, failed: %d, actor through mms_mlp_grad / mms_mlp_grad_rop: %s, losses finite: %s"
                % (calls[0], out.count("linear search fail"), fused, all(map(lambda v: v == v and abs(v) != float("inf"), losses))))
        rrl.say(rec.line())
        for l in [l.strip() for l in out.splitlines() if any(k in l for k in ("Learning iteration", "Value function loss", "Surrogate loss"))][-3:]:
            rrl.say("    " + " ".join(l.split()))
        task.engine.close()


def main():
    if not os.path.isdir(rrl.REF):
        sys.exit("reference tree not present: this script runs in the build container only")
    rrl.setup_imports()
    rrl.say("# generated by tests/golden/run_reference_trpo.py; torch %s" % torch.__version__)
    with tempfile.TemporaryDirectory() as tmp:
        run_trpo(tmp)
    with open(os.path.join(HERE, "reference_trpo_dropin.log"), "w") as f:
        f.write("\n".join(rrl.LOG) + "\n")


if __name__ == "__main__":
    main()
