"""The recorded drop-in run of the reference's unmodified learners (tests/golden/run_reference_learners.py, which needs the reference
tree and so is run where that exists): thirteen combinations, each completed -- and the six single-agent ones (PPO, DDPG, TD3; the
reference's classes and this build's; with the two TRPO runs of reference_trpo_dropin.log, eight) stored, at EVERY step of `run`, the observation `actor_critic.act` was given, with
next_observations the tensor `step` returned (the recorder is StoredIsSeen in that script; the contract itself, on this build's
classes alone, is tests/test_dropin_contract.py)."""
import os
import re

LOG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_learners_dropin.log")
CONTRACT = re.compile(r"^    stored observations == observations acted on: (\d+)/(\d+) steps; observations != next_observations: (\d+)/(\d+)$", re.M)


def check_contract_line(entry, steps):
    """The entry carries the line, N/N on both counts, for `steps` add_transitions calls."""
    m = CONTRACT.search(entry)
    assert m, entry
    same, of, differ, differ_of = (int(x) for x in m.groups())
    assert same == of == steps, entry
    assert differ == differ_of and differ_of >= steps - 1, entry


def test_reference_learners_dropin_log():
    text = open(LOG).read()
    entries = re.split(r"(?m)^(?=(?:PPO|DDPG|TD3|Runner)\.run )", text)[1:]
    assert len(entries) == 13, text
    heads = [e.splitlines()[0] for e in entries]
    assert all(h.endswith(": ok") and "unmodified" in h for h in heads), heads
    assert [h.split(".run")[0] for h in heads] == ["PPO"] * 2 + ["Runner"] * 7 + ["DDPG"] * 2 + ["TD3"] * 2
    assert sum(", reference " in h for h in heads) == 6 and sum(", this build's " in h for h in heads) == 7     # (mappo: a third, grouped form)
    single = [e for e in entries if not e.startswith("Runner")]
    assert len(single) == 6
    for e in single:
        # PPO: 2 iterations x nsteps 8 (cfg/ppo); DDPG / TD3: 3 iterations x nsteps 8 (cfg/ddpg, cfg/td3)
        check_contract_line(e, 16 if e.startswith("PPO") else 24)
    assert not any(CONTRACT.search(e) for e in entries if e.startswith("Runner"))     # (the MARL runners insert at once: test_dropin_contract.py)
