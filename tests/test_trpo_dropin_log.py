"""The recorded drop-in run of the reference's unmodified TRPO.run (tests/golden/run_reference_trpo.py, which needs the reference tree
and so is run where that exists): both runs -- the reference's classes and this build's, with the actor's backward and HVPs on
mms_mlp_grad / mms_mlp_grad_rop -- completed, with finite losses and the same number of line searches."""
import os
import re

from test_learners_dropin_log import check_contract_line

LOG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_trpo_dropin.log")


def test_reference_trpo_dropin_log():
    text = open(LOG).read()
    runs = re.split(r"(?m)^(?=TRPO\.run )", text)[1:]
    assert len(runs) == 2, text
    assert "reference RolloutStorage + ActorCritic: ok" in runs[0].splitlines()[0]
    assert "this build's RolloutStorage + ActorCritic(fused_grad=True): ok" in runs[1].splitlines()[0]
    stats = []
    for r in runs:
        m = re.search(r"line_search calls: (\d+), failed: (\d+), actor through mms_mlp_grad / mms_mlp_grad_rop: (\w+), losses finite: (\w+)", r)
        assert m, r
        stats.append(m.groups())
        losses = [float(x) for x in re.findall(r"(?:Value function|Surrogate) loss: (\S+)", r)]
        assert len(losses) == 2 and all(abs(x) < 1e30 for x in losses), r
        assert m.group(4) == "True"
        check_contract_line(r, 2 * 8)                            # every stored observation is the one `act` was given: 2 iterations x nsteps 8
    assert stats[0][0] == stats[1][0] == str(2 * 5 * 4)          # 2 iterations x noptepochs 5 x nminibatches 4 (cfg/trpo)
    assert stats[0][2] == "False" and stats[1][2] == "True"      # the second run's actor took the kernels
