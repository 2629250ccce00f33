#!/usr/bin/env python3
"""Fixtures for the configuration checks of tests/test_host_logic.py, so that they run without the reference tree:

    reference_cfg.json   cfg/TenAnt.yaml, cfg/OneAnt.yaml and cfg/MultiIngenuity.yaml as parsed values (yaml.safe_load), one
                         entry per task: what model.default_cfg must equal
    nv_ant.xml           assets/mjcf/open_ai_assets/ant/nv_ant.xml, the ant's model description: the input of model.load_mjcf_ant

Runs only where the reference tree exists (MMS_REFERENCE, as tests/golden/make_fixtures.py).

    python tests/golden/make_config_fixtures.py
"""
import json
import os
import shutil
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import REF  # noqa: E402

TASKS = ("TenAnt", "OneAnt", "MultiIngenuity")


def main():
    if not os.path.isdir(REF):
        sys.exit("reference tree not found at %s" % REF)
    cfg = {task: yaml.safe_load(open(os.path.join(REF, "cfg", task + ".yaml"))) for task in TASKS}
    with open(os.path.join(HERE, "reference_cfg.json"), "w") as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write("\n")
    shutil.copyfile(os.path.join(REF, "assets", "mjcf", "open_ai_assets", "ant", "nv_ant.xml"), os.path.join(HERE, "nv_ant.xml"))
    print("wrote reference_cfg.json, nv_ant.xml")


if __name__ == "__main__":
    main()
