"""Generates tests/golden/reference_cfg_model.json: the `model` dict of the reference's shipped configuration
(configs/raggesture_beatx/basegesture_len150_beat.py), evaluated and stored as data, so that
tests/test_reference_config_cpu.py runs without the reference tree.  Runs only where the reference exists."""
import json
import os
import sys
sys.dont_write_bytecode = True   # the reference is read-only: no __pycache__ there

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

CFG = os.path.join(_ref_import.REF_ROOT, "configs", "raggesture_beatx", "basegesture_len150_beat.py")


def main():
    ns = {}
    with open(CFG) as f:
        exec(compile(f.read(), CFG, "exec"), ns)      # a plain-Python mmcv config: `model` only uses names of the same file
    with open(os.path.join(HERE, "reference_cfg_model.json"), "w") as f:
        json.dump(ns["model"], f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
