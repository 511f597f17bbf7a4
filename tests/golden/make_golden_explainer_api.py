#!/usr/bin/env python3
"""The public surface of the caption explainers, recorded once: `inspect.signature` of every public method (inherited ones included) and
every public class constant of `GridTDEngine`, `AOAEngine` and the ten drop-in `Explain*` classes.  tests/test_explainer_api_host.py
compares the tree at hand against tests/golden/explainer_api.json.  No GPU needed (the modules import without the HIP library).

    python tests/golden/make_golden_explainer_api.py --commit <hash of the checkout this runs in>"""
import argparse
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
JSON = os.path.join(HERE, "explainer_api.json")
CLASSES = {"gridtd": ("GridTDEngine", "ExplainGridTDAttention", "ExplainiGridTDGuidedGradient", "ExplainGridTDGuidedGradCam",
                      "ExplainGridTDGradient", "ExplainGridTDGradCam"),
           "aoa": ("AOAEngine", "ExplainAOAAttention", "ExplainAOAGradient", "ExplainAOAGuidedGradient", "ExplainAOAGuidedGradCam",
                   "ExplainAOAGradCam")}


def inventory():
    """{"module.Class": {"methods": {name: signature}, "constants": {name: value}}} of the tree `lrp_amd` is imported from"""
    import importlib
    out = {}
    for mod, names in CLASSES.items():
        m = importlib.import_module("lrp_amd.explainers." + mod)
        for name in names:
            cls = getattr(m, name)
            methods = {k: str(inspect.signature(v)) for k, v in inspect.getmembers(cls, callable)
                       if not k.startswith("_") or k == "__init__"}
            consts = {k: v for k, v in inspect.getmembers(cls, lambda v: not callable(v)) if not k.startswith("_")}
            out["%s.%s" % (mod, name)] = {"methods": methods, "constants": json.loads(json.dumps(consts))}      # (tuples as lists)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit of the checkout this runs in")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lrp_amd  # noqa: F401
    with open(JSON, "w") as f:
        json.dump({"recorded_from_commit": a.commit, "classes": inventory()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(os.path.basename(JSON) + ":", os.path.getsize(JSON), "bytes")


if __name__ == "__main__":
    main()
