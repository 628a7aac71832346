"""Generate the zero-background backward fixtures the feature tests add, by
running the REFERENCE renderer (make_golden.run_case, same file format).

    python tests/golden/make_feature_golden.py --ref <reference checkout> [--only NAME ...]

With bg = 0 the reference's image is sum_i c_i sigmoid(logit_i) and its clamp
never binds, so its image and gradients pin a feature render of
sigmoid(logits) (tests/test_features_gpu.py) as well as the colour render
(every test that walks tests/golden/*.npz picks these up too).  Like
make_golden.py this runs at fixture-generation time only, never from the tests.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import run_case, synth  # noqa: E402


def cases(ref, only=None):
    ident = np.eye(4, dtype=np.float32)
    out = []
    if only is None or "zero_bg_random" in only:  # the default tile, overlapping footprints
        rng = np.random.default_rng(21)
        xyz, cov, lg, op, fx, fy = synth(60, 64, 64, rng, slo=0.01, shi=0.05)
        out.append(run_case(ref, "zero_bg_random", xyz, cov, lg, op, ident, 64, 64, fx, fy, [0, 0, 0]))
    if only is None or "zero_bg_tile12" in only:  # clipped edge cells, partial tiles
        rng = np.random.default_rng(22)
        xyz, cov, lg, op, fx, fy = synth(50, 52, 44, rng, slo=0.01, shi=0.05)
        out.append(run_case(ref, "zero_bg_tile12", xyz, cov, lg, op, ident, 52, 44, fx, fy, [0, 0, 0], tile=12))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    # (these cases' records: a manifest of their own, make_golden.py's stays as it wrote it)
    man_path = os.path.join(HERE, "feature_manifest.json")
    manifest = json.load(open(man_path)) if os.path.exists(man_path) else {}
    for rec in cases(a.ref, set(a.only) if a.only else None):
        manifest[rec["name"]] = rec
        print(json.dumps(rec), flush=True)
    json.dump(manifest, open(man_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
