"""Share of the visible (view, Gaussian) pairs of the headline workload (1M Gaussians, 1024^2, seeded scene, orbit
cameras) whose packed span word (csrc/gsr_span_word.h) is "not encodable", and why, on the CPU: the oracle's fp32
preprocess values through span_prep / span_row restated in float32 (tests/emit_span_cases.py spans_cpu).
  python profiles/diag_emit_spans.py [--gaussians N] [--res R] [--views V]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("threestudio-3dgs_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import gsr_synthetic as gs  # noqa: E402
from emit_span_cases import spans_cpu  # noqa: E402
from gsr_testutil import make_camera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gaussians", type=int, default=1_000_000)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--views", type=int, default=2)
args = ap.parse_args()
scene = gs.make_scene(args.gaussians, sh_degree=0, seed=0)
for v in range(args.views):
    cam = make_camera(args.res, args.res, elevation=15.0, azimuth=360.0 * v / 64)
    sp = spans_cpu(scene, cam)
    vis = int(sp["vis"].sum())
    rows5 = int((sp["vis"] & (sp["rows"] > 4)).sum())
    len16 = int((sp["vis"] & (sp["len"].max(1) > 15)).sum())
    print(json.dumps(dict(view=v, visible=vis, not_encodable=vis - int(sp["enc"].sum()),
                          share=round(1.0 - sp["enc"].sum() / max(vis, 1), 5), more_than_4_rows=rows5,
                          row_longer_than_15=len16, rect_tiles=int((sp["rows"] * (sp["rect"][:, 2] - sp["rect"][:, 0]))[sp["vis"]].sum()),
                          kept_tiles=int(sp["len"].sum()))))
