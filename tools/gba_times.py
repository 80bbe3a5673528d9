#!/usr/bin/env python3
"""Times of asd_bundle_adjustment on TIMING_CASES of tests/golden/make_gba_golden.py (the two-keyframe initial map, 128 and 1024
keyframes with banded covisibility, a loop and ~100 points per keyframe), against the parent's only route to such a problem:
  local_ba  asd_local_ba(its_first = n, its_second = 0) on the same graph (LocalBA's Huber width: a timing comparison only);
  single    asd_bundle_adjustment, ASD_GBA_SOLVE=single (LocalBA's one-workgroup dense solvers);
  tiled     asd_bundle_adjustment, ASD_GBA_SOLVE=tiled (gba.hip, trailing update on f64 MFMA);
  tiled_fma the same with ASD_GBA_UPDATE=fma (trailing update on plain FMA).
Each form runs in a context of its own (the switches are read at asd_ctx_create).  Wall time of the call and device time between
the call's events: median and minimum of --reps calls after --warmup.  Where one trial of a one-workgroup solve takes seconds (the
1024-keyframe map: an n = 6138 Cholesky in one workgroup) the form runs ONCE with --slow-its iterations and the time per trial is
what is reported.  --sweep adds the crossover: single against tiled on banded maps of 33..64 free keyframes.
DESIGN.md quotes the output (profiles/gba_times.json) next to g2o's time on the same problems (`make_gba_golden.py --times`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
from tests.golden.make_gba_golden import BAND, TIMING_CASES, C, problem  # noqa: E402

FORMS = {"local_ba": {}, "single": {"ASD_GBA_SOLVE": "single"}, "tiled": {"ASD_GBA_SOLVE": "tiled"},
         "tiled_fma": {"ASD_GBA_SOLVE": "tiled", "ASD_GBA_UPDATE": "fma"}}
SLOW_FROM = 400   # free keyframes from which a one-workgroup dense solve is run once, not --reps times


def make_ctx(pkg, env):
    for k in ("ASD_GBA_SOLVE", "ASD_GBA_UPDATE"):
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
    finally:
        for k in env:
            os.environ.pop(k, None)


def time_form(pkg, form, pp, its, reps, warmup):
    ctx = make_ctx(pkg, FORMS[form])
    try:
        wall, dev, last = [], [], None
        for k in range(warmup + reps):
            t0 = time.perf_counter()
            try:
                if form == "local_ba":
                    r = ctx.local_ba(pp, its_first=its, its_second=0)
                    last = dict(iterations=int(r["iters_first"]), trials=int(ctx.local_ba_lm()[0][1]), forms=[int(v) for v in ctx.local_ba_forms()[0]])
                else:
                    r = ctx.bundle_adjustment(pp, n_iterations=its, robust=True)
                    last = dict(iterations=r["iterations"], trials=r["trials"], forms=ctx.gba_forms())
            except pkg.AsdError as e:
                return dict(form=form, refused=str(e))
            t1 = time.perf_counter()
            if k >= warmup:
                wall.append((t1 - t0) * 1e3)
                dev.append(float(ctx.last_stage_ms("ba")))
        return dict(form=form, reps=reps, its=its, call_ms_median=float(np.median(wall)), call_ms_min=float(min(wall)),
                    device_ms_median=float(np.median(dev)), device_ms_min=float(min(dev)),
                    device_ms_per_trial=float(np.median(dev)) / max(last["trials"], 1), **last)
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-its", type=int, default=1)
    ap.add_argument("--cases", default="", help="comma-separated subset of TIMING_CASES")
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    out = dict(cases=[], sweep=[])
    for case in TIMING_CASES:
        if a.cases and case["name"] not in a.cases.split(","):
            continue
        pp = problem(case, pkg.synth)
        n_free = int((pp["fixed"] == 0).sum())
        rec = dict(name=case["name"], poses=len(pp["poses"]), points=len(pp["points"]), edges=len(pp["e_point"]), forms=[])
        for form in a.forms.split(","):
            slow = n_free >= SLOW_FROM and form in ("local_ba", "single")
            r = time_form(pkg, form, pp, a.slow_its if slow else case["its"], 1 if slow else a.reps, 0 if slow else a.warmup)
            rec["forms"].append(r)
            print(f"{case['name']} P {rec['poses']} L {rec['points']} E {rec['edges']} | {json.dumps(r)}", flush=True)
        out["cases"].append(rec)
    if a.sweep:
        for n_free in (33, 36, 40, 44, 48, 56, 64):
            pp = problem(C(f"sweep_{n_free}", BAND(n_free, 80 + n_free), its=6), pkg.synth)
            rec = dict(free=n_free, forms=[time_form(pkg, form, pp, 6, a.reps, a.warmup) for form in ("single", "tiled")])
            out["sweep"].append(rec)
            print(f"sweep nPf {n_free}: " + " | ".join(f"{r['form']} device {r['device_ms_median']:.3f} ms call {r['call_ms_median']:.3f} ms ({r['trials']} trials)"
                                                     for r in rec["forms"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
