#!/usr/bin/env python3
"""Equal bits of LocalBA and BundleAdjustment between two builds of libasdhip.so (a refactor's check: nothing may move).

  python tools/ba_identity.py --a PATH/libasdhip.so --b PATH/libasdhip.so [--out profiles/ba_setup_identity.json]

Each library runs in a child process of its own (ASDHIP_LIB picks it): the CASES of tests/golden/make_ba_paths_golden.py and of
make_ba_lm_golden.py through asd_local_ba with ASD_BA_STRUCT unset and with ASD_BA_STRUCT=host, and the CASES of make_gba_golden.py
through asd_bundle_adjustment in the form the size picks and in both forced forms (ASD_GBA_SOLVE).  Poses, points, per-edge chi2,
flags, chi2 sums, iteration and trial counts and the debug reports (forms, lm_rounds, gba_forms, gba_trials) are compared with
array_equal; every field must be equal.  Both builds are deterministic run to run (test_gba_two_runs_equal_bits,
tools/diag/ba_determinism.py), so a difference is a difference of the builds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LBA_KEYS = ("poses", "points", "edge_chi2", "edge_outlier1", "edge_depth_pos", "chi2_first", "chi2_second", "iters_first", "iters_second")
GBA_KEYS = ("poses", "points", "edge_chi2", "chi2", "iterations", "trials")


def child(out):
    import __graft_entry__ as g
    from tests.golden import make_ba_lm_golden, make_ba_paths_golden, make_gba_golden
    pkg = g.load_package()

    def ctx(**env):
        for k in ("ASD_BA_STRUCT", "ASD_GBA_SOLVE", "ASD_GBA_UPDATE"):
            os.environ.pop(k, None)
        os.environ.update(env)
        try:
            return pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)   # the switches are read here
        finally:
            for k in env:
                os.environ.pop(k, None)

    res = {}
    for mode, env in (("device", {}), ("host", {"ASD_BA_STRUCT": "host"})):
        c = ctx(**env)
        for mod, tag in ((make_ba_paths_golden, "paths"), (make_ba_lm_golden, "lm")):
            for case in mod.CASES:
                got = c.local_ba(mod.problem(case, pkg.synth), *case.get("its", (5, 10)))
                key = f"lba/{mode}/{tag}/{case['name']}"
                for k in LBA_KEYS:
                    res[f"{key}/{k}"] = np.asarray(got[k])
                res[f"{key}/forms"] = np.asarray(c.local_ba_forms())
                lm = np.asarray(c.local_ba_lm())
                res[f"{key}/lm_rounds"] = lm
        c.close()
    for form in ("default", "tiled", "single"):
        c = ctx(**({} if form == "default" else {"ASD_GBA_SOLVE": form}))
        for case in make_gba_golden.CASES:
            pp = make_gba_golden.problem(case, pkg.synth)
            got = c.bundle_adjustment(pp, n_iterations=int(pp["n_iterations"]), robust=int(pp["robust"]))
            key = f"gba/{form}/{case['name']}"
            for k in GBA_KEYS:
                res[f"{key}/{k}"] = np.asarray(got[k])
            res[f"{key}/gba_forms"] = np.asarray(c.gba_forms())
            res[f"{key}/gba_trials"] = np.asarray(c.gba_trials())
        c.close()
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="the first library (the parent's build)")
    ap.add_argument("--b", help="the second library (this tree's build)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, lib in (("a", a.a), ("b", a.b)):
            npz = os.path.join(tmp, name + ".npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", npz], env=dict(os.environ, ASDHIP_LIB=os.path.abspath(lib)))
            with np.load(npz) as z:
                runs.append({k: z[k] for k in z.files})
    ra, rb = runs
    # lm_rounds[:, 2:] (blocks enqueued, length of the first chunk) follow the PREVIOUS call on the context; the sequence of calls is the same
    # in both children, so they are compared like everything else
    differ = sorted(k for k in set(ra) | set(rb) if k not in ra or k not in rb or not np.array_equal(ra[k], rb[k], equal_nan=True))
    runs_n = len({k.rsplit("/", 1)[0] for k in ra})
    rec = dict(a=a.a, b=a.b, runs=runs_n, fields=len(ra), fields_that_differ=differ, equal=not differ,
               local_ba_forms_seen=sorted({tuple(int(v) for v in ra[k][0][:2]) for k in ra if k.endswith("/forms")}),
               gba_forms_seen=sorted({int(ra[k][0]) for k in ra if k.endswith("/gba_forms")}))
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(main())
