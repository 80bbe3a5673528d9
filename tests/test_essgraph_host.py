"""host/test_essential_graph --edges: asd::Optimizer::EssentialGraphProblem (asd_adapters.hpp) builds, from the flat keyframe views of
every case, exactly the edge list the reference's rules give in g2o's own run (i, j, order; tests/golden/essgraph_golden.npz), the
same fixed mask, and entry estimates and measurements within 4 x S of the driver's (Eigen's arithmetic there, plain C++ here).  No
GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from tests.golden.make_essgraph_golden import CASES, S_NAMES, problem

PROBE = os.path.join(ROOT, "asd-slam_amd", "host", "test_essential_graph")
NAMES = [c["name"] for c in CASES]


def parse_hex(v):
    return np.array([float.fromhex(x) for x in v], np.float64)


def write_problem(path, pp):
    """the views of synth.essential_graph as the probe's problem file"""
    K, M = len(pp["mnId"]), len(pp["mp_ref"])
    hx = lambda a: " ".join(float(x).hex() for x in np.asarray(a).ravel())
    out = [f"{K} {M} {len(pp['lc_kf'])} {int(pp['loop_kf'])} {int(pp['cur_kf'])} {int(pp['fix_scale'])} {int(pp['n_iterations'])}"]
    for k in range(K):
        out.append(f"{int(pp['mnId'][k])} {int(pp['parent'][k])} {int(pp['corrected'][k])} {int(pp['noncorrected'][k])}")
        out += [hx(pp["Tcw"][k]), hx(pp["corrected_sim3"][k]), hx(pp["noncorrected_sim3"][k])]
        for s, f in (("child_start", "child"), ("loop_start", "loop")):
            v = pp[f][pp[s][k]:pp[s][k + 1]]
            out.append(" ".join(map(str, [len(v), *map(int, v)])))
        a, b = pp["cov_start"][k], pp["cov_start"][k + 1]
        out.append(" ".join(map(str, [b - a, *[int(x) for pair in zip(pp["cov"][a:b], pp["cov_w"][a:b]) for x in pair]])))
    for m, kf in enumerate(pp["lc_kf"]):
        v = pp["lc"][pp["lc_start"][m]:pp["lc_start"][m + 1]]
        out.append(" ".join(map(str, [int(kf), len(v), *map(int, v)])))
    for q in range(M):
        out.append(f"{hx(pp['mp_Xw'][q])} {int(pp['mp_ref'][q])} {int(pp['mp_corrected_by'][q])} {int(pp['mp_corrected_ref'][q])}")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "essgraph_golden.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_adapter_builds_the_reference_edge_list(name, golden, synth, tmp_path):
    assert os.path.exists(PROBE), "host/test_essential_graph not built (run __graft_entry__.build())"
    i = NAMES.index(name)
    pp = problem(CASES[i], synth)
    path = str(tmp_path / "problem.txt")
    write_problem(path, pp)
    got = json.loads(subprocess.run([PROBE, "--edges", path], check=True, capture_output=True, text=True).stdout)
    assert got["e_i"] == golden[f"c{i}_e_i"].tolist() and got["e_j"] == golden[f"c{i}_e_j"].tolist()
    K = len(pp["mnId"])
    assert got["fixed"] == [int(r == int(pp["loop_kf"])) for r in range(K)]
    S = dict(zip(S_NAMES, golden["S"]))
    for key, ref in (("sim3", golden[f"c{i}_sim3_in"]), ("e_meas", golden[f"c{i}_e_meas"])):
        a = parse_hex(got[key]).reshape(-1, 8)
        assert a.shape == ref.shape
        if not len(ref):
            continue
        assert float(np.abs(a[:, :4] - ref[:, :4]).max()) <= 4 * S["quaternion"], key    # (the same expression: no sign ambiguity)
        assert float(np.abs(a[:, 4:7] - ref[:, 4:7]).max()) <= 4 * S["translation"], key
        assert float(np.abs(a[:, 7] / ref[:, 7] - 1).max()) <= 4 * S["scale"], key
