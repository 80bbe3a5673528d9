"""asd::Initializer (asd-slam_amd/host/asd_adapters.hpp) through host/test_initializer.

Without a device: --draws against the restatement -- the first Initializer of the process srand(0)s (SeedRandOnce), eight RandomInt per
iteration in iteration order (Initializer.cc:84-100), and a second Initializer in the same process continues the rand() sequence.  On the
device (marked gpu): asd::Initializer::Initialize equal to the direct call with those draws, for two Initializers in one process."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import initializer_cases as C
from tests import initializer_ref as R
from tests.conftest import ROOT

PROBE = os.path.join(ROOT, "asd-slam_amd", "host", "test_initializer")


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "asd-slam_amd", "csrc"), "../host/test_initializer"])
    return lambda *a: subprocess.run([PROBE, *map(str, a)], capture_output=True, text=True, timeout=120)


def expected_draws(calls):
    """calls = [(N, iterations)] in process order -> the draws of each, from one rand() sequence after srand(0)"""
    raw = R.libc_rand(0, 8 * sum(it for _, it in calls))
    out, at = [], 0
    for N, it in calls:
        out.append(R.draws_from_raw(raw[at:at + 8 * it], N, it))
        at += 8 * it
    return out


def test_draws_mode_equals_the_restatement(probe):
    for iterations, Ns in ((200, (64, 120)), (3, (8, 9, 300)), (1, (8,))):
        r = probe("--draws", iterations, *Ns)
        assert r.returncode == 0, r.stderr
        lines = [l.split() for l in r.stdout.strip().splitlines()]
        assert len(lines) == len(Ns) and all(l[0] == "draws" for l in lines)
        for l, e in zip(lines, expected_draws([(N, iterations) for N in Ns])):
            assert [int(x) for x in l[1:]] == e.reshape(-1).tolist()


def _hex(v):
    return " ".join(float(x).hex() for x in np.asarray(v, np.float32).reshape(-1))


@pytest.mark.gpu
def test_initialize_equals_the_direct_call(probe, hip, tmp_path):
    cases = ["general64", "small40", "unmatched"]     # ok, refused, keys without a match; the second and third continue the sequence
    Ps = [C.problem(c) for c in cases]
    path = tmp_path / "problem.txt"
    with open(path, "w") as f:
        f.write(f"{len(Ps)}\n")
        for P in Ps:
            f.write(f"{len(P['keys1'])} {len(P['keys2'])} {float(P['sigma']).hex()} {P['n_iter']}\n{_hex(P['K'])}\n{_hex(P['keys1'])}\n"
                    f"{_hex(P['keys2'])}\n{' '.join(str(int(m)) for m in P['matches12'])}\n")
    r = probe(path)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    draws = expected_draws([(P["N"], P["n_iter"]) for P in Ps])
    assert not np.array_equal(draws[1][:8], C.problem("small40")["draws"][:8])          # (not the draws of a fresh process)
    f32 = lambda v: np.array([float.fromhex(x) for x in v], np.float32)
    oks = []
    for P, d, g in zip(Ps, draws, got):
        assert g["draws"] == d.reshape(-1).tolist()
        res = hip.initialize([dict(P, draws=d)])[0]
        oks.append(res["ok"])
        assert g["ok"] == res["ok"] and g["model"] == res["model"]
        assert f32([g["SH"], g["SF"]]).tobytes() == np.array([res["SH"], res["SF"]], np.float32).tobytes()
        if res["ok"]:
            assert f32(g["R21"]).tobytes() == res["R21"].tobytes() and f32(g["t21"]).tobytes() == res["t21"].tobytes()
            assert f32(g["P3D"]).tobytes() == res["P3D"].tobytes() and g["triangulated"] == res["triangulated"].tolist()
        else:
            assert g["R21"] == [] and g["P3D"] == [] and g["triangulated"] == []
    assert oks[0] == 1 and oks[1] == 0
