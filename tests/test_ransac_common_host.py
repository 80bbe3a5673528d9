"""The host-callable pieces of asd-slam_amd/csrc/ransac.h through host/test_ransac_common (no device, no library).

ransac_sample<K> (K = 3, 4, 8) against the literal swap-with-back replay -- every draw tuple at n = K and n = K + 1, 10^5 seeded tuples at
n = 64 and n = 2000 -- and jacobi_svd<true> / <false> on seeded 16x9, 8x9, 6x5, 6x3, 3x3 matrices, a zero column and two equal columns:
orthogonal columns, W V^T equal to the input, and identical bits of the two forms on matrices of full column rank.  The program states
its bounds and prints every figure; its exit status is the number of failed checks."""
import os
import subprocess

from tests.conftest import ROOT

PROBE = os.path.join(ROOT, "asd-slam_amd", "host", "test_ransac_common")


def test_ransac_sample_and_jacobi_svd():
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "asd-slam_amd", "csrc"), "../host/test_ransac_common"])
    r = subprocess.run([PROBE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    assert [l for l in lines if l.startswith("sample")] == [
        "sample K=3: 200030 tuples, 0 differ from the replay",     # 3! + 4! + 2 x 10^5
        "sample K=4: 200144 tuples, 0 differ from the replay",     # 4! + 5! + 2 x 10^5
        "sample K=8: 603200 tuples, 0 differ from the replay"]     # 8! + 9! + 2 x 10^5
    assert sum(l.endswith("identical bits") for l in lines) == 4   # 16x9, 6x5, 6x3, 3x3
    assert sum(l.startswith("svd") and "bound 1" in l for l in lines) == 14 and not any("FAILED" in l for l in lines)
