"""bench.py's two hosts -- the C++ loop over the C ABI (asd-slam_amd/host/track_loop.cpp) and the Python loop -- run the
same tracking step: identical per-frame statistics, with and without read-ahead."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if "asd_bench" in sys.modules:
        return sys.modules["asd_bench"]
    spec = importlib.util.spec_from_file_location("asd_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["asd_bench"] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline,fused,async_ba,split,chain", [(True, True, False, True, False), (False, True, False, True, False), (True, False, False, True, False),
                                                                   (True, True, True, True, False), (True, True, False, False, False), (True, True, False, True, True)])
def test_cxx_host_equals_python_host(pkg, pipeline, fused, async_ba, split, chain):
    """fused: the stages run as asd_track_motion_model / asd_track_local_map (one submission each, bench default) or as
    matcher + PoseOptimization calls (--no-fuse); async_ba: LocalBA in line (default, the reference's order) or on the optional lane (--lane-ba); split: the C++ host's split-phase
    stages (asd_track_async / asd_track_finish, default) or each stage run to completion (--no-split); chain: both stages as one submission
    (asd_track_frame, --chain: the one_submission_variant) instead of two calls with the host between them (default)"""
    bench = _bench()
    wl = bench.Workload(pkg.synth)
    n = bench.KF_INTERVAL + 3          # crosses one LocalBA
    py = bench.HipBackend(pkg, wl, 0, pipeline=pipeline)
    py.fused = fused
    py.async_ba = async_ba
    try:
        last, ref = None, []
        for t in range(n):
            last, st = bench.run_steps_python(py, wl, t, 1, last, prefetch_beyond=True)
            ref.append(st)
    finally:
        py.close()
    cx = bench.HipBackend(pkg, wl, 0, pipeline=pipeline)
    cx.fused = fused
    cx.async_ba = async_ba
    cx.split = split
    cx.chain = chain
    cx.native = bench.NativeHost(pkg, cx, wl, pipeline=pipeline)
    try:
        got = [cx.native.run(t, 1, True) for t in range(n)]
        whole = None
    finally:
        cx.close()
    assert got == ref
    assert any("ba_chi2" in s for s in got) and got[-1]["m1"] > 500 and got[-1]["inliers"] > 500
    # one call over the whole range gives the same final state as frame-by-frame calls
    cx = bench.HipBackend(pkg, wl, 0, pipeline=pipeline)
    cx.fused = fused
    cx.async_ba = async_ba
    cx.split = split
    cx.chain = chain
    cx.native = bench.NativeHost(pkg, cx, wl, pipeline=pipeline)
    try:
        whole = cx.native.run(0, n, True)
    finally:
        cx.close()
    assert whole == ref[-1]


@pytest.mark.gpu
def test_cxx_host_bank_growth_and_map_copies(pkg):
    """The native host in its default split form, 4 frames from t = 0 (no LocalBA among them).
    Nine copies of ~2010 keypoints are more rows than a bank starts with, so both banks grow while the next frame is constructed inside
    the asd_prep_async bracket, beside a stage in flight: the per-frame statistics must be those of a context whose banks were grown
    beforehand (one row put at 140000 into each).  Like the bracket test of tests/test_banks.py this depends on timing: required to pass
    with the growth that waits for every stream, never run without it.
    asd_track_set_map_copies between two steps: the frame already prepared under the old count is prepared again -- 2 steps at 2 copies,
    the count set to 5, 2 more steps, against a handle that had the count set before each step with nothing prepared ahead."""
    bench = _bench()
    wl = bench.Workload(pkg.synth)
    frames = range(4)
    assert all(t % bench.KF_INTERVAL != bench.KF_INTERVAL - 1 for t in frames)

    def backend(pregrown):
        be = bench.HipBackend(pkg, wl, 0, pipeline=True)
        if pregrown:
            be.hip.bank_put(140000, np.zeros((1, 128), np.float32))
            be.hip.mpbank_put(140000, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.ones(1, np.float32), np.ones(1, np.float32))
        return be

    def with_handle(be, body):
        nh = bench.NativeHost(pkg, be, wl, pipeline=True)   # the defaults: fused, split-phase, two submissions per frame
        try:
            out = body(nh)
            nh.lib.asd_track_drain(nh.h)
            return out
        finally:
            nh.close()

    def nine_copies(nh):
        nh.lib.asd_track_set_map_copies(nh.h, 9)
        return [nh.run(t, 1, True) for t in frames]

    def copies_changed_between_steps(nh):
        out = [nh.run(t, 1, True) for t in (0, 1)]          # frame 2 is prepared under 2 copies when this returns
        nh.lib.asd_track_set_map_copies(nh.h, 5)
        return out + [nh.run(t, 1, True) for t in (2, 3)]

    def copies_set_before_each_step(nh):
        out = []
        for t, copies in zip(frames, (2, 2, 5, 5)):
            nh.lib.asd_track_set_map_copies(nh.h, copies)
            out.append(nh.run(t, 1, False))                  # no read-ahead, nothing prepared beyond frame t
        return out

    be = backend(False)
    try:
        fresh = with_handle(be, nine_copies)
    finally:
        be.close()
    be = backend(True)
    try:
        grown = with_handle(be, nine_copies)
        changed = with_handle(be, copies_changed_between_steps)
        stepwise = with_handle(be, copies_set_before_each_step)
    finally:
        be.close()
    assert fresh == grown
    assert all(s["m1"] > 500 and s["inliers"] > 500 for s in fresh[1:])
    assert fresh[-1]["m2"] > 0
    assert changed == stepwise
    assert all(s["m1"] > 500 and s["inliers"] > 500 for s in changed[1:])


@pytest.mark.gpu
def test_cxx_stereo_host_equals_python_stereo_host(pkg):
    """BASELINE configs[3] through the product's host path: libasdtrack in stereo mode (both extractors reading ahead, the right frame
    adopted device to device, asd_stereo_match on the kept pyramids during frame construction, one submission per frame) against the
    Python loop with sequential extractions: the same per-frame statistics, stereo matches included"""
    bench = _bench()
    wl = bench.EurocWorkload(pkg.synth)
    n = bench.KF_INTERVAL + 3
    py = bench.StereoBackend(pkg, wl, 0)
    try:
        last, ref = None, []
        for t in range(n):
            last, st = bench.stereo_steps(py, wl, t, 1, last)
            ref.append(st)
    finally:
        py.close()
    cx = bench.StereoBackend(pkg, wl, 0)
    cx.native = cx.native_host(pkg)
    try:
        got = [cx.native.run(t, 1, True) for t in range(n)]
        cx.native.lib.asd_track_drain(cx.native.h)
        cx.native.close()
        cx.native = None
    finally:
        cx.close()
    assert got == ref
    assert got[-1]["stereo_matched"] > 300 and got[-1]["m1"] > 300 and any("ba_chi2" in s for s in got)
