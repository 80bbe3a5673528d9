"""cv::undistort in front of the extractor (Tracking.cc:104,125; asd_undistort_map / asd_set_undistortion / asd_undistort).

CPU: the host map builder against tests/undistort_ref.py (every int16 and uint16 equal) at the EuRoC coefficients, an odd size
whose stripe height does not divide the rows, a strong tangential case that sends map entries outside the image, and the three
KITTI intrinsics with zero coefficients (the identity).  GPU: k_undistort against the numpy remap byte for byte from device,
pinned and pageable sources; extractions with the map set against extractions of the numpy-undistorted image on a context
without one (synchronous and pipelined); zero coefficients and set / clear; the error paths; asd_replay with an EuRoC camera file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import undistort_ref as R

EUROC_K = (458.654, 457.296, 367.215, 248.375)                          # cameraconfig/MH_EUROC/EuRoC_config.txt
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
KITTI_K = [(718.856, 718.856, 607.1928, 185.2157), (721.5377, 721.5377, 609.5593, 172.854),
           (707.0912, 707.09127, 601.8873, 183.1104)]                    # cameraconfig/KITTI/*.txt, coefficients 0
W, H = 752, 480
TOOL = os.path.join(ROOT, "asd-slam_amd", "host", "asd_replay")


def _map(pkg, K, d, w, h):
    return pkg.capi.undistort_map(K, d, w, h)


# ---------------------------------------------------------------- CPU: the map pair
@pytest.mark.parametrize("K,d,w,h", [(EUROC_K, EUROC_D, W, H), (EUROC_K, EUROC_D, 641, 361)], ids=["euroc_752x480", "euroc_641x361"])
def test_map_equals_numpy_reference(pkg, K, d, w, h):
    xy, frac = _map(pkg, K, d, w, h)
    rxy, rfrac = R.undistort_map(K, d, w, h)
    assert xy.dtype == np.int16 and frac.dtype == np.uint16 and xy.shape == (h, w, 2) and frac.shape == (h, w)
    np.testing.assert_array_equal(xy, rxy)
    np.testing.assert_array_equal(frac, rfrac)
    if w == 641:
        assert h % min(max(1, 4096 // w), h) != 0      # the last stripe is shorter
    assert frac.max() < 1024 and np.any(frac != 0)


def test_map_with_entries_outside_the_image(pkg):
    K, d, w, h = (300.0, 310.0, 320.5, 180.25), (0.3, 0.1, 0.1, -0.1), 641, 361
    xy, frac = _map(pkg, K, d, w, h)
    rxy, rfrac = R.undistort_map(K, d, w, h)
    np.testing.assert_array_equal(xy, rxy)
    np.testing.assert_array_equal(frac, rfrac)
    assert (xy[..., 0] < 0).any() and (xy[..., 0] >= w).any() and (xy[..., 1] < 0).any() and (xy[..., 1] >= h).any()
    # the remap of such a map has a zero border where the whole neighbourhood is outside
    img = np.full((h, w), 200, np.uint8)
    out = R.remap(img, xy, frac)
    outside = (xy[..., 0] < -1) | (xy[..., 0] >= w) | (xy[..., 1] < -1) | (xy[..., 1] >= h)
    assert outside.any() and (out[outside] == 0).all()


@pytest.mark.parametrize("K", KITTI_K, ids=["kitti00-02", "kitti03", "kitti04-12"])
def test_zero_coefficients_give_the_identity(pkg, K):
    w, h = 1241, 376
    for d in ((0, 0, 0, 0), None):
        xy, frac = _map(pkg, K, d, w, h)
        jj, ii = np.meshgrid(np.arange(w), np.arange(h))
        np.testing.assert_array_equal(xy[..., 0], jj)
        np.testing.assert_array_equal(xy[..., 1], ii)
        assert not frac.any()
    rxy, rfrac = R.undistort_map(K, (0, 0, 0, 0), w, h)
    np.testing.assert_array_equal(xy, rxy)
    np.testing.assert_array_equal(frac, rfrac)


def test_map_refuses_bad_arguments(pkg):
    lib = pkg.capi.load_library()
    K = np.array(EUROC_K, np.float32)
    d = np.array(EUROC_D, np.float32)
    xy = np.empty((4, 4, 2), np.int16)
    fr = np.empty((4, 4), np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for w, h in ((0, 4), (4, 0), (-3, 4), (4, -1)):
        assert lib.asd_undistort_map(p(K), p(d), w, h, p(xy), p(fr)) == -1
    assert lib.asd_undistort_map(p(K), p(d), 4, 4, None, p(fr)) == -1
    assert lib.asd_undistort_map(p(K), p(d), 4, 4, p(xy), None) == -1
    assert lib.asd_undistort_map(None, p(d), 4, 4, p(xy), p(fr)) == -1
    assert lib.asd_undistort_map(p(np.zeros(4, np.float32)), p(d), 4, 4, p(xy), p(fr)) == -1   # singular camera matrix
    assert lib.asd_undistort_map(p(K), p(d), 4, 4, p(xy), p(fr)) == 0


def test_remap_reference_properties():
    """The fixed-point weights sum to 2^15: a constant image stays constant where the neighbourhood is inside, and a = b = 0
    returns the source pixel."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (20, 30), dtype=np.uint8)
    jj, ii = np.meshgrid(np.arange(30), np.arange(20))
    xy = np.stack([jj, ii], -1).astype(np.int16)
    np.testing.assert_array_equal(R.remap(img, xy, np.zeros((20, 30), np.uint16)), img)
    frac = rng.integers(0, 1024, (20, 30)).astype(np.uint16)
    out = R.remap(np.full((20, 30), 77, np.uint8), xy, frac)
    assert (out[:-1, :-1] == 77).all()


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctxs(pkg, synth):
    """two contexts at the EuRoC size: `und` gets the map, `plain` never does"""
    a = pkg.AsdHip(n_features=1000, max_width=W, max_height=H, max_patches=4096)
    b = pkg.AsdHip(n_features=1000, max_width=W, max_height=H, max_patches=4096)
    try:
        for c in (a, b):
            c.load_weights(synth.asdnet_weights(0))
        yield a, b
    finally:
        a.close()
        b.close()


def _frame(synth, t):
    return synth.scene_frame(t, w=W, h=H)


def _strided(img, stride):
    buf = np.full((img.shape[0], stride), 0xA5, np.uint8)
    buf[:, :img.shape[1]] = img
    return buf


def _assert_same(k1, d1, k2, d2, what):
    assert len(k1) == len(k2), (what, len(k1), len(k2))
    for f in ("x", "y", "angle", "response", "octave", "size"):
        assert np.array_equal(k1[f], k2[f]), (what, f)
    np.testing.assert_array_equal(d1, d2, err_msg=what)


@pytest.mark.gpu
def test_undistort_equals_numpy_from_every_source(ctxs, synth):
    und, _ = ctxs
    und.set_undistortion(EUROC_K, EUROC_D, W, H)
    try:
        img = _frame(synth, 3)
        ref = R.undistort(img, EUROC_K, EUROC_D)
        assert not np.array_equal(ref, img)
        stride = W + 40
        buf = _strided(img, stride)
        # pageable: a strided view of a wider host array
        np.testing.assert_array_equal(und.undistort(buf[:, :W]), ref)
        # pinned
        hp = und.host_alloc(buf.nbytes)
        dp = und.device_alloc(buf.nbytes)
        try:
            C.memmove(hp.value, buf.ctypes.data, buf.nbytes)
            hv = np.frombuffer((C.c_uint8 * buf.nbytes).from_address(hp.value), np.uint8).reshape(H, stride)
            np.testing.assert_array_equal(und.undistort(hv[:, :W]), ref)
            # device-resident, read in place
            und.h2d(dp, buf)
            np.testing.assert_array_equal(und.undistort(dp, device_resident=True, w=W, h=H, stride=stride), ref)
        finally:
            und.device_free(dp)
            und.lib.asd_host_free(und.ctx, hp)
    finally:
        und.set_undistortion(None, None, W, H)


@pytest.mark.gpu
def test_extraction_runs_on_the_undistorted_image(ctxs, synth):
    und, plain = ctxs
    und.set_undistortion(EUROC_K, EUROC_D, W, H)
    try:
        frames = [_frame(synth, t) for t in (5, 6, 7)]
        refs = [R.undistort(f, EUROC_K, EUROC_D) for f in frames]
        expect = []
        for r in refs:
            k, d = plain.extract(r)
            expect.append((k.copy(), d.copy()))
        # synchronous, pageable source
        k, d = und.extract(frames[0])
        np.testing.assert_array_equal(und.level_image(0), refs[0])
        _assert_same(k, d, *expect[0], "asd_extract")
        # synchronous, device source with stride > width
        stride = W + 64
        buf = _strided(frames[1], stride)
        dp = und.device_alloc(buf.nbytes)
        try:
            und.h2d(dp, buf)
            k, d = und.extract_device(dp, W, H, stride)
            _assert_same(k.copy(), d.copy(), *expect[1], "asd_extract_device")
            np.testing.assert_array_equal(und.level_image(0), refs[1])
            # pipelined: ASD_EXTRACT_QUEUE submissions outstanding, device / pinned / pageable sources
            bufs = [_strided(f, stride) for f in frames]
            hp = und.host_alloc(bufs[1].nbytes)
            try:
                C.memmove(hp.value, bufs[1].ctypes.data, bufs[1].nbytes)
                und.h2d(dp, bufs[0])
                und.extract_submit(dp, W, H, stride, device_resident=True)
                und.extract_submit(hp, W, H, stride, device_resident=False)
                und.extract_submit(C.c_void_p(bufs[2].ctypes.data), W, H, stride, device_resident=False)
                for i in range(3):
                    k, d = und.extract_wait(view=True)
                    _assert_same(k, d, *expect[i], f"asd_extract_submit {i}")
            finally:
                und.lib.asd_host_free(und.ctx, hp)
        finally:
            und.device_free(dp)
    finally:
        und.set_undistortion(None, None, W, H)


@pytest.mark.gpu
def test_zero_coefficients_and_clear_change_nothing(ctxs, synth):
    und, plain = ctxs
    img = _frame(synth, 9)
    k0, d0 = plain.extract(img)
    k0, d0 = k0.copy(), d0.copy()
    und.set_undistortion(EUROC_K, (0, 0, 0, 0), W, H)             # zero coefficients: no map
    k, d = und.extract(img)
    _assert_same(k, d, k0, d0, "zero coefficients")
    und.set_undistortion(EUROC_K, EUROC_D, W, H)
    k, d = und.extract(img)
    assert not np.array_equal(und.level_image(0), img)
    und.set_undistortion(EUROC_K, None, W, H)                    # clear
    k, d = und.extract(img)
    _assert_same(k, d, k0, d0, "after a clear")
    np.testing.assert_array_equal(und.level_image(0), img)
    with pytest.raises(Exception):
        und.undistort(img)                                        # no map: refused


@pytest.mark.gpu
def test_undistortion_error_paths_leave_the_context_usable(ctxs, synth, pkg):
    und, plain = ctxs
    img = _frame(synth, 11)
    ref = R.undistort(img, EUROC_K, EUROC_D)
    und.set_undistortion(EUROC_K, EUROC_D, W, H)
    try:
        # another size than the map's
        small = np.ascontiguousarray(img[:400, :700])
        with pytest.raises(pkg.AsdError) as e:
            und.extract(small)
        assert e.value.code == -1 and "undistortion map" in str(e.value)
        with pytest.raises(pkg.AsdError) as e:
            und.extract_submit(C.c_void_p(small.ctypes.data), 700, 400, 700, device_resident=False)
        assert e.value.code == -1
        # over capacity
        with pytest.raises(pkg.AsdError) as e:
            und.set_undistortion(EUROC_K, EUROC_D, W + 1, H)
        assert e.value.code == -5
        # set while submissions are outstanding
        und.extract_submit(C.c_void_p(img.ctypes.data), W, H, W, device_resident=False)
        with pytest.raises(pkg.AsdError) as e:
            und.set_undistortion(EUROC_K, None, W, H)
        assert e.value.code == -1 and "outstanding" in str(e.value)
        k, d = und.extract_wait()
        k, d = k.copy(), d.copy()
        # the map in place is the EuRoC one and still works
        k2, d2 = plain.extract(ref)
        _assert_same(k, d, k2, d2, "after the refused calls")
        np.testing.assert_array_equal(und.undistort(img), ref)
    finally:
        und.set_undistortion(None, None, W, H)


def _write_sequence(tmp, synth, frames, name, K, d):
    seq = tmp / name
    (seq / "image_0").mkdir(parents=True)
    with open(seq / "times.txt", "w") as f:
        for t in range(len(frames)):
            f.write(f"{0.05 * t:.6e}\n")
    for t, im in enumerate(frames):
        with open(seq / "image_0" / f"{t:06d}.pgm", "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.tobytes())
    cam = tmp / f"{name}_cam.txt"
    cam.write_text(", ".join(repr(float(v)) for v in tuple(K) + tuple(d)) + "\n")
    return str(seq), str(cam)


@pytest.mark.gpu
def test_replay_tool_undistorts_like_tracking(tmp_path, synth):
    assert os.path.exists(TOOL), "asd_replay not built: run __graft_entry__.build()"
    frames = [_frame(synth, 20 + t) for t in range(4)]
    weights = tmp_path / "weights.bin"
    with open(weights, "wb") as f:
        for w, m, v in synth.asdnet_weights(0):
            f.write(np.ascontiguousarray(w, np.float32).tobytes() + np.ascontiguousarray(m, np.float32).tobytes() +
                    np.ascontiguousarray(v, np.float32).tobytes())
    seq_raw, cam_euroc = _write_sequence(tmp_path, synth, frames, "raw", EUROC_K, EUROC_D)
    seq_und, cam_zero = _write_sequence(tmp_path, synth, [R.undistort(f, EUROC_K, EUROC_D) for f in frames], "und", EUROC_K,
                                        (0, 0, 0, 0))
    counts = []
    for seq, cam in ((seq_raw, cam_euroc), (seq_und, cam_zero), (seq_raw, cam_zero)):
        stats = str(tmp_path / "stats.csv")
        p = subprocess.run([TOOL, seq, cam, str(weights), "--stats", stats], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        rows = [l.strip().split(",") for l in open(stats).read().splitlines()[1:]]
        assert len(rows) == len(frames)
        counts.append([(r[2], r[3]) for r in rows])
    assert counts[0] == counts[1]
    assert counts[0] != counts[2]      # the raw images without the map are a different sequence
