"""Render-free tracking against the rendering trackers (include/mrhash_sdftrack.h), in one process on the two
workloads of tools/bench_track.py:

  depth   the 640 x 480 frame of orbit pose 20 tracked from pose 19 against the Replica stand-in after 20 fused frames:
          mrh_track_depth_device against mrh_track_depth_sdf_device, same frame, same start
  scan    a 128 x 1024 scan (131 072 points) 0.32 m and 1 degree of yaw from the last pose of the street fused from five range images
          at 20 cm voxels and a 4-voxel truncation: mrh_track_scan_device (128 x 1024 model) against mrh_track_points_sdf_device

Every timed call blocks (the solve is on the host), so a host clock around the call is the call's time.  Prints one JSON line with,
per leg and per tracker (`icp`: the rendering one, `sdf`: the render-free one):

  us_10, us_1        the call at 10 iterations and at 1, median over CALLS calls after a warm-up of 10
  us_iteration       (us_10 - us_1) / 9: one linearisation, its reduction, the read-back, the host's solve and update
  us_setup           us_1 - us_iteration: argument checks, the pipeline restart and — for icp — the one model render
  us_10_host         the host-input entry point (pinned staging) at 10 iterations
  pixels, rms_m, status, translation_error_m, rotation_error_deg   of the 10-iteration result against the true pose
and, per leg, the start's own errors and `sdf_pixels_at_the_start`: the samples inside the band at the first linearisation.

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_sdftrack.py 50`, a run of its own, the kernels' own times are the rows
of k_sdftrack_depth_linearise, k_sdftrack_points_linearise, k_track_linearise, k_track_scan_linearise, k_track_finish and k_raycast.

`--depth-only` / `--scan-only` run one leg; `--probe` prints the render-free tracker's result on the scan leg at other iteration counts
and bands (scan_probe)."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(_pos[0]) if _pos else 50


def median_us(fn, n=None):
    for _ in range(10):  # warm-up: the buffers grow on the first call
        fn()
    out = []
    for _ in range(n or CALLS):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out) * 1e6)


def errors(R, t, R_true, t_true):
    try:
        import track_ref
    except ImportError:
        return {}
    dt, dr = track_ref.pose_errors(R, t, R_true, t_true)
    return dict(translation_error_m=round(dt, 6), rotation_error_deg=round(dr, 5))


def leg(call, call_host, R_true, t_true):
    """call(iterations) / call_host(iterations) -> (R, t, info)."""
    t10 = median_us(lambda: call(10))
    t1 = median_us(lambda: call(1))
    t10b = median_us(lambda: call(10))  # again, behind the 1-iteration leg: the spread of the same command
    th = median_us(lambda: call_host(10))
    R, t, info = call(10)
    it = (t10 - t1) / 9
    return dict(us_10=round(t10, 1), us_10_again=round(t10b, 1), us_1=round(t1, 1), us_iteration=round(it, 1), us_setup=round(t1 - it, 1), us_10_host=round(th, 1),
                status=info["status"], iterations_done=info["iterations_done"], pixels=info["pixels"], rms_m=round(info["rms"], 6), **errors(R, t, R_true, t_true))


def depth_leg(hip):
    K = synth.REPLICA_640
    near, far = 0.1, 8.0
    p = capi.Params(num_sdf_blocks=262144, **synth.REPLICA_PARAMS)
    e = capi.Engine(hip, p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    for f in synth.replica_stream(20):
        e.set_pose(f.R, f.t)
        e.upload_depth(f.depth)
        e.upload_rgb(f.rgb)
        e.integrate()
    e.sync()
    poses = synth.orbit_poses(21)
    R19, t19 = synth.quat_to_rot(poses[19][1]), poses[19][0]
    f20 = synth.render(synth.replica_room(), K, *poses[20], depth_scaling=6553.5)
    cam = (K.fx, K.fy, K.cx, K.cy, K.rows, K.cols)
    d_depth = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(f20.depth, np.float32))
    out = dict(rows=K.rows, cols=K.cols, min_depth=near, max_depth=far, blocks=int(e.stats().occupied_fine), band_m=synth.REPLICA_PARAMS["sdf_truncation"],
               start=errors(R19, t19, f20.R, f20.t))
    out["icp"] = leg(lambda it: e.track_depth_device(d_depth.ptr, *cam, R19, t19, near, far, iterations=it),
                     lambda it: e.track_depth(f20.depth, *cam, R19, t19, near, far, iterations=it), f20.R, f20.t)
    out["sdf"] = leg(lambda it: e.track_depth_sdf_device(d_depth.ptr, *cam, R19, t19, near, far, iterations=it),
                     lambda it: e.track_depth_sdf(f20.depth, *cam, R19, t19, near, far, iterations=it), f20.R, f20.t)
    out["sdf_pixels_at_the_start"] = e.track_depth_sdf_device(d_depth.ptr, *cam, R19, t19, near, far, iterations=1)[2]["pixels"]
    # the render-free tracker started where the rendering one ends, and the other way round: what either leaves of the other's result
    R, t, _ = e.track_depth_device(d_depth.ptr, *cam, R19, t19, near, far)
    R2, t2, info2 = e.track_depth_sdf_device(d_depth.ptr, *cam, R, t, near, far)
    out["sdf_from_icp_result"] = dict(pixels=info2["pixels"], rms_m=round(info2["rms"], 6), **errors(R2, t2, f20.R, f20.t))
    e.close()
    return out


def street(hip):
    """The street map and the scan of the scan leg: (engine, points, start R0, t0, truth R1, t1, near, far, model camera, params)."""
    params = dict(synth.VBR_PARAMS, min_weight_threshold=1, sdf_truncation=0.8)
    near, far = params["min_depth"], 60.0
    cam_in = synth.spherical_camera(64, 512)
    c = synth.spherical_camera(128, 1024)
    cam = (c["fx"], c["fy"], c["cx"], c["cy"], c["rows"], c["cols"])
    scene = synth.street_canyon()
    e = capi.Engine(hip, capi.Params(num_sdf_blocks=131072, **params))
    e.set_camera(cam_in["fx"], cam_in["fy"], cam_in["cx"], cam_in["cy"], 64, 512, near, far, model=1)
    poses = synth.drive_poses(5, step=1.0)
    for t, q in poses:
        depth, rgb = synth.spherical_range_image(scene, t, q, cam_in)
        e.set_pose(synth.quat_to_rot(q), t)
        e.upload_depth(depth)
        e.upload_rgb(rgb)
        e.integrate()
    e.sync()
    t0, q0 = poses[-1]
    R0 = synth.quat_to_rot(q0)
    yaw = np.deg2rad(1.0)
    q1 = np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])
    R1 = R0.astype(np.float64) @ synth.quat_to_rot(q1).astype(np.float64)
    t1 = np.asarray(t0, np.float64) + np.array([0.25, 0.2, 0.0])
    d = synth.lidar_dirs(128, 1024)
    rng, _ = scene.cast_dirs(d, R1, t1)
    pts = d * rng[:, None]
    pts[~np.isfinite(rng) | (rng > far) | (rng <= 0)] = 0.0
    pts = np.ascontiguousarray(pts, np.float32)
    return e, pts, R0, t0, R1, t1, near, far, cam, params, c


def scan_leg(hip):
    e, pts, R0, t0, R1, t1, near, far, cam, params, c = street(hip)
    n = len(pts)
    d_pts = hipmem.DeviceBuffer.from_numpy(pts)
    d_shuf = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(pts[np.random.default_rng(0).permutation(n)]))
    out = dict(points=n, valid_points=int(np.count_nonzero(np.any(pts != 0, axis=1))), rows=c["rows"], cols=c["cols"], min_depth=near, max_depth=far,
               blocks=int(e.stats().occupied_fine), band_m=params["sdf_truncation"], start=errors(R0, t0, R1, t1))
    out["icp"] = leg(lambda it: e.track_scan_device(d_pts.ptr, n, *cam, R0, t0, near, far, iterations=it),
                     lambda it: e.track_scan(pts, *cam, R0, t0, near, far, iterations=it), R1, t1)
    out["sdf"] = leg(lambda it: e.track_points_sdf_device(d_pts.ptr, n, R0, t0, near, far, iterations=it),
                     lambda it: e.track_points_sdf(pts, R0, t0, near, far, iterations=it), R1, t1)
    s10 = median_us(lambda: e.track_points_sdf_device(d_shuf.ptr, n, R0, t0, near, far, iterations=10))
    s1 = median_us(lambda: e.track_points_sdf_device(d_shuf.ptr, n, R0, t0, near, far, iterations=1))
    a, b = e.track_points_sdf_device(d_pts.ptr, n, R0, t0, near, far), e.track_points_sdf_device(d_shuf.ptr, n, R0, t0, near, far)
    out["sdf_shuffled"] = dict(us_10=round(s10, 1), us_iteration=round((s10 - s1) / 9, 1),
                               same_bits=bool(np.array_equal(a[2]["sums"], b[2]["sums"]) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()))
    out["sdf_pixels_at_the_start"] = e.track_points_sdf_device(d_pts.ptr, n, R0, t0, near, far, iterations=1)[2]["pixels"]
    e.close()
    return out


def scan_probe(hip):
    """--probe: the render-free tracker on the scan leg at 1 .. 64 iterations and three bands, and from the truth: one line each with
    the accepted points, the rms and the error against the true pose (t - t_true last)."""
    import track_ref

    e, pts, R0, t0, R1, t1, near, far, _, _, _ = street(hip)
    for band in (0.0, 0.6, 0.4):
        for it in (1, 3, 10, 20, 40, 64):
            R, t, info = e.track_points_sdf(pts, R0, t0, near, far, band=band, iterations=it)
            print("band", band, "iterations", it, "status", info["status"], "points", info["pixels"], "rms %.4f" % info["rms"],
                  "error %.4f m %.4f deg" % track_ref.pose_errors(R, t, R1, t1), "dt", np.round(t - t1, 3))
    R, t, info = e.track_points_sdf(pts, R1.astype(np.float32), t1.astype(np.float32), near, far)
    print("from the truth: points", info["pixels"], "error %.4f m %.4f deg" % track_ref.pose_errors(R, t, R1, t1), "dt", np.round(t - t1, 3))
    e.close()


def main():
    hip = capi.load_hip()
    if "--probe" in sys.argv:
        return scan_probe(hip)
    out = dict(calls=CALLS)
    if "--scan-only" not in sys.argv:
        out["depth"] = depth_leg(hip)
    if "--depth-only" not in sys.argv:
        out["scan"] = scan_leg(hip)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
