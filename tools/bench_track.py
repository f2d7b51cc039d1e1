"""Tracking timing (include/mrhash_track.h): the 640x480 frame of orbit pose 20 tracked from pose 19 against the
Replica stand-in after 20 fused frames.  Every timed call blocks (the solve is on the host), so a host clock around the call is
the call's time.  Prints one JSON line:

  us_per_call_10        mrh_track_depth_device at 10 iterations, median over CALLS calls after a warm-up
  us_per_call_1         the same at 1 iteration
  us_per_call_10_host   mrh_track_depth (host image through pinned staging) at 10 iterations
  us_per_iteration      (us_per_call_10 - us_per_call_1) / 9: k_track_linearise + k_track_finish + the read-back and the host's
                        solve and update
  us_render_and_setup   us_per_call_1 - us_per_iteration: argument checks, the pipeline restart and the one model render
  us_render_alone       mrh_raycast_device (depth + normals) + mrh_sync at the same pose, for comparison
  translation_error_m, rotation_error_deg, pixels, rms_m   of the 10-iteration result against the true pose

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_track.py` the kernels' own times are the rows of k_track_linearise,
k_track_finish and k_raycast; us_per_iteration minus the first two is the host round trip of one iteration.

`python tools/bench_track.py [CALLS] --scan` times scan tracking instead: see scan_main."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(_pos[0]) if _pos else 200
K = synth.REPLICA_640
NEAR, FAR = 0.1, 8.0


def median_us(fn, n):
    for _ in range(10):  # warm-up
        fn()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out) * 1e6), float(np.quantile(out, 0.9) * 1e6)


def main():
    hip = capi.load_hip()
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
    n = K.rows * K.cols
    d_depth = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(f20.depth, np.float32))
    bufs = (hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n))

    def call(iterations):
        return e.track_depth_device(d_depth.ptr, *cam, R19, t19, NEAR, FAR, iterations=iterations)

    def render():
        e.raycast_device(*cam, R19, t19, NEAR, FAR, d_depth=bufs[0].ptr, d_normals=bufs[1].ptr)
        e.sync()

    t10, t10_p90 = median_us(lambda: call(10), CALLS)
    t1, _ = median_us(lambda: call(1), CALLS)
    t10b, _ = median_us(lambda: call(10), CALLS)  # again, behind the 1-iteration leg: the spread of the same command
    th, _ = median_us(lambda: e.track_depth(f20.depth, *cam, R19, t19, NEAR, FAR, iterations=10), CALLS)
    tr_, _ = median_us(render, CALLS)
    R, t, info = call(10)
    out = dict(calls=CALLS, rows=K.rows, cols=K.cols, min_depth=NEAR, max_depth=FAR, blocks=int(e.stats().occupied_fine),
               us_per_call_10=round(t10, 1), us_per_call_10_p90=round(t10_p90, 1), us_per_call_10_again=round(t10b, 1), us_per_call_1=round(t1, 1),
               us_per_call_10_host=round(th, 1), us_per_iteration=round((t10 - t1) / 9, 1), us_render_and_setup=round(t1 - (t10 - t1) / 9, 1),
               us_render_alone=round(tr_, 1), status=info["status"], pixels=info["pixels"], rms_m=round(info["rms"], 6),
               largest_sum_log2=round(float(np.log2(np.abs(info["sums"]).max())), 2))
    try:
        import track_ref

        dt, dr = track_ref.pose_errors(R, t, f20.R, f20.t)
        out.update(translation_error_m=round(dt, 6), rotation_error_deg=round(dr, 5))
    except ImportError:
        pass
    e.close()
    print(json.dumps(out))


def scan_main():
    """--scan: a 128 x 1024 scan (131 072 points) tracked against a 128 x 1024 spherical render of the street:
    five 64 x 512 range images one metre apart fused at 20 cm voxels and a 4-voxel truncation, the scan taken 0.32 m and 1 degree
    of yaw away from the last pose.  The same fields as the depth leg (mrh_track_scan_device / mrh_track_scan), plus
    us_per_iteration_shuffled for the same cloud in a seeded random order (the gathers from the model images scatter)."""
    hip = capi.load_hip()
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
    n = len(pts)
    d_pts = hipmem.DeviceBuffer.from_numpy(pts)
    d_shuf = hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(pts[np.random.default_rng(0).permutation(n)]))
    npix = c["rows"] * c["cols"]
    bufs = (hipmem.DeviceBuffer(4 * npix), hipmem.DeviceBuffer(12 * npix), hipmem.DeviceBuffer(12 * npix))

    def call(buf, iterations):
        return e.track_scan_device(buf.ptr, n, *cam, R0, t0, near, far, iterations=iterations)

    def render():
        e.raycast_spherical_device(*cam, R0, t0, near, far, d_range=bufs[0].ptr, d_normals=bufs[1].ptr, d_points=bufs[2].ptr)
        e.sync()

    t10, t10_p90 = median_us(lambda: call(d_pts, 10), CALLS)
    t1_, _ = median_us(lambda: call(d_pts, 1), CALLS)
    t10b, _ = median_us(lambda: call(d_pts, 10), CALLS)
    s10, _ = median_us(lambda: call(d_shuf, 10), CALLS)
    s1_, _ = median_us(lambda: call(d_shuf, 1), CALLS)
    th, _ = median_us(lambda: e.track_scan(pts, *cam, R0, t0, near, far, iterations=10), CALLS)
    tr_, _ = median_us(render, CALLS)
    R, t, info = call(d_pts, 10)
    Rs, ts_, infos = call(d_shuf, 10)
    out = dict(leg="scan", calls=CALLS, points=n, rows=c["rows"], cols=c["cols"], min_depth=near, max_depth=far, blocks=int(e.stats().occupied_fine),
               us_per_call_10=round(t10, 1), us_per_call_10_p90=round(t10_p90, 1), us_per_call_10_again=round(t10b, 1), us_per_call_1=round(t1_, 1),
               us_per_call_10_host=round(th, 1), us_per_iteration=round((t10 - t1_) / 9, 1), us_render_and_setup=round(t1_ - (t10 - t1_) / 9, 1),
               us_per_call_10_shuffled=round(s10, 1), us_per_iteration_shuffled=round((s10 - s1_) / 9, 1),
               us_render_alone=round(tr_, 1), status=info["status"], pixels=info["pixels"], rms_m=round(info["rms"], 6),
               shuffled_same_bits=bool(np.array_equal(info["sums"], infos["sums"]) and R.tobytes() == Rs.tobytes() and t.tobytes() == ts_.tobytes()),
               largest_sum_log2=round(float(np.log2(np.abs(info["sums"]).max())), 2))
    try:
        import track_ref

        dt0, dr0 = track_ref.pose_errors(R0, t0, R1, t1)
        dt, dr = track_ref.pose_errors(R, t, R1, t1)
        out.update(initial_translation_error_m=round(dt0, 6), initial_rotation_error_deg=round(dr0, 5), translation_error_m=round(dt, 6),
                   rotation_error_deg=round(dr, 5))
    except ImportError:
        pass
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    scan_main() if "--scan" in sys.argv[1:] else main()
