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
k_track_finish and k_raycast; us_per_iteration minus the first two is the host round trip of one iteration."""
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


if __name__ == "__main__":
    main()
