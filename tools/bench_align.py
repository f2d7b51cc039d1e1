"""Map-to-map registration timing (include/mrhash_align.h): the two Replica maps of examples/align_maps_synthetic.py —
frames 0-9 of the stand-in stream in map A, frames 10-19 in map B, whose frame is displaced by 0.35 rad about (0.2, 1, -0.3) and
(0.4, -0.25, 0.15) m — aligned from a start 2.3 degrees and 52 mm off.  Prints one JSON line:

  call_us          mrh_align_map with the default 10 iterations (blocking: selection, gather, 10 x (linearise, finish, read-back,
                   solve)), median over CALLS calls after a warm-up
  one_us           the same with iterations = 1: the gather and one linearisation
  iteration_us     (call_us - one_us) / 9: one linearisation with its reduction, read-back and solve
  source_blocks, samples, accepted, rms_mm, status, deg, mm (the error of the result against the known displacement)

The phases — k_select_blocks, k_align_gather (count, emit), the scan, k_align_linearise, k_track_finish — are the kernel rows of
`rocprofv3 --kernel-trace --stats -- python tools/bench_align.py 10`, a run of its own."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, synth  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(_pos[0]) if _pos else 50
K = synth.REPLICA_640


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


T_R, T_T = rotation((0.2, 1.0, -0.3), 0.35), np.array([0.4, -0.25, 0.15])
START_R, START_T = rotation((1, -2, 0.5), 0.04) @ T_R, T_T + np.array([0.03, -0.03, 0.03])


def median_us(fn):
    for _ in range(3):  # warm-up: the buffers grow on the first call
        fn()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()  # every call timed here blocks
        t.append(time.perf_counter() - t0)
    return round(float(np.median(t) * 1e6), 1)


def main():
    hip = capi.load_hip()
    p = capi.Params(num_sdf_blocks=131072, **synth.REPLICA_PARAMS)
    a, b = capi.Engine(hip, p), capi.Engine(hip, p)
    for i, f in enumerate(synth.replica_stream(20)):
        e = a if i < 10 else b
        e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
        if i < 10:
            e.set_pose(f.R, f.t)
        else:  # the same camera poses, expressed in B's frame: T^-1 o pose
            e.set_pose(T_R.T @ f.R.astype(np.float64), T_R.T @ (f.t.astype(np.float64) - T_T))
        e.upload_depth(f.depth)
        e.upload_rgb(f.rgb)
        e.integrate()
    a.sync()
    b.sync()
    R, t, info = a.align_map(b, START_R, START_T)
    ang = np.degrees(np.arccos(np.clip((np.trace(R.astype(np.float64) @ T_R.T) - 1) / 2, -1, 1)))
    out = dict(calls=CALLS, **{k: info[k] for k in ("source_blocks", "samples", "accepted", "status", "iterations_done")}, rms_mm=round(1e3 * info["rms"], 4),
               deg=round(float(ang), 4), mm=round(1e3 * float(np.linalg.norm(t - T_T)), 3))
    out["call_us"] = median_us(lambda: a.align_map(b, START_R, START_T))
    out["one_us"] = median_us(lambda: a.align_map(b, START_R, START_T, iterations=1))
    out["iteration_us"] = round((out["call_us"] - out["one_us"]) / 9, 1)
    for e in (a, b):
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
