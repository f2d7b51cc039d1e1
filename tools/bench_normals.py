"""Scan-normal timing (include/mrhash_normals.h): the 128 x 1024 street-canyon scan (2 cm range noise) as the sensor delivers
it and the same points shuffled.  Prints one JSON line:

  organised / shuffled   us_per_estimate: mrh_estimate_normals_device + mrh_sync, median over >= 200 calls after a warm-up;
                         the counts of the estimate (mrh_normals_info)
  us_per_integrate       mrh_integrate_points + mrh_sync of that scan into a projective map, median: what estimating stands beside
  scans_per_s_estimate   a drive of scans through mrh_upload_points + mrh_estimate_normals + mrh_integrate_points, projective_sdf = False
  scans_per_s_upload     the same drive with mrh_upload_normals of host normals (the device's own, read back beforehand) instead
  fold                   MRH_NORMALS_FOLD of this run: 1 sums runs of equal cells inside the wave, 0 one set of atomics per point

usage: python tools/bench_normals.py [calls] [--only organised|shuffled]
Under `rocprofv3 --kernel-trace --stats -- python tools/bench_normals.py 200 --only organised` the per-kernel split is the four
k_normals_* rows."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 200
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
ROWS, COLS, NOISE, DRIVE = 128, 1024, 0.02, 24
hip = capi.load_hip()


def engine(**over):
    p = dict(synth.VBR_PARAMS, **over)
    e = capi.Engine(hip, capi.Params(num_sdf_blocks=262144, **p))
    e.set_camera(1.0, 1.0, 0.0, 0.0, 1, 1, p["min_depth"], 100.0, model=1)
    e.set_pose(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    return e


def time_estimates(e, pts):
    d_pts, d_out = hipmem.DeviceBuffer.from_numpy(pts), hipmem.DeviceBuffer(pts.nbytes)
    for _ in range(20):  # warm-up
        e.estimate_normals_device(d_pts.ptr, len(pts), d_out.ptr)
    e.sync()
    dt = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        e.estimate_normals_device(d_pts.ptr, len(pts), d_out.ptr)
        e.sync()
        dt.append(time.perf_counter() - t0)
    e.upload_points(pts)
    info = e.estimate_normals(info=True)
    return dict(us_per_estimate=round(float(np.median(dt) * 1e6), 1), us_min=round(float(np.min(dt) * 1e6), 1), **info)


def time_integrate(pts):
    e = engine()
    dt = []
    for i in range(20 + CALLS):
        e.upload_points(pts)
        t0 = time.perf_counter()
        e.integrate_points()
        e.sync()
        if i >= 20:
            dt.append(time.perf_counter() - t0)
    e.close()
    return round(float(np.median(dt) * 1e6), 1)


def drive_rate(scans, normals):
    """scans / s of the normal-direction SDF over the drive; normals = None: estimated on the device"""
    e = engine(projective_sdf=False)
    best = 0.0
    for rep in range(3):
        e.reset()
        e.sync()
        t0 = time.perf_counter()
        for k, (t, q, pts) in enumerate(scans):
            e.set_pose(synth.quat_to_rot(q), t)
            e.upload_points(pts)
            if normals is None:
                e.estimate_normals()
            else:
                e.upload_normals(normals[k])
            e.integrate_points()
        e.sync()
        best = max(best, len(scans) / (time.perf_counter() - t0))
    e.close()
    return round(best, 1)


def main():
    scene = synth.street_canyon()
    ident = (np.zeros(3, np.float32), np.array([0, 0, 0, 1], np.float32))
    pts = synth.lidar_scan(scene, *ident, rows=ROWS, cols=COLS, noise_sigma=NOISE, max_range=100.0)
    out = {"calls": CALLS, "rows": ROWS, "cols": COLS, "noise_sigma": NOISE, "fold": int(os.environ.get("MRH_NORMALS_FOLD", "1") != "0")}
    e = engine()
    if ONLY in (None, "organised"):
        out["organised"] = time_estimates(e, pts)
    if ONLY in (None, "shuffled"):
        out["shuffled"] = time_estimates(e, pts[np.random.default_rng(1).permutation(len(pts))])
    if ONLY is None:
        out["us_per_integrate"] = time_integrate(pts)
        rng = np.random.default_rng(0)
        scans = [(t, q, synth.lidar_scan(scene, t, q, rows=ROWS, cols=COLS, noise_sigma=NOISE, rng=rng)) for t, q in synth.drive_poses(DRIVE)]
        normals = []
        for _, _, p in scans:
            e.upload_points(p)
            e.estimate_normals()
            normals.append(e.get_normals()[0])
        out["drive_scans"] = DRIVE
        out["scans_per_s_estimate"] = drive_rate(scans, None)
        out["scans_per_s_upload"] = drive_rate(scans, normals)
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
