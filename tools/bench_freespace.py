"""The free-space layer (include/mrhash_freespace.h) in one process, on the two maps of the other reader benchmarks.

  room     the 20-frame synthetic Replica stream at 640 x 480, 1 cm voxels, fused; a layer of 128^3 cells at s = 3 (8 cm cells,
           10.24 m per side) around the orbit
    carve_empty      mrh_freespace_carve_depth_device of the last frame into a cleared layer: every word a ray meets first needs its atomic
    carve_saturated  the same frame again, after all 20 frames were carved: every word is already set, the kernel only loads
    raycast          mrh_raycast_device of the same camera from the last pose: a yardstick (k_raycast)
    integrate        one more mrh_integrate of the last frame + mrh_sync: a yardstick (k_front + k_back)
    box              mrh_freespace_box_device of 256 x 256 x 128 cells around the layer
    segments         mrh_freespace_segments_device of 2^17 random segments of up to 2 m inside the layer
  street   the five-scan street of tools/bench_rays.py at 20 cm voxels; a layer of 128 x 128 x 32 cells at s = 3 (1.6 m cells)
    scan_empty / scan_saturated  mrh_freespace_carve_points_device of the 131 072 points the 128 x 1024 spherical camera returns
           from the last pose, into a cleared layer and again

Every timed call is the device form followed by mrh_sync, a host clock around both (the empty legs clear the layer and sync before
the clock starts); the median over CALLS calls after a warm-up of 10.  Prints one JSON line.  `--legs a,b` runs only the named
legs, so that under `rocprofv3 --kernel-trace --stats -- python tools/bench_freespace.py 20 --legs carve_empty`, a run of its own,
the row of k_freespace_carve is that leg's alone."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

_ap = argparse.ArgumentParser()
_ap.add_argument("calls", type=int, nargs="?", default=50)
_ap.add_argument("--legs", default="")
_args = _ap.parse_args()
CALLS = _args.calls
LEGS = set(_args.legs.split(",")) if _args.legs else None
F = np.float32


def wanted(leg):
    return LEGS is None or leg in LEGS


def median_us(fn, before=None):
    out = []
    for i in range(10 + CALLS):  # warm-up: the buffers grow on the first call
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= 10:
            out.append(time.perf_counter() - t0)
    return round(float(np.median(out) * 1e6), 1)


def room(hip, out):
    K = synth.REPLICA_640
    p = capi.Params(num_sdf_blocks=262144, **synth.REPLICA_PARAMS)
    e = capi.Engine(hip, p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    frames = list(synth.replica_stream(20))
    for f in frames:
        e.set_pose(f.R, f.t)
        e.upload_depth(f.depth)
        e.upload_rgb(f.rgb)
        e.integrate()
    e.sync()
    last = frames[-1]
    cam = (K.fx, K.fy, K.cx, K.cy, K.rows, K.cols)
    near, far, margin = 0.01, 8.0, 0.08
    e.freespace_create((-64, -64, -64), (128, 128, 128), 3)
    d_depth = [hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(f.depth, F)) for f in frames]

    def carve(i=-1):
        e.freespace_carve_depth_device(d_depth[i].ptr, *cam, frames[i].R, frames[i].t, near, far, margin=margin)
        e.sync()

    def clear():
        e.freespace_clear()
        e.sync()

    n_cells = 128 ** 3
    d_box = hipmem.DeviceBuffer(256 * 256 * 128)
    clear()
    carve()
    e.freespace_box_device((-64, -64, -64), (128, 128, 128), d_box.ptr)
    e.sync()
    out["room_cells_one_frame"] = int(np.count_nonzero(d_box.to_numpy(np.uint8)[:n_cells] & capi.FREE_FREE))
    if wanted("carve_empty"):
        out["carve_empty_us"] = median_us(carve, before=clear)
    if LEGS is None or LEGS & {"carve_saturated", "box", "segments"}:  # a run of carve_empty alone traces no other carve than its own
        for i in range(20):
            carve(i)
    e.freespace_box_device((-64, -64, -64), (128, 128, 128), d_box.ptr)
    e.sync()
    st = d_box.to_numpy(np.uint8)[:n_cells]
    out["room_cells_20_frames"] = int(np.count_nonzero(st & capi.FREE_FREE))
    if wanted("carve_saturated"):
        out["carve_saturated_us"] = median_us(carve)
    if wanted("raycast"):
        d_img = hipmem.DeviceBuffer(4 * K.rows * K.cols)

        def render():
            e.raycast_device(*cam, last.R, last.t, 0.1, far, d_depth=d_img.ptr)
            e.sync()
        out["raycast_us"] = median_us(render)
    if wanted("box"):
        def box():
            e.freespace_box_device((-128, -128, -64), (256, 256, 128), d_box.ptr)
            e.sync()
        out["box_256x256x128_us"] = median_us(box)
        st = d_box.to_numpy(np.uint8)
        out["box_histogram"] = np.bincount(st, minlength=16)[:16].tolist()
    if wanted("segments"):
        n = 1 << 17
        rng = np.random.default_rng(0)
        a = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
        d = rng.normal(size=(n, 3)).astype(F)
        b = (a + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 2.0, (n, 1))).astype(F)
        d_a, d_b, d_s, d_c = hipmem.DeviceBuffer.from_numpy(a), hipmem.DeviceBuffer.from_numpy(b), hipmem.DeviceBuffer(n), hipmem.DeviceBuffer(8 * n)

        def segs():
            e.freespace_segments_device(d_a.ptr, d_b.ptr, n, d_s.ptr, d_c.ptr)
            e.sync()
        out["segments_2e17_us"] = median_us(segs)
        out["segments_free"] = int(np.count_nonzero(d_s.to_numpy(np.uint8) == 0))
        out["segments_mean_samples"] = round(float(d_c.to_numpy(np.uint32).reshape(n, 2)[:, 0].mean()), 1)
    if wanted("integrate"):
        def integrate():
            e.set_pose(last.R, last.t)
            e.upload_depth(last.depth)
            e.upload_rgb(last.rgb)
            e.integrate()
            e.sync()
        out["integrate_us"] = median_us(integrate)
    e.close()


def street(hip, out):
    params = dict(synth.VBR_PARAMS, min_weight_threshold=1, sdf_truncation=0.8)
    near, far = params["min_depth"], 60.0
    cam_in = synth.spherical_camera(64, 512)
    e = capi.Engine(hip, capi.Params(num_sdf_blocks=131072, **params))
    e.set_camera(cam_in["fx"], cam_in["fy"], cam_in["cx"], cam_in["cy"], 64, 512, near, far, model=1)
    poses = synth.drive_poses(5, step=1.0)
    for t, q in poses:
        depth, rgb = synth.spherical_range_image(synth.street_canyon(), t, q, cam_in)
        e.set_pose(synth.quat_to_rot(q), t)
        e.upload_depth(depth)
        e.upload_rgb(rgb)
        e.integrate()
    e.sync()
    t0, q0 = poses[-1]
    R, t = synth.quat_to_rot(q0).astype(F), np.asarray(t0, F)
    c = synth.spherical_camera(128, 1024)
    n = c["rows"] * c["cols"]
    d_rng, d_pts = hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n)
    e.raycast_spherical_device(c["fx"], c["fy"], c["cx"], c["cy"], c["rows"], c["cols"], R, t, near, far, d_range=d_rng.ptr, d_points=d_pts.ptr)
    e.sync()
    out["scan_points"], out["scan_returns"] = n, int(np.count_nonzero(d_rng.to_numpy(F)))
    vs = params["virtual_voxel_size"]
    centre = np.floor(t / (vs * 8)).astype(int)
    e.freespace_create((int(centre[0]) - 64, int(centre[1]) - 64, int(centre[2]) - 16), (128, 128, 32), 3)

    def carve():
        e.freespace_carve_points_device(d_pts.ptr, n, R, t, near, far, margin=float(vs * 8))
        e.sync()

    def clear():
        e.freespace_clear()
        e.sync()

    out["scan_empty_us"] = median_us(carve, before=clear)
    out["scan_saturated_us"] = median_us(carve)
    e.close()


def main():
    hip = capi.load_hip()
    out = dict(calls=CALLS)
    if LEGS is None or LEGS - {"scan"}:
        room(hip, out)
    if wanted("scan"):
        street(hip, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
