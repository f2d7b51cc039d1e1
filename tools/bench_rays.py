"""Ray queries against the spherical render (include/mrhash_rays.h), in one process on the street of
tools/bench_track.py: five range images fused at 20 cm voxels and a 4-voxel truncation, seen through the 128 x 1024 spherical camera
of the tracking benchmarks from the last pose — 131 072 rays, range + normals + colours.

  render        mrh_raycast_spherical_device: the yardstick (twice, around the casts: the spread of the same command)
  cast_tiles    mrh_cast_rays_device of the same rays in the render's order — 8 x 8 tiles, four of them per 16 x 16 workgroup tile
  cast_rows     ... in row-major order
  cast_shuffled ... in a seeded shuffle
  cast_tiles_counts  the tile order again, with MRH_RAYS_COUNTS

Every timed call is the device form followed by mrh_sync, a host clock around both; the median over CALLS calls after a warm-up of
10.  The rays are the camera's own: origin (0, 0, 0) and d_c of every pixel in the sensor frame, the camera's pose for the batch;
d_c comes from numpy's float32 sine and cosine, not the library's, so a few rays differ from the render's in the last bit —
`ranges_equal` says how many pixels return the render's bits all the same.  Prints one JSON line.

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_rays.py 20`, a run of its own, the kernels' own times are the rows of
k_raycast and k_cast_rays."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(_pos[0]) if _pos else 50
F = np.float32


def median_us(fn, n=None):
    for _ in range(10):  # warm-up: the buffers grow on the first call
        fn()
    out = []
    for _ in range(n or CALLS):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return round(float(np.median(out) * 1e6), 1)


def street(hip):
    """The street map of tools/bench_track.py's scan leg and its last pose."""
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
    return e, synth.quat_to_rot(q0).astype(F), np.asarray(t0, F), near, far


def pixel_directions(c):
    """d_c of every pixel, row-major [rows * cols, 3]: the render's expressions with numpy's float32 sine and cosine."""
    rows, cols = c["rows"], c["cols"]
    ifx, ify = F(1.0) / F(c["fx"]), F(1.0) / F(c["fy"])
    az = (ifx * ((np.arange(cols, dtype=F) - F(c["cx"])) - F(0.5))).astype(F)
    el = (ify * ((np.arange(rows, dtype=F) - F(c["cy"])) - F(0.5))).astype(F)
    s0, c0, s1, c1 = np.sin(az), np.cos(az), np.sin(el)[:, None], np.cos(el)[:, None]
    return np.stack([np.broadcast_to(c0 * c1, (rows, cols)), np.broadcast_to(s0 * c1, (rows, cols)), np.broadcast_to(s1, (rows, cols))], -1).astype(F).reshape(-1, 3)


def tile_order(rows, cols):
    """The pixels in the order k_raycast's lanes take them: 16 x 16 workgroup tiles row-major, in each four 8 x 8 wave tiles."""
    r, c = np.mgrid[0:rows, 0:cols]
    key = ((r // 16) * ((cols + 15) // 16) + c // 16) * 256 + (((r % 16) // 8) * 2 + (c % 16) // 8) * 64 + (r % 8) * 8 + c % 8
    return np.argsort(key.ravel(), kind="stable")


def main():
    hip = capi.load_hip()
    e, R, t, near, far = street(hip)
    c = synth.spherical_camera(128, 1024)
    cam = (c["fx"], c["fy"], c["cx"], c["cy"], c["rows"], c["cols"])
    n = c["rows"] * c["cols"]
    d_rows = pixel_directions(c)
    d_rng, d_nrm, d_rgb = hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n), hipmem.DeviceBuffer(3 * n)
    d_sta, d_cnt, d_fu = hipmem.DeviceBuffer(n), hipmem.DeviceBuffer(8 * n), hipmem.DeviceBuffer(4 * n)
    d_org = hipmem.DeviceBuffer.from_numpy(np.zeros((n, 3), F))

    def render():
        e.raycast_spherical_device(*cam, R, t, near, far, d_range=d_rng.ptr, d_normals=d_nrm.ptr, d_rgb=d_rgb.ptr)
        e.sync()

    def cast(d_dirs, counts=False):
        def go():
            e.cast_rays_device(d_org.ptr, d_dirs.ptr, n, far, near, R=R, t=t, d_range=d_rng.ptr, d_status=d_sta.ptr, d_normals=d_nrm.ptr, d_rgb=d_rgb.ptr,
                               d_counts=d_cnt.ptr if counts else 0, d_first_unknown=d_fu.ptr if counts else 0)
            e.sync()
        return go

    orders = {"tiles": tile_order(c["rows"], c["cols"]), "rows": np.arange(n), "shuffled": np.random.default_rng(0).permutation(n)}
    dirs = {k: hipmem.DeviceBuffer.from_numpy(np.ascontiguousarray(d_rows[v])) for k, v in orders.items()}
    out = dict(calls=CALLS, rays=n, rows=c["rows"], cols=c["cols"], min_range=near, max_range=far, blocks=int(e.stats().occupied_fine))
    render()
    want = d_rng.to_numpy(F).copy()
    out["hits"] = int(np.count_nonzero(want))
    out["render_us"] = median_us(render)
    for k in ("tiles", "rows", "shuffled"):
        out["cast_%s_us" % k] = median_us(cast(dirs[k]))
    out["cast_tiles_counts_us"] = median_us(cast(dirs["tiles"], counts=True))
    out["render_again_us"] = median_us(render)
    out["cast_tiles_again_us"] = median_us(cast(dirs["tiles"]))
    cast(dirs["rows"], counts=True)()
    got, status, counts = d_rng.to_numpy(F), d_sta.to_numpy(np.uint8), d_cnt.to_numpy(np.uint32).reshape(n, 2)
    out["ranges_equal"] = int(np.count_nonzero(got.view(np.uint32) == want.view(np.uint32)))
    out["status_histogram"] = np.bincount(status, minlength=8)[:8].tolist()
    out["mean_free_samples"], out["mean_unknown_samples"] = round(float(counts[:, 0].mean()), 2), round(float(counts[:, 1].mean()), 2)
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
