"""Distance-field timing (include/mrhash_esdf.h): a 256 x 256 x 128 box at a reach of 64 voxels on the Replica
stand-in after 20 fused frames, laid over the far wall (voxels x, y in [-128, 128), z in [-232, -104); the wall is at z = -200).
Prints one JSON line:

  us_per_field        mrh_esdf_device (dist, state and d2) + mrh_sync, median over >= 200 calls after a warm-up
  us_per_field_dist   the same with dist alone
  us_per_field_host   the same through mrh_esdf (blocking, read-back of dist and state included)
  cells_per_s         cells / us_per_field
  site_fraction, far_fraction, observed_fraction of the cells

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_esdf.py` the kernels' own times are the k_esdf_* rows."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(_pos[0]) if _pos else 200
K = synth.REPLICA_640
ORIGIN, DIMS, REACH = (-128, -128, -232), (256, 256, 128), 64


def median_us(fn, e):
    for _ in range(10):  # warm-up
        fn()
    e.sync()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        e.sync()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e6), float(np.quantile(t, 0.9) * 1e6)


def main():
    p = capi.Params(num_sdf_blocks=262144, **synth.REPLICA_PARAMS)
    e = capi.Engine(capi.load_hip(), p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    for f in synth.replica_stream(20):
        e.set_pose(f.R, f.t)
        e.upload_depth(f.depth)
        e.upload_rgb(f.rgb)
        e.integrate()
    e.sync()
    n = DIMS[0] * DIMS[1] * DIMS[2]
    dd, ds, dq = hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(n), hipmem.DeviceBuffer(4 * n)
    full, full90 = median_us(lambda: e.esdf_device(ORIGIN, DIMS, REACH, d_dist=dd.ptr, d_state=ds.ptr, d_d2=dq.ptr), e)
    dist_only, _ = median_us(lambda: e.esdf_device(ORIGIN, DIMS, REACH, d_dist=dd.ptr), e)
    host, _ = median_us(lambda: e.esdf(ORIGIN, DIMS, REACH), e)
    state = ds.to_numpy(np.uint8)
    out = dict(calls=CALLS, origin=ORIGIN, dims=DIMS, reach=REACH, cells=n, blocks=int(e.stats().occupied_fine),
               us_per_field=round(full, 1), us_per_field_p90=round(full90, 1), us_per_field_dist=round(dist_only, 1),
               us_per_field_host=round(host, 1), cells_per_s=round(n / (full * 1e-6)),
               site_fraction=round(float(((state & capi.ESDF_SITE) != 0).mean()), 4), far_fraction=round(float(((state & capi.ESDF_FAR) != 0).mean()), 4),
               observed_fraction=round(float(((state & capi.ESDF_OBSERVED) != 0).mean()), 4))
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
