"""A restatement of the spherical raycast (include/mrhash_raycast.h) on top of tests/raycast_ref.py: the march,
the refinement, the normal and the colour are raycast_ref.Raycaster's (D11); the ray leaves through the spherical back-projection
(camera.cuh:91-99 with d = 1) and the crossing comes back as a sensor-frame point as well.

Sine and cosine are the oracle's orc_softmath (ops 0 and 1: include/mrh_softmath.h compiled for the host), so the direction has
the kernel's bits; every product and sum around them is a numpy float32 operation.  Test infrastructure only."""
from __future__ import annotations

import ctypes

import numpy as np

import parity_utils as pu
import raycast_ref as rr

F = np.float32


def _softmath():
    o = pu.oracle_lib()
    o.orc_softmath.restype = ctypes.c_float
    o.orc_softmath.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_float]
    return lambda op, a: F(o.orc_softmath(op, float(a), 0.0))


class SphericalRaycaster(rr.Raycaster):
    """One render: spherical intrinsics (fx, fy in pixels per radian), sensor-to-world pose, range interval and sample spacing."""

    def __init__(self, m, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step):
        super().__init__(m, fx, fy, cx, cy, rows, cols, R, t, min_depth, max_depth, step)
        self._f = _softmath()

    def sensor_directions(self, rows, cols) -> np.ndarray:
        """d_c = (cos az cos el, sin az cos el, sin el), az = ifx * ((c - cx) - 0.5), el = ify * ((r - cy) - 0.5)."""
        rows, cols = np.asarray(rows).ravel(), np.asarray(cols).ravel()
        cam = self.cam
        az = (cam.ifx * ((cols.astype(F) - cam.cx) - F(0.5))).astype(F)
        el = (cam.ify * ((rows.astype(F) - cam.cy) - F(0.5))).astype(F)
        sc = {}  # an image has few distinct angles: rows + cols of them

        def sincos(x):
            k = float(x)
            if k not in sc:
                sc[k] = (self._f(0, x), self._f(1, x))
            return sc[k]

        out = np.zeros((len(rows), 3), F)
        for i in range(len(rows)):
            s0, c0 = sincos(az[i])
            s1, c1 = sincos(el[i])
            out[i] = (F(c0 * c1), F(s0 * c1), s1)
        return out

    def directions(self, rows, cols) -> np.ndarray:
        """d_w = R d_c, every row summed left to right."""
        dc = self.sensor_directions(rows, cols)
        R = self.cam.R
        return np.stack([R[i, 0] * dc[..., 0] + R[i, 1] * dc[..., 1] + R[i, 2] * dc[..., 2] for i in range(3)], -1).astype(F)

    def render(self, rows, cols):
        """The pixels (rows[i], cols[i]): range [n], normals [n, 3], rgb [n, 3], points [n, 3] (sensor frame; a miss is +0)."""
        rng, nrm, rgb = super().render(rows, cols)
        dc = self.sensor_directions(rows, cols)
        pts = np.where((rng > 0)[:, None], (rng[:, None] * dc).astype(F), F(0)).astype(F)
        return rng, nrm, rgb, pts
