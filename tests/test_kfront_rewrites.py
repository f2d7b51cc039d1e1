"""The rewrites of the allocation rays' world -> block conversion (mrh_device.h: voxel_round_arg, world_to_block_fast; mrh_pipe.h:
ray_from_segment's `bound`) against the literal expressions, in numpy's float32 (IEEE, denormals kept), over the float range: every
exponent with a dense mantissa sample, +-0, denormals, inf, NaN, and the three neighbours of every integer and half-integer up to
2^24 on both sides of zero.  No GPU."""
import numpy as np

EPS = np.float32(1e-5)
HALF = np.float32(0.5)


def cvt_i32(x):
    """v_cvt_i32_f32 / f2i: toward zero, saturating, NaN -> 0"""
    t = np.trunc(x.astype(np.float64))
    t = np.where(np.isnan(t), 0.0, np.clip(t, -2147483648.0, 2147483647.0))
    return t.astype(np.int64)


def literal_arg(p):
    """world_to_voxel (vhu.cuh:143-151) up to the conversion: a = p + sign(p) * 0.5; a >= 0 ? floor(a + eps) : ceil(a - eps)"""
    with np.errstate(invalid="ignore", over="ignore"):
        sgn = (np.float32(0) < p).astype(np.int32) - (p < np.float32(0)).astype(np.int32)
        a = p + sgn.astype(np.float32) * HALF
        return np.where(a >= 0, np.floor(a + EPS), np.ceil(a - EPS)).astype(np.float32)


def rewritten_arg(p):
    with np.errstate(invalid="ignore", over="ignore"):
        return (p + np.copysign(HALF, p)) + np.copysign(EPS, p)


def check(p):
    p = np.concatenate([p, -p])
    x_lit, x_new = literal_arg(p), rewritten_arg(p)
    v_lit, v_new = cvt_i32(x_lit), cvt_i32(x_new)
    bad = np.nonzero(v_lit != v_new)[0]
    assert len(bad) == 0, (p[bad[:4]], v_lit[bad[:4]], v_new[bad[:4]])
    # the shift-limit test: |int(x)| < L on the integers == |x| < L on the floats for every integer L up to 2^22, i.e.
    # floor(|x|) == |int(x)| below 2^23 (NaN: compared through fmaxf, which drops it, as the OR drops its v == 0)
    ok = ~np.isnan(x_new)
    ax = np.minimum(np.abs(x_new[ok]).astype(np.float64), float(1 << 23))  # limits go up to 2^22
    av = np.minimum(np.abs(v_new[ok]), 1 << 23)
    assert np.array_equal(np.floor(ax).astype(np.int64), av)  # same integer part => the same side of every integer L
    return len(p)


def test_voxel_rounding_over_the_float_range():
    rng = np.random.default_rng(0)
    man = np.unique(np.concatenate([rng.integers(0, 1 << 23, 4096), [0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF]])).astype(np.uint32)
    exp = np.arange(256, dtype=np.uint32)  # 0: zero and the denormals, 255: inf and NaN
    bits = ((exp[:, None] << 23) | man[None, :]).ravel()
    n = check(bits.view(np.float32))
    special = np.array([0.0, np.inf, np.nan, 0.5, 1e-5, 0.49999, 0.5 - 1e-5, 2147483648.0, 2147483520.0, 4294967296.0], np.float32)
    n += check(special)
    print("patterns checked:", n)


def test_voxel_rounding_at_every_integer_and_half_integer():
    n = 0
    for lo in range(0, 1 << 25, 1 << 17):  # k / 2 for k = 0 .. 2^25: every integer and half-integer up to 2^24 (cache-sized chunks)
        c = np.arange(lo, lo + (1 << 17) + 1, dtype=np.float64).astype(np.float32) * HALF
        # ... and c - eps, from where a + eps = (p + 0.5) + eps comes back to an integer (c runs over the half-integers too)
        n += check(np.concatenate([c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf)), c - EPS]))
    print("patterns checked:", n)


def test_bound_is_the_integer_sum_inside_the_key_range():
    """bound = int(float(end) + step): equal to end + step for |end| < 2^24; from there on both lie outside the key range
    (|block| < 2^20), which is all ray_keys_in_range asks of them"""
    rng = np.random.default_rng(1)
    end = np.unique(np.concatenate([np.arange(-(1 << 21), (1 << 21) + 1), rng.integers(-(1 << 28), 1 << 28, 1 << 20),
                                    np.array([-(1 << 24), (1 << 24), -(1 << 24) - 1, (1 << 24) + 1, -(1 << 28), (1 << 28) - 1])])).astype(np.int64)
    for step in (-1, 0, 1):
        lit = cvt_i32(end.astype(np.float32) + np.float32(step))
        new = end + step
        small = np.abs(end) < (1 << 24)
        assert np.array_equal(lit[small], new[small])
        out = lambda b: (b + (1 << 20) < 0) | (b + (1 << 20) >= (1 << 21))  # noqa: E731  pack_key's range test
        assert out(lit[~small]).all() and out(new[~small]).all()
