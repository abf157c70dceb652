"""The class key of the NIF stage's class level (ipu_path_trace_amd/csrc/ptmi_share_plan.h: class_coord, class_key) restated in
numpy, with numpy's own binary16 conversion, for the tests that count classes or build rows of one class."""
import numpy as np


def class_coord(coord):
    """numpy's class_coord: uint32 per float32 coordinate."""
    x = (np.asarray(coord, dtype=np.float32) - np.float32(1.0)) * np.float32(2.0)
    bits = x.view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    in_range = (mag >= np.uint32(0x38800000)) & (mag <= np.uint32(0x40000000))
    with np.errstate(over="ignore", invalid="ignore"):
        named = x.astype(np.float16).astype(np.float32).view(np.uint32)
    return np.where(in_range, named, bits)


def class_key(u, v):
    return (class_coord(u).astype(np.uint64) << np.uint64(32)) | class_coord(v).astype(np.uint64)


def class_mates(rng, n):
    """(a, b): n float32 coordinates of [0, 1] each, b[i] another float of a[i]'s class wherever the class has one."""
    a = rng.random(n, dtype=np.float32)
    a[:8] = [0.0, 1.0, 0.5, 0.25, 0.75, 1.0 - 2.0 ** -15, 2.0 ** -20, 0.999]
    b = a.copy()
    for step in (1, 2, 3, 5, 8, 13, 40, 200, 1000):   # ulps of the coordinate: the farthest that stays in the class wins
        for sign in (1, -1):
            c = (a.view(np.int32) + np.int32(sign * step)).view(np.float32)
            ok = (class_coord(c) == class_coord(a)) & (c >= 0) & (c <= 1)
            b = np.where(ok, c, b)
    return a, b
