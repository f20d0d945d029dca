"""Field volumes, the parts that need no GPU: scenes.volume_points is the library's voxel rule -- origin + step * idx in
float32, one multiplication and one addition, each rounded -- in the output order of dsl_field_volume (x fastest), and the
library exports the entry point."""
import numpy as np


def _rule_f64(origin, step, idx):
    """the float32 rule from float64 arithmetic rounded step by step.  (A float64 product of two float32 values is exact,
    and so is the float64 sum of two float32 values unless their exponents lie more than 29 apart, where rounding it to
    float32 still gives the correctly rounded sum: each np.float32(...) below is ONE rounding of the exact result.)"""
    t = np.float32(np.float64(np.float32(step)) * np.float64(np.float32(idx)))
    return np.float32(np.float64(np.float32(origin)) + np.float64(t))


def test_volume_points_follow_the_float32_rule_in_x_fastest_order():
    from dieselfluid_amd import scenes
    cases = [((-2.3, -2.1, -1.9), (0.37, 0.41, 0.43), (13, 11, 9)),
             ((-4.6, -0.7, -0.5), 0.45, (21, 4, 3)),
             ((1.0e-3, 3.0e4, -7.77), (1.0 / 3.0, 0.1, 1.0e-5), (5, 1, 40)),
             ((-0.09375,) * 3, 0.0625, (27, 23, 19))]
    for origin, step, dims in cases:
        pts = scenes.volume_points(origin, step, dims)
        nx, ny, nz = dims
        assert pts.shape == (nx * ny * nz, 3) and pts.dtype == np.float32
        s3 = np.broadcast_to(np.asarray(step, dtype=np.float32), (3,))
        fused_differs = False
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    row = pts[(k * ny + j) * nx + i]
                    want = [_rule_f64(origin[a], s3[a], idx) for a, idx in enumerate((i, j, k))]
                    assert row.view(np.uint32).tolist() == np.array(want, np.float32).view(np.uint32).tolist(), (dims, i, j, k)
                    fused = np.float32(np.float64(np.float32(origin[0])) + np.float64(s3[0]) * np.float64(i))
                    fused_differs |= bool(fused != want[0])
        if dims == (13, 11, 9):
            assert fused_differs  # (the case tells the two-rounding rule from a fused multiply-add)
    # x runs fastest, then y, then z
    pts = scenes.volume_points((0.0, 10.0, 20.0), 1.0, (3, 2, 2))
    assert pts[:4].tolist() == [[0.0, 10.0, 20.0], [1.0, 10.0, 20.0], [2.0, 10.0, 20.0], [0.0, 11.0, 20.0]]
    assert pts[6].tolist() == [0.0, 10.0, 21.0]


def test_the_library_exports_the_entry_point():
    import ctypes as C
    from dieselfluid_amd import _lib
    _lib.build_library()
    assert hasattr(C.CDLL(_lib.library_path()), "dsl_field_volume") and len(_lib.EXPORTS["dsl_field_volume"][1]) == 7
