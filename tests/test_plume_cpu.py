"""The odor plume's specification ``tests/plume_spec.py`` against the properties its definition promises, and the ctypes mirror of
``nmf_plume_params`` against the library (no GPU)."""
import ctypes

import numpy as np
import pytest

import plume_spec as spec

from flygym_amd import _native
from flygym_amd.sensors import OdorPlume, _PlumeParams

# (seed, world, tick) -> hash(x_m) >> 8 for m = 0..7, computed with Python integers from the definition
UNIFORMS = {
    (0, 0, 0): [0, 6412156, 8406067, 811773, 15571589, 7340156, 13348648, 12009533],
    (1, 0, 0): [6850960, 13611694, 12852974, 13706648, 12342396, 11731829, 695777, 7964234],
    (0, 1, 0): [130277, 7041185, 671754, 16441093, 9288977, 4366896, 308104, 10290372],
    (0, 0, 1): [2031336, 10829048, 9197356, 11661589, 15860773, 15947045, 10506963, 252203],
    (20240917, 4095, 39): [7211424, 12226424, 1314283, 865545, 2961196, 15748652, 16766275, 1889694],
    (4294967295, 65535, 1000000): [642614, 13199442, 3350485, 10742105, 9873391, 12668031, 12065176, 1672402],
}
# the float32 noise (xi_x, xi_y) of the same triples
NOISE32 = {
    (0, 0, 0): (-1.8504878282546997, 1.5192019939422607),
    (1, 0, 0): (1.3903969526290894, -0.0846756175160408),
    (0, 1, 0): (-0.9570313692092896, -0.9601246118545532),
    (0, 0, 1): (0.01702357828617096, 0.9304403066635132),
    (20240917, 4095, 39): (-1.232330083847046, 0.39348068833351135),
    (4294967295, 65535, 1000000): (-0.5801770091056824, 0.28127968311309814),
}


def test_hash_and_noise_golden_values():
    assert spec.hash32([0, 1, 0xDEADBEEF]).tolist() == [0, 1753845952, 3861431939]
    for (seed, world, tick), want in UNIFORMS.items():
        assert [int(spec.uniforms(seed, world, tick, m)) for m in range(8)] == want
        for m0, xi in zip((0, 4), NOISE32[(seed, world, tick)]):
            got = spec.noise(seed, np.array([world]), np.array([tick]), m0, np.float32)
            assert got.dtype == np.float32 and float(got[0]) == xi
            u = np.array(want[m0:m0 + 4], dtype=np.float64) * 2.0 ** -24
            assert float(spec.noise(seed, np.array([world]), np.array([tick]), m0, np.float64)[0]) == pytest.approx((u.sum() - 2) * np.sqrt(3.0), abs=1e-15)


def test_noise_has_zero_mean_and_unit_variance():
    xi = spec.noise(7, np.arange(4096)[:, None], np.arange(64)[None, :], 0, np.float64)
    assert abs(xi.mean()) < 0.01 and abs(xi.var() - 1.0) < 0.02 and np.abs(xi).max() <= 2 * np.sqrt(3.0)


def _blob(H=21, W=33, dtype=np.float64):
    jj, ii = np.mgrid[0:H, 0:W]
    return np.exp(-((jj - 10.0) ** 2 + (ii - 16.0) ** 2) / 4.0).astype(np.float32).astype(dtype)[None]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_still_air_is_the_explicit_heat_step(dtype):
    c = _blob(dtype=dtype)
    c[0, :4] = c[0, -4:] = 0
    c[0, :, :6] = c[0, :, -6:] = 0                            # the blob stays away from the border for three ticks
    D = np.float32(0.2)
    new = spec.tick(c, np.zeros((1, 2)), r=np.float32(1.0), D=D, source=np.zeros(c.shape[1:]), dtype=dtype)
    want = c[0].copy()
    want[1:-1, 1:-1] += dtype(D) * (c[0, 1:-1, :-2] + c[0, 1:-1, 2:] + c[0, :-2, 1:-1] + c[0, 2:, 1:-1] - 4 * c[0, 1:-1, 1:-1])
    assert new.dtype == dtype
    np.testing.assert_allclose(new[0], want, rtol=0, atol=4 * np.finfo(dtype).eps)
    total = c.sum(dtype=np.float64)
    for _ in range(3):
        c = spec.tick(c, np.zeros((1, 2)), r=np.float32(1.0), D=D, source=np.zeros(c.shape[1:]), dtype=dtype)
    assert c[0, 0].max() == 0 and c[0, :, 0].max() == 0      # nothing reached the border
    assert abs(c.sum(dtype=np.float64) - total) <= 64 * np.finfo(dtype).eps * total


def test_one_cell_per_tick_shifts_the_field_exactly():
    c = _blob()
    for wind, shift in (((1.0, 0.0), (0, 1)), ((0.0, -1.0), (-1, 0)), ((-3.0, 2.0), (2, -3))):
        for dtype in (np.float32, np.float64):
            new = spec.tick(c, np.array([wind]), r=np.float32(1.0), D=np.float32(0.0), source=np.zeros(c.shape[1:]), dtype=dtype)
            want = np.zeros_like(c[0])
            H, W = want.shape
            dj, di = shift
            want[max(dj, 0):H + min(dj, 0), max(di, 0):W + min(di, 0)] = c[0, max(-dj, 0):H + min(-dj, 0), max(-di, 0):W + min(-di, 0)]
            assert np.array_equal(new[0], want.astype(dtype))


def test_two_and_a_half_cells_blend_two_cells():
    c = _blob()
    new = spec.tick(c, np.array([[2.5, 0.0]]), r=np.float32(1.0), D=np.float32(0.0), source=np.zeros(c.shape[1:]))
    want = np.zeros_like(c[0])
    want[:, 3:] = 0.5 * c[0, :, 1:-2] + 0.5 * c[0, :, :-3]
    want[:, 2] = 0.5 * c[0, :, 0]
    assert np.array_equal(new[0], want)
    # a displacement far beyond the grid empties it: no clamp
    gone = spec.tick(c, np.array([[1e6, -1e30]]), r=np.float32(1.0), D=np.float32(0.0), source=np.zeros(c.shape[1:]))
    assert not gone.any()


def test_source_cells_are_held_at_peak():
    H, W = 21, 33
    S = OdorPlume.disc_source((H, W), 0.5, (-1.0, 2.0), 3.2, 6.1, 1.2, 7.0)
    assert S.dtype == np.float32 and S.shape == (H, W) and 10 <= int((S > 0).sum()) <= 25 and set(np.unique(S)) == {0.0, 7.0}
    jj, ii = np.nonzero(S)
    assert np.all((-1.0 + (ii + 0.5) * 0.5 - 3.2) ** 2 + (2.0 + (jj + 0.5) * 0.5 - 6.1) ** 2 <= 1.2 ** 2)
    c = np.zeros((1, H, W))
    for _ in range(5):
        c = spec.tick(c, np.array([[0.7, -0.3]]), r=np.float32(1.0), D=np.float32(0.1), source=S)
        assert np.all(c[0][S > 0] == 7.0) and c.max() == 7.0 and c.min() >= 0.0
    assert (c[0] > 0).sum() > (S > 0).sum()                  # and the odor spreads from them


def _scenario(dtype, n_ticks=40):
    H, W, n = 19, 27, 3
    r, D, a, b = spec.constants(0.5, 0.02, 0.6, 0.5, 3.0)
    S = OdorPlume.disc_source((H, W), 0.5, (0.0, 0.0), 3.0, 5.0, 1.0, 2.0)
    jj, ii = np.mgrid[0:H, 0:W]
    E = (5.0 * np.stack([np.sin(2 * np.pi * jj / H) * np.cos(np.pi * ii / W), np.cos(2 * np.pi * ii / W)], axis=-1)).astype(np.float32)
    wind = np.array([[30.0, 4.0], [-12.0, -20.0], [0.0, 0.0]], dtype=np.float32)
    out = spec.advance(np.zeros((n, H, W)), wind, np.zeros(n), n_ticks, r=r, D=D, a=a, b=b, mean=(20.0, 0.0), seed=11, source=S,
                       eddies=E, eddy_gain=0.7, dtype=dtype)
    return out, (r, D, a, b)


def test_float32_and_float64_flavours_agree():
    (c32, w32, t32, ws32), (r, D, a, b) = _scenario(np.float32)
    (c64, w64, t64, ws64), _ = _scenario(np.float64)
    assert c32.dtype == np.float32 and ws32.dtype == np.float32 and all(v.dtype == np.float32 for v in (r, D, a, b))
    assert t32.tolist() == t64.tolist() == [40, 40, 40]
    assert c64.max() == 2.0 and (c64 > 1e-3).sum() > 50
    # One tick is a blend of four cells plus a stencil of five: some eight float32 roundings of values up to the peak, and blend
    # weights that the rounding of d = v r moves by an ulp of d (here d < 4 cells) times a gradient of at most one peak per cell:
    # 10 ulp of the peak per tick.  In this smooth flow a tick does not amplify (see DESIGN.md section 7 for the flows that do), so
    # 40 ticks stay below 400 ulp of the peak; the wind sums 40 roundings at its own size.
    ulp_peak = float(np.spacing(np.float32(2.0)))
    assert np.abs(c32 - c64).max() < 400 * ulp_peak
    assert np.abs(ws32 - ws64).max() < 40 * 2 * np.spacing(np.float32(30.0))
    pts = np.random.default_rng(6).uniform(-1.0, 14.5, (3, 50, 2)).astype(np.float32)
    v32, f32 = spec.read(c32, pts, cell_size=0.5, origin=(0.0, 0.0), scale=3.0, dtype=np.float32)
    v64, f64 = spec.read(c64, pts, cell_size=0.5, origin=(0.0, 0.0), scale=3.0, dtype=np.float64)
    assert v32.dtype == np.float32 and f32.tolist() == f64.tolist() == [1, 1, 1]
    # (a reading adds the rounding of u, v at 30 cells — an ulp of 30 times a peak per cell — to the grid's own deviation)
    assert np.abs(v32 - v64).max() < 3.0 * (400 * ulp_peak + 4 * 2.0 * float(np.spacing(np.float32(30.0))))


def test_readings_interpolate_between_centres_and_flag_the_outside():
    c = np.arange(8 * 8, dtype=np.float64).reshape(1, 8, 8)
    pts = np.array([[[1.0, 1.0],          # centre of cell (0, 0)
                     [3.0, 1.0],          # centre of cell (0, 1)
                     [2.0, 2.0],          # the corner four cells share
                     [0.5, 1.0],          # a quarter cell inside the border: half of cell (0, 0)
                     [-0.5, 1.0],         # a quarter cell outside: a quarter of it, and flagged
                     [-1.0, 1.0],         # half a cell outside: 0
                     [16.5, 15.5]]])      # a quarter cell beyond the last centres: cell (7, 7) times 1/4 * 3/4
    val, flag = spec.read(c, pts, cell_size=2.0, origin=(0.0, 0.0), scale=2.0)
    np.testing.assert_allclose(val[0], [0.0, 2.0, 9.0, 0.0, 0.0, 0.0, 2.0 * 63 * 0.25 * 0.75], atol=1e-12)
    assert flag.tolist() == [1]
    c1 = np.ones((1, 8, 8))
    val, flag = spec.read(c1, pts[:, :4], cell_size=2.0, origin=(0.0, 0.0))
    np.testing.assert_allclose(val[0], [1.0, 1.0, 1.0, 0.75], atol=1e-12)
    assert flag.tolist() == [0]
    val, flag = spec.read(c1, pts[:, 4:6], cell_size=2.0, origin=(0.0, 0.0))
    np.testing.assert_allclose(val[0], [0.25, 0.0], atol=1e-12)
    assert flag.tolist() == [1]


def test_params_struct_matches_the_library():
    """The library loads without a GPU; the ctypes mirror has the layout it was compiled with."""
    _native.build()
    L = _native.lib()
    assert ctypes.sizeof(_PlumeParams) == L.nmf_plume_params_size() == 64
    for name in ("nmf_plume_create", "nmf_plume_destroy", "nmf_plume_reset", "nmf_plume_advance", "nmf_plume_field_ptr",
                 "nmf_plume_sample_points", "nmf_plume_sample_sites"):
        assert name in _native.exported_symbols() and hasattr(L, name)
