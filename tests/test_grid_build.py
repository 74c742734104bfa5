"""GPU: the distance field that loikb_collision_set_world_grid builds (include/loik_amd_grid.h, kernels in loik_pose_grid.hpp) against the
brute force of tests/grid_numpy.py, exactly: the sizes at which the three passes change their shape (one voxel, one past a wavefront on
each axis, a partial x tile with several row groups, the cap of an axis, the y and z lengths on either side of the tile change at 256),
the occupancies from empty to full, the device-pointer route, replacing and clearing."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

from test_clearance import _open
import grid_numpy as GN
import qp_cases as QC

pytestmark = pytest.mark.gpu

_S = {}


def _solver():
    """one handle for the module: the grid is a latch of its own and every test sets it afresh"""
    if "s" not in _S:
        model = QC.model_of("panda7")
        _S["s"] = _open(model, model.random_configurations(np.random.default_rng(1), 2))
    return _S["s"]


def _check(occ, origin=(0.1, -0.2, 0.3), h=0.05):
    s = _solver()
    s.set_collision_grid(occ, origin, h)
    got = s.collision_grid()
    occ = np.asarray(occ)
    assert got["dims"] == occ.shape[::-1] and got["voxel"] == h and np.array_equal(got["origin"], np.asarray(origin, dtype=float))
    assert got["G"].dtype == np.uint32 and got["G"].shape == occ.shape
    want = GN.field_brute(occ)
    assert np.array_equal(got["G"], want), "%d voxels differ" % int((got["G"] != want).sum())
    return got["G"]


@pytest.mark.parametrize("filled", [0, 1])
def test_one_voxel(filled):
    G = _check(np.full((1, 1, 1), filled, dtype=np.uint8))
    assert G[0, 0, 0] == (0 if filled else capi.GRID_EMPTY)


@pytest.mark.parametrize("dims", [(65, 1, 1), (1, 65, 1), (1, 1, 65), (65, 3, 130), (512, 1, 2)])
def test_shapes(dims):
    """(nx, ny, nz): one past a wavefront on each axis; a partial x tile in the y and z passes with 130 / 4 row groups in z; the cap of
    an axis, where g reaches 1021^2"""
    occ = GN.random_occupancy(dims, 0.03, sum(dims))
    occ[0, 0, 0] = 1
    G = _check(occ)
    if dims == (512, 1, 2):
        one = np.zeros((2, 1, 512), dtype=np.uint8)
        one[0, 0, 0] = 1
        G = _check(one)
        assert int(G[1, 0, 511]) == 1021 ** 2 + 1 and int(G.max()) == 1021 ** 2 + 1


@pytest.mark.parametrize("dims", [(33, 256, 1), (33, 1, 256), (33, 300, 1), (33, 1, 257), (3, 512, 1), (3, 1, 512)])
def test_long_y_and_z_axes(dims):
    """(nx, ny, nz): k_grid_pass changes its tile at 256 voxels.  256: the widest tile of 64 lanes, exactly 64 KB of LDS; 257 and 300: the
    first sizes with 32 lanes a line group, eight row groups and a partial x tile; 512: the cap, the other 64 KB tile, and with a single
    far corner occupied the largest g, 1021^2, on that pass"""
    occ = GN.random_occupancy(dims, 0.02, sum(dims))
    occ[0, 0, 0] = 1
    _check(occ)
    if max(dims) == 512:
        one = np.zeros(dims[::-1], dtype=np.uint8)
        one[0, 0, 0] = 1
        G = _check(one)
        assert int(G[-1, -1, 0]) == 1021 ** 2 and int(G[-1, -1, 2]) == 1021 ** 2 + 9 == int(G.max())


@pytest.mark.parametrize("frac", [0.05, 0.2, 0.6])
def test_occupancies(frac):
    _check(GN.random_occupancy((7, 5, 6), frac, int(frac * 100)))


def test_empty_full_and_corner():
    assert np.all(_check(np.zeros((6, 5, 7), dtype=np.uint8)) == capi.GRID_EMPTY)
    assert np.all(_check(np.ones((6, 5, 7), dtype=np.uint8)) == 0)
    occ = np.zeros((6, 5, 7), dtype=np.uint8)
    occ[5, 4, 6] = 1
    G = _check(occ)
    assert int(G[0, 0, 0]) == 11 ** 2 + 7 ** 2 + 9 ** 2 and int(G[5, 4, 6]) == 0
    # any integer or bool dtype, nonzero is occupied
    s = _solver()
    for dtype in (bool, np.int64, np.int8):
        s.set_collision_grid((occ * 3).astype(dtype), (0, 0, 0), 0.1)
        assert np.array_equal(s.collision_grid()["G"], G)


class _DeviceBytes:
    """a uint8 array in device memory behind the data_ptr() / is_cuda protocol of the binding (capi.DeviceArray holds the bytes)"""

    def __init__(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        raw = np.zeros((a.size + 7) // 8 * 8, dtype=np.uint8)
        raw[:a.size] = a.ravel()
        self._d = capi.DeviceArray(raw.view(np.float64))
        self.shape, self.is_cuda = a.shape, True

    def data_ptr(self):
        return self._d.data_ptr()

    def element_size(self):
        return 1


def test_device_route_replace_and_clear():
    s = _solver()
    occ = GN.random_occupancy((65, 3, 9), 0.1, 3)
    host = _check(occ).copy()
    s.set_collision_grid(None)
    assert s.collision_grid() is None
    s.set_collision_grid(_DeviceBytes(occ), (0.1, -0.2, 0.3), 0.05)
    got = s.collision_grid()
    assert got["dims"] == (65, 3, 9) and np.array_equal(got["G"], host)
    # a second set replaces the first: another shape, another occupancy, then the first again
    other = GN.random_occupancy((5, 4, 3), 0.3, 4)
    _check(other, origin=(1.0, 2.0, 3.0), h=0.25)
    assert np.array_equal(_check(occ), host)
    # the field into a device buffer (LOIKB_OUT_DEVICE)
    dev = capi.DeviceArray(np.zeros((occ.size + 1) // 2))
    assert s.L.loikb_collision_get_world_grid(s.h, None, None, None, C.c_void_p(dev.data_ptr()), capi.OUT_DEVICE) == 1
    back = np.empty(occ.shape, dtype=np.uint32)
    assert capi.DeviceArray.hip().hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr()), back.nbytes, 2) == 0   # DeviceToHost
    assert np.array_equal(back, host)
    s.set_collision_grid(None)
    assert s.collision_grid() is None
    assert s.L.loikb_collision_get_world_grid(s.h, None, None, None, None, 0) == 0
    assert s.L.loikb_collision_get_world_grid(s.h, None, None, None, None, 2) == -20      # LOIKB_ERR_ARG for bad flags, grid or no grid
