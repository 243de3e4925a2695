"""The mean squared displacement without a GPU: the numpy restatement of tests/_msd_ref.py against plain loops over the
definition and against the S1 - 2 S2 / FFT formula; ``MeanSquaredDisplacement`` — its attributes, dtypes, shapes, what it
refuses — with that restatement installed as ``kernels.msd``; and the argument checks of the real shim, which come before any
device work."""
import math

import numpy as np
import pytest

import _msd_ref
import mdapy_amd as mp
from mdapy_amd import _msd, mean_squared_displacement  # noqa: F401  (what this file is about)

EPS = 2.0 ** -53


@pytest.fixture
def restated(monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "msd", _msd_ref)
    return _msd_ref


def _trajectory(F, N, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 2.0, (1, N, 3)) + np.cumsum(rng.normal(0.0, 0.3, (F, N, 3)), axis=0)


def _term(a, b):
    dx, dy, dz = (float(a[c]) - float(b[c]) for c in range(3))
    return (dx * dx + dy * dy) + dz * dz


def _loops(pos):
    """the definition, entry by entry; the sums rounded once (fsum), then divided once"""
    F, N = pos.shape[:2]
    window, direct = np.zeros((F, N)), np.zeros((F, N))
    for m in range(F):
        for i in range(N):
            window[m, i] = math.fsum(_term(pos[t + m, i], pos[t, i]) for t in range(F - m)) / (F - m)
            direct[m, i] = _term(pos[m, i], pos[0, i])
    window_msd = np.array([math.fsum(window[m, i] for i in range(N)) / N for m in range(F)])
    direct_msd = np.array([math.fsum(direct[m, i] for i in range(N)) / N for m in range(F)])
    return window, direct, window_msd, direct_msd


def test_restatement_against_plain_loops():
    pos = _trajectory(5, 4, 3)
    got = _msd_ref.restate(pos)
    window, direct, window_msd, direct_msd = _loops(pos)
    assert np.array_equal(got.window, window) and np.array_equal(got.direct, direct)  # the same operations on the same numbers
    assert np.array_equal(got.window_msd, window_msd) and np.array_equal(got.direct_msd, direct_msd)
    assert not got.window[0].any() and not got.direct[0].any() and np.all(got.window[1:] > 0)
    # the module's two functions fill the caller's arrays; either may be None; fewer rows = fewer lags
    table, mean = np.full((5, 4), np.nan), np.full(5, np.nan)
    _msd_ref.window(pos, table, mean)
    assert np.array_equal(table, window) and np.array_equal(mean, window_msd)
    short = np.full(3, np.nan)
    _msd_ref.window(pos, None, short)
    assert np.array_equal(short, window_msd[:3])
    _msd_ref.direct(pos, table, None)
    assert np.array_equal(table, direct)


def test_restatement_against_the_fft_formula():
    pos = _trajectory(37, 70, 11)
    want = _msd_ref.restate(pos).window
    got = _msd_ref.fft_window(pos)  # S1 - 2 S2 with numpy's double FFT, written from the docstring's formulas
    scale = float(np.square(pos).sum(axis=2).max())
    worst = float(np.abs(got - want).max())
    print(f"FFT formula against the restatement: worst difference {worst / (EPS * scale):.1f} x 2^-53 max |r|^2 (allowed 1024)")
    assert worst <= 1024 * EPS * scale


def test_class_attributes(restated):
    assert mp.MeanSquaredDisplacement is mp.mean_squared_displacement.MeanSquaredDisplacement
    assert "MeanSquaredDisplacement" in mp.__all__ and not hasattr(mp.MeanSquaredDisplacement, "plot")
    pos = _trajectory(6, 9, 1)
    want = restated.restate(pos)
    by_mode = {}
    for mode, table, mean in (("window", want.window, want.window_msd), ("direct", want.direct, want.direct_msd)):
        one = mp.MeanSquaredDisplacement(pos, mode=mode)
        assert one.mode == mode and one.pos_list is not None and one.particle_msd is None and one.msd is None
        assert one.compute() is None
        assert isinstance(one.particle_msd, np.ndarray) and one.particle_msd.dtype == np.float64 and one.particle_msd.shape == (6, 9)
        assert isinstance(one.msd, np.ndarray) and one.msd.dtype == np.float64 and one.msd.shape == (6,)
        assert np.array_equal(one.particle_msd, table) and np.array_equal(one.msd, mean)
        assert one.msd[0] == 0 and not one.particle_msd[0].any()
        by_mode[mode] = one
    assert mp.MeanSquaredDisplacement(pos).mode == "window"
    # at the last lag both modes are the one term |r[F-1] - r[0]|^2
    assert np.array_equal(by_mode["window"].particle_msd[-1], by_mode["direct"].particle_msd[-1])
    assert by_mode["window"].msd[-1] == by_mode["direct"].msd[-1]
    # convertible input: a list, float32, a strided array
    as_list = mp.MeanSquaredDisplacement(pos.tolist())
    as_list.compute()
    assert isinstance(as_list.pos_list, np.ndarray) and np.array_equal(as_list.particle_msd, want.window)
    single = pos.astype(np.float32)
    narrow = mp.MeanSquaredDisplacement(single, mode="direct")
    narrow.compute()
    assert narrow.pos_list.dtype == np.float64 and np.array_equal(narrow.particle_msd, restated.restate(single.astype(np.float64)).direct)
    strided = mp.MeanSquaredDisplacement(np.asfortranarray(pos))
    strided.compute()
    assert strided.pos_list.flags.c_contiguous and np.array_equal(strided.msd, want.window_msd)


@pytest.mark.parametrize("shape", [(5, 4), (5, 4, 2), (0, 4, 3), (5, 0, 3), (5, 4, 3, 1)])
def test_class_refuses_other_shapes(restated, shape):
    with pytest.raises(ValueError, match="pos_list"):
        mp.MeanSquaredDisplacement(np.zeros(shape))
    with pytest.raises(ValueError, match="pos_list"):
        mp.MeanSquaredDisplacement(np.zeros(shape), mode="direct")


def test_class_refuses_another_mode(restated):
    with pytest.raises(ValueError, match="mode"):
        mp.MeanSquaredDisplacement(np.zeros((3, 2, 3)), mode="fft")


def test_shim_checks_arguments_without_the_library():
    """the shim's own shape checks raise before the library is loaded: no device, no built library needed"""
    from mdapy_amd import kernels

    shim = kernels.msd
    assert shim.__name__ == "mdapy_amd._msd" and "msd" not in kernels.NAMES
    pos = _trajectory(3, 4, 2)
    for run in (shim.window, shim.direct):
        for bad in (np.zeros((3, 4)), np.zeros((3, 4, 2)), np.zeros((0, 4, 3)), np.zeros((3, 0, 3))):
            with pytest.raises(ValueError, match="pos_list"):
                run(bad, np.zeros((max(bad.shape[0], 1), bad.shape[1])), None)
        with pytest.raises(ValueError, match="both None"):
            run(pos, None, None)
        with pytest.raises(ValueError, match="particle_msd"):
            run(pos, np.zeros((3, 5)), np.zeros(3))
        with pytest.raises(ValueError, match="msd has shape"):
            run(pos, np.zeros((3, 4)), np.zeros(2))
        with pytest.raises(ValueError, match="msd has shape"):
            run(pos, None, np.zeros((3, 1)))
        with pytest.raises(ValueError, match="rows"):  # L > F
            run(pos, np.zeros((4, 4)), np.zeros(4))
        with pytest.raises(ValueError, match="rows"):
            run(pos, None, np.zeros(0))
    with pytest.raises(ValueError, match="fewer rows"):
        shim.direct(pos, None, np.zeros(2))


def test_library_checks_arguments_before_any_device_work():
    """the built library with host pointers: a bad size is MDH_ERR_ARG (ValueError in Python) on any machine; valid arguments
    reach the device, and without one the library says so"""
    from mdapy_amd import _lib, kernels

    shim = kernels.msd
    pos = _trajectory(3, 4, 2)
    L = _lib.lib()
    table, mean = np.zeros((3, 4)), np.zeros(3)
    p, t, m = pos.ctypes.data, table.ctypes.data, mean.ctypes.data
    assert L.mdh_msd_window(None, 3, 4, 3, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_window(p, 0, 4, 1, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_window(p, 3, 0, 3, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_window(p, 3, 4, 0, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_window(p, 3, 4, 4, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_window(p, 3, 4, 3, None, None, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_direct(None, 3, 4, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_direct(p, 0, 4, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_direct(p, 3, 0, t, m, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_msd_direct(p, 3, 4, None, None, _lib.HOST, None) == _lib.ERR_ARG
    with pytest.raises(ValueError, match="both NULL"):
        _lib.check(L.mdh_msd_direct(p, 3, 4, None, None, _lib.HOST, None))
    if _lib.device_count() > 0:
        return  # (with a device the valid calls compute: test_gpu_msd.py)
    with pytest.raises(RuntimeError, match="HIP error"):
        shim.window(pos, table, mean)
    with pytest.raises(RuntimeError, match="HIP error"):
        shim.direct(pos, None, mean)
