"""The Lindemann index without a GPU: ``LindemannParameter`` — its attributes, dtypes, shapes, what stays ``None``, what it
refuses — with the numpy restatement of tests/_lindemann_ref.py installed as ``kernels.lindemann``; that restatement against a
plain triple loop over the formulas; and the argument checks of the real shim, which come before any device work."""
import math

import numpy as np
import pytest

import _lindemann_ref
import mdapy_amd as mp
from mdapy_amd import _lindemann, lindemann_parameter  # noqa: F401  (what this file is about)


@pytest.fixture
def restated(monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "lindemann", _lindemann_ref)
    return _lindemann_ref


def _trajectory(F, N, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 2.0, (1, N, 3)) + rng.normal(0.0, 0.3, (F, N, 3))


def _loops(pos):
    """the formulas of the issue, pair by pair and frame by frame; sums in index order"""
    F, N = pos.shape[:2]

    def dist(f, i, j):
        dx, dy, dz = (float(pos[f, i, c]) - float(pos[f, j, c]) for c in range(3))
        return math.sqrt(dx * dx + dy * dy + dz * dz)

    # global mode
    total = 0.0
    for i in range(N):
        for j in range(i + 1, N):
            s1 = s2 = 0.0
            for f in range(F):
                r = dist(f, i, j)
                s1 += r
                s2 += r * r
            delta = s2 / F - (s1 / F) * (s1 / F)
            if delta > 0:
                total += math.sqrt(delta) / (s1 / F)
    trj = total / (N * (N - 1) / 2)
    # full mode
    mean, var = np.zeros((N, N)), np.zeros((N, N))
    frame, atom = np.zeros(F), np.zeros((F, N))
    for f in range(F):
        for i in range(N):
            for j in range(N):
                if i != j:
                    r = dist(f, i, j)
                    delta = r - mean[i, j]
                    mean[i, j] += delta / (f + 1)
                    var[i, j] += delta * (r - mean[i, j])
        for i in range(N):
            for j in range(N):
                if i != j and var[i, j] > 0:
                    term = math.sqrt(var[i, j] / (f + 1)) / mean[i, j]
                    frame[f] += term / (N * (N - 1))
                    atom[f, i] += term / (N - 1)
    return trj, frame, atom, mean, var


def test_restatement_against_plain_loops():
    pos = _trajectory(4, 6, 3)
    got = _lindemann_ref.restate(pos)
    trj, frame, atom, mean, var = _loops(pos)
    assert np.array_equal(got.mean, mean) and np.array_equal(got.var, var)  # the same operations on the same numbers
    assert np.allclose(got.frame, frame, rtol=1e-14, atol=0) and np.allclose(got.atom, atom, rtol=1e-14, atol=0)
    assert math.isclose(got.trj, trj, rel_tol=1e-14)
    assert not got.frame[0] and not got.atom[0].any() and np.all(got.frame[1:] > 0)
    assert np.array_equal(got.mean, got.mean.T) and np.array_equal(got.var, got.var.T) and not got.mean.diagonal().any()
    assert got.var_positive.shape == (4, 6, 6) and got.var_positive[1:].sum() == 3 * 30 and got.delta_positive.sum() == 15
    # the module's two functions fill the caller's arrays as the reference's do
    s1, s2 = np.full((6, 6), -1.0), np.full((6, 6), -1.0)
    assert _lindemann_ref.compute_global(pos, s1, s2, 1) == got.trj
    assert np.all(s1[~got.upper] == -1.0) and np.array_equal(s1[got.upper], got.sum[got.upper]) and np.all(s2[got.upper] > 0)
    f_out, a_out = np.zeros(4), np.zeros((4, 6))
    _lindemann_ref.compute_all(pos, None, None, f_out, a_out)
    assert np.array_equal(f_out, got.frame) and np.array_equal(a_out, got.atom)


def test_class_attributes(restated):
    assert mp.LindemannParameter is mp.lindemann_parameter.LindemannParameter and "LindemannParameter" in mp.__all__
    assert not hasattr(mp.LindemannParameter, "plot")
    pos = _trajectory(5, 9, 1)
    want = restated.restate(pos)
    full = mp.LindemannParameter(pos)
    assert full.only_global is False and full.lindemann_frame is None and full.lindemann_atom is None
    assert full.compute() is None
    assert type(full.lindemann_trj) is float and full.lindemann_trj == want.frame[-1]
    assert isinstance(full.lindemann_frame, np.ndarray) and full.lindemann_frame.dtype == np.float64 and full.lindemann_frame.shape == (5,)
    assert isinstance(full.lindemann_atom, np.ndarray) and full.lindemann_atom.dtype == np.float64 and full.lindemann_atom.shape == (5, 9)
    assert np.array_equal(full.lindemann_frame, want.frame) and np.array_equal(full.lindemann_atom, want.atom)
    only = mp.LindemannParameter(pos, only_global=True)
    only.compute()
    assert type(only.lindemann_trj) is float and only.lindemann_trj == want.trj
    assert only.lindemann_frame is None and only.lindemann_atom is None
    assert np.isclose(only.lindemann_trj, full.lindemann_trj)
    # convertible input, as the reference's np.ascontiguousarray(pos_list, dtype=float64) takes it
    as_list = mp.LindemannParameter(pos.tolist(), only_global=True)
    as_list.compute()
    strided = mp.LindemannParameter(np.asfortranarray(pos), only_global=True)
    strided.compute()
    assert as_list.lindemann_trj == want.trj and strided.pos_list.flags.c_contiguous and strided.lindemann_trj == want.trj


def test_class_never_asks_for_the_pair_tables(monkeypatch):
    import mdapy_amd.kernels as K

    seen = []

    class Spy:
        @staticmethod
        def compute_global(pos_list, pos_mean, pos_variance, num_t):
            seen.append(("global", pos_mean, pos_variance))
            return 0.25

        @staticmethod
        def compute_all(pos_list, pos_mean, pos_variance, lindemann_frame, lindemann_atom):
            seen.append(("all", pos_mean, pos_variance))
            lindemann_frame[...] = 0.5
            lindemann_atom[...] = 0.5

    monkeypatch.setattr(K, "lindemann", Spy)
    pos = _trajectory(3, 4, 0)
    a = mp.LindemannParameter(pos, only_global=True)
    a.compute()
    b = mp.LindemannParameter(pos)
    b.compute()
    assert seen == [("global", None, None), ("all", None, None)]
    assert a.lindemann_trj == 0.25 and b.lindemann_trj == 0.5


@pytest.mark.parametrize("shape", [(5, 4), (5, 4, 2), (5, 1, 3), (0, 4, 3), (5, 4, 3, 1)])
def test_class_refuses_other_shapes(restated, shape):
    with pytest.raises(ValueError, match="pos_list"):
        mp.LindemannParameter(np.zeros(shape))
    with pytest.raises(ValueError, match="pos_list"):
        mp.LindemannParameter(np.zeros(shape), only_global=True)


def test_shim_checks_arguments_before_any_device_work():
    """through the real ``kernels.lindemann`` on host arrays: a bad argument is a ValueError (from the shim or from the library's
    MDH_ERR_ARG) on any machine; valid arguments reach the device, and without one the library says so"""
    from mdapy_amd import _lib, kernels

    shim = kernels.lindemann
    assert shim.__name__ == "mdapy_amd._lindemann" and "lindemann" not in kernels.NAMES
    frame, atom = np.zeros(3), np.zeros((3, 4))
    for bad in (np.zeros((3, 4)), np.zeros((3, 4, 2)), np.zeros((3, 1, 3)), np.zeros((0, 4, 3))):
        F, N = bad.shape[0], bad.shape[1]
        with pytest.raises(ValueError):
            shim.compute_global(bad, None, None, 1)
        with pytest.raises(ValueError):
            shim.compute_all(bad, None, None, np.zeros(F), np.zeros((F, N)))
    pos = _trajectory(3, 4, 2)
    with pytest.raises(ValueError, match="pos_mean"):
        shim.compute_global(pos, np.zeros((4, 3)), None, 1)
    with pytest.raises(ValueError, match="lindemann_atom"):
        shim.compute_all(pos, None, None, frame, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="go together"):
        shim.compute_all(pos, np.zeros((4, 4)), None, frame, atom)
    with pytest.raises(ValueError, match="segments"):
        shim.compute_all(pos, None, None, frame, atom, segments=-2)
    L = _lib.lib()
    out = np.zeros(1)
    assert L.mdh_lindemann_global(None, 3, 4, None, None, out.ctypes.data, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_lindemann_all(pos.ctypes.data, 3, 4, None, None, None, atom.ctypes.data, 0, _lib.HOST, None) == _lib.ERR_ARG
    if _lib.device_count() > 0:
        return  # (with a device the valid calls compute: test_gpu_lindemann.py)
    with pytest.raises(RuntimeError, match="HIP error"):
        shim.compute_global(pos, None, None, 1)
    with pytest.raises(RuntimeError, match="HIP error"):
        shim.compute_all(pos, None, None, frame, atom)
