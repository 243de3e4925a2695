"""``mdapy_amd.potential_tool`` without a GPU: the host side of ``fps_sample``, ``PCA`` and ``rmse`` with the numpy restatement of
tests/_fps_ref.py installed as ``kernels.sample``; the two restated rules against each other; what the real shim refuses before
any device work."""
import os

import numpy as np
import pytest

import _fps_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca", "pca.npz")


@pytest.fixture
def restated(monkeypatch):
    from mdapy_amd import kernels as K

    monkeypatch.setattr(K, "sample", _fps_ref.Shim)
    from mdapy_amd import potential_tool

    return potential_tool


# (N, D, n_sample) of the integer cases: tests/test_gpu_potential_tool.py runs the same on the device
SHAPES = [(1, 1, 1), (7, 1, 7), (257, 3, 257), (300, 8, 300), (1000, 30, 200), (5000, 33, 300), (4096, 16, 64), (70001, 5, 50)]


def integer_table(N, D):
    return np.random.default_rng(1000 * D + N).integers(-50, 51, (N, D)).astype(np.float64)


def test_module_is_not_reexported():
    import mdapy_amd

    assert not hasattr(mdapy_amd, "fps_sample") and not hasattr(mdapy_amd, "PCA")
    from mdapy_amd import kernels

    assert kernels.sample.__name__ == "mdapy_amd._sample" and "sample" not in kernels.NAMES


@pytest.mark.parametrize("call, message", [
    (lambda f: f(3, np.zeros(10)), "Only support 2-D ndarray."),
    (lambda f: f(3, np.zeros((2, 3, 4))), "Only support 2-D ndarray."),
    (lambda f: f(0, np.zeros((10, 2))), "n_sample must be a positive number."),
    (lambda f: f(11, np.zeros((10, 2))), "n_sample must <= 10."),
    (lambda f: f(3, np.zeros((10, 2)), start_idx=10), "start_idx must belong [0, 9]."),
    (lambda f: f(3, np.zeros((10, 2)), start_idx=-1), "start_idx must belong [0, 9]."),
])
def test_argument_errors_carry_the_reference_messages(restated, call, message):
    with pytest.raises(ValueError) as caught:
        call(restated.fps_sample)
    assert str(caught.value) == message


@pytest.mark.parametrize("N, D, n", SHAPES)
def test_fps_sample_is_the_reference_rule_on_integer_tables(restated, N, D, n):
    """on integer data every difference, square and sum is exact: the squared rule and the norm rule see the same order"""
    X = integer_table(N, D)
    for start in sorted({0, N // 3, N - 1}):
        got = restated.fps_sample(n, X, start)
        assert got.dtype == np.int32 and got.shape == (n,) and got[0] == start
        assert np.array_equal(got, _fps_ref.fps_norm(n, X, start))


def test_fps_sample_quarter_lattice_and_identical_points(restated):
    X = np.random.default_rng(12).integers(-400, 401, (3000, 12)) * 0.25
    assert np.array_equal(restated.fps_sample(500, X), _fps_ref.fps_norm(500, X, 0))
    assert restated.fps_sample(5, np.ones((50, 4)), start_idx=3).tolist() == [3, 0, 0, 0, 0]
    assert _fps_ref.fps_norm(5, np.ones((50, 4)), 3).tolist() == [3, 0, 0, 0, 0]


def test_return_distance_is_the_root_of_the_minima(restated):
    X = np.random.default_rng(3).random((400, 7))
    picks, distance = restated.fps_sample(40, X, start_idx=11, return_distance=True)
    want, minima = _fps_ref.fps_squared(40, X, 11)
    assert np.array_equal(picks, want)
    assert distance.dtype == np.float64 and np.array_equal(distance, np.sqrt(minima))
    assert np.all(distance[picks[:-1]] == 0.0) and distance.max() == distance[picks[-1]]
    alone, far = restated.fps_sample(1, X, return_distance=True)
    assert alone.tolist() == [0] and np.all(np.isinf(far))


def test_input_forms_on_the_host(restated):
    X = np.random.default_rng(4).integers(-9, 10, (60, 6)).astype(np.float64)
    want = _fps_ref.fps_norm(20, X, 5)
    assert np.array_equal(restated.fps_sample(20, X.astype(np.float32), 5), want)
    assert np.array_equal(restated.fps_sample(20, X.tolist(), 5), want)
    wide = np.zeros((60, 12))
    wide[:, ::2] = X
    assert np.array_equal(restated.fps_sample(20, wide[:, ::2], 5), want)


def test_pca_meets_the_recorded_result(restated):
    data = np.load(GOLDEN)
    np.random.seed(int(data["seed"]))
    X = np.random.random((int(data["n_samples"]), int(data["n_features"])))
    model = restated.PCA(n_components=int(data["n_components"]))
    assert model.explained_variance is None and model.explained_variance_ratio is None
    got = model.fit_transform(X)
    assert got.shape == data["transformed"].shape
    assert np.allclose(got, data["transformed"])
    assert np.allclose(model.explained_variance, data["explained_variance"])
    ratio = model.explained_variance_ratio
    assert ratio.shape == (3,) and np.all(ratio > 0) and ratio.sum() <= 1.0 and np.all(np.diff(ratio) <= 0)
    mine, variance, share = _fps_ref.pca(X, 3)
    assert np.allclose(got, mine, rtol=0, atol=1e-13) and np.allclose(variance, model.explained_variance, rtol=1e-13)
    assert abs(np.abs(mine - data["transformed"]).max()) < 1e-13


def test_pca_small_inputs(restated):
    X = np.random.default_rng(5).random((30, 4))
    full = restated.PCA(9)
    out = full.fit_transform(X)
    assert out.shape == (30, 4) and full.explained_variance.shape == (4,)
    assert abs(full.explained_variance_ratio.sum() - 1.0) < 1e-12
    assert np.allclose(np.cov(out.T), np.diag(full.explained_variance), atol=1e-12)  # the components are uncorrelated
    assert restated.PCA(1).fit_transform(np.array([[0.0], [2.0]])).tolist() == [[-1.0], [1.0]]
    with pytest.raises(ValueError):
        restated.PCA(2).fit_transform(np.ones((1, 4)))
    with pytest.raises(ValueError):
        restated.PCA(2).fit_transform(np.ones(4))
    with pytest.raises(ValueError):
        restated.PCA(0).fit_transform(X)


def test_rmse():
    from mdapy_amd.potential_tool import rmse

    assert rmse(np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0])) == 0.0
    assert rmse(np.array([3.0, 0.0]), np.array([0.0, 4.0])) == np.sqrt(12.5)
    a, b = np.random.default_rng(6).random((2, 5, 3))
    assert rmse(a, b) == np.sqrt(((a - b) ** 2).mean())


def test_shim_rejects_mismatched_shapes_before_any_device_work():
    """through the real ``kernels.sample`` on host arrays: every one of these is a ValueError of the shim itself — on a machine
    without a GPU a call that reached the library would be a RuntimeError"""
    from mdapy_amd import kernels

    shim = kernels.sample
    X = np.zeros((10, 3))
    picks = np.zeros(4, np.int32)
    with pytest.raises(ValueError):
        shim.fps(np.zeros(10), 4, 0, picks)
    with pytest.raises(ValueError):
        shim.fps(X, 5, 0, picks)  # picks is (4,)
    with pytest.raises(ValueError):
        shim.fps(X, 4, 0, picks, np.zeros(9))
    with pytest.raises(ValueError):
        shim.fps(X, 4, 10, picks)
    with pytest.raises(ValueError):
        shim.fps(X, 11, 0, np.zeros(11, np.int32))
    with pytest.raises(ValueError):
        shim.fps(X, 4, 0, picks, _path="tiles")
    with pytest.raises(TypeError):
        shim.fps(X, 4, 0, np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        shim.moments(X, np.zeros(4), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        shim.moments(X, np.zeros(3), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        shim.moments(np.zeros((1, 3)), np.zeros(3), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        shim.project(X, np.zeros(3), np.zeros((4, 2)), np.zeros((10, 2)))
    with pytest.raises(ValueError):
        shim.project(X, np.zeros(3), np.zeros((3, 2)), np.zeros((10, 3)))
    with pytest.raises(ValueError):
        shim.project(X, np.zeros(2), np.zeros((3, 2)), np.zeros((10, 2)))
    assert shim.block_path_takes(70001, 5) and not shim.block_path_takes(10 ** 6, 30) and not shim.block_path_takes(10, 513)
