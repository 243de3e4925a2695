"""Farthest-point sampling and the PCA on the GPU: ``kernels.sample`` (csrc/sample.hip) and ``mdapy_amd.potential_tool`` against
the numpy restatements of tests/_fps_ref.py.

Sampling is compared with ``np.array_equal`` — picks AND squared minima: both sides evaluate the pinned sum, the same IEEE
binary64 operations in the same order, on every path.  The reference's own rule (norms) is compared on data where it must agree:
integers and quarter-integers, whose differences, squares and sums are exact, so that two different squared minima are two
different integers (times 1/16) below 2^53 and their roots cannot round together.

The PCA's sums are compared with the exactly added (``math.fsum``) terms within the first-order bound of a sum of n terms taken
in any order, n 2^-53 sum |term|, doubled for the roundings of the products and of the final division."""
import functools
import os

import numpy as np
import pytest

import _fps_ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca", "pca.npz")
# (N, D, n_sample): one row; one column; every point picked (one tile and a ragged second one on either path); two chunks of
# features on the one-workgroup path; an odd D that no chunk width divides; whole tiles; many workgroups with a ragged last one
SHAPES = [(1, 1, 1), (7, 1, 7), (257, 3, 257), (300, 8, 300), (1000, 30, 200), (5000, 33, 300), (4096, 16, 64), (70001, 5, 50)]
PATHS = ("grid", "block")


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_potential_tool needs a HIP device")


@functools.lru_cache(maxsize=None)
def table(kind, N, D):
    rng = np.random.default_rng(1000 * D + N)
    if kind == "continuous":
        X = rng.random((N, D))
    elif kind == "integer":
        X = rng.integers(-50, 51, (N, D)).astype(np.float64)
    elif kind == "ties":
        X = rng.integers(0, 4, (N, D)).astype(np.float64)
    else:
        X = rng.integers(-400, 401, (N, D)) * 0.25
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def want(kind, N, D, n, start):
    """(picks, squared minima) of the restatement, made once; read-only"""
    picks, minima = _fps_ref.fps_squared(n, table(kind, N, D), start)
    picks.setflags(write=False)
    minima.setflags(write=False)
    return picks, minima


def device(X, n, start=0, path=None):
    from mdapy_amd import kernels

    picks = np.full(n, -1, np.int32)
    minima = np.full(X.shape[0], np.nan)
    taken = kernels.sample.fps(X, n, start, picks, minima, _path=path)
    assert taken == (path or taken) and taken in PATHS
    return picks, minima


def starts(N):
    return sorted({0, N // 3, N - 1})


# ---- 1. the pinned sum, both paths
@pytest.mark.parametrize("kind", ["continuous", "integer"])
@pytest.mark.parametrize("N, D, n", SHAPES)
def test_fps_equals_the_restatement_bit_for_bit(N, D, n, kind):
    from mdapy_amd import kernels

    X = table(kind, N, D)
    assert kernels.sample.block_path_takes(N, D)  # (every shape of this file fits the one-workgroup path)
    for start in starts(N):
        picks, minima = want(kind, N, D, n, start)
        for path in PATHS:
            got, got_minima = device(X, n, start, path)
            assert np.array_equal(got, picks), (path, start)
            assert np.array_equal(got_minima, minima), (path, start)


def test_the_library_chooses_a_path_by_size():
    assert device(table("continuous", 300, 8), 5)[0].tolist() == want("continuous", 300, 8, 5, 0)[0].tolist()
    from mdapy_amd import kernels

    X = table("continuous", 70001, 5)
    picks = np.empty(3, np.int32)
    assert kernels.sample.fps(X, 3, 0, picks) == "grid"
    assert kernels.sample.fps(table("continuous", 7, 1), 3, 0, picks) == "block"
    with pytest.raises(ValueError):  # beyond what one workgroup takes
        kernels.sample.fps(np.zeros((2100, 513)), 3, 0, picks, _path="block")


# ---- 2. the reference's rule
@pytest.mark.parametrize("N, D, n", SHAPES)
def test_fps_sample_equals_the_reference_rule_on_integer_tables(N, D, n):
    from mdapy_amd.potential_tool import fps_sample

    X = table("integer", N, D)
    for start in starts(N):
        by_norm = _fps_ref.fps_norm(n, X, start)
        assert np.array_equal(by_norm, want("integer", N, D, n, start)[0])  # the two rules agree on this input ...
        got = fps_sample(n, X, start)
        assert got.dtype == np.int32 and np.array_equal(got, by_norm)  # ... and the device with them


def test_fps_sample_equals_the_reference_rule_on_a_quarter_lattice():
    from mdapy_amd.potential_tool import fps_sample

    X = table("quarter", 3000, 12)
    by_norm = _fps_ref.fps_norm(500, X, 0)
    assert np.array_equal(by_norm, want("quarter", 3000, 12, 500, 0)[0])
    picks, distance = fps_sample(500, X, return_distance=True)
    assert np.array_equal(picks, by_norm)
    assert np.array_equal(distance, np.sqrt(want("quarter", 3000, 12, 500, 0)[1]))
    for path in PATHS:
        assert np.array_equal(device(X, 500, 0, path)[0], by_norm)


# ---- 3. ties
def test_ties_across_workgroups_go_to_the_lowest_row():
    X = table("ties", 70001, 5)
    picks, minima = want("ties", 70001, 5, 50, 0)
    tied = 0  # steps whose maximum is held by rows of different 128-row tiles
    running = np.full(70001, np.inf)
    for s in range(49):
        running = np.minimum(running, _fps_ref.squared_distances(X, picks[s]))
        holders = np.flatnonzero(running == running.max())
        tied += len(set(holders // 128)) > 1
    assert tied >= 40
    for path in PATHS:
        got, got_minima = device(X, 50, 0, path)
        assert np.array_equal(got, picks) and np.array_equal(got_minima, minima), path


def test_identical_points():
    for path in PATHS:
        assert device(np.ones((50, 4)), 5, 3, path)[0].tolist() == [3, 0, 0, 0, 0]


# ---- 4. 5. state between calls, repeatability
def test_calls_leave_nothing_behind():
    big, small = table("continuous", 70001, 5), table("continuous", 7, 1)
    for path in PATHS:
        first = device(big, 50, 23333, path)
        between = device(small, 7, 2, path)
        again = device(big, 50, 23333, path)
        for got in (first, again):
            assert np.array_equal(got[0], want("continuous", 70001, 5, 50, 23333)[0]), path
            assert np.array_equal(got[1], want("continuous", 70001, 5, 50, 23333)[1]), path
        assert np.array_equal(between[0], want("continuous", 7, 1, 7, 2)[0]), path
        assert np.array_equal(between[1], want("continuous", 7, 1, 7, 2)[1]), path


def test_two_runs_give_the_same_bits():
    X = table("continuous", 5000, 33)
    for path in PATHS:
        a, b = device(X, 300, 7, path), device(X, 300, 7, path)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 6. input forms
def test_input_forms():
    import torch

    from mdapy_amd.devarray import HArray
    from mdapy_amd.potential_tool import fps_sample

    X32 = np.random.default_rng(8).random((3000, 12)).astype(np.float32)
    X = X32.astype(np.float64)
    base = fps_sample(100, X, 17)
    assert np.array_equal(base, _fps_ref.fps_squared(100, X, 17)[0])
    assert np.array_equal(fps_sample(100, X32, 17), base)
    wide = np.zeros((3000, 24))
    wide[:, ::2] = X
    assert np.array_equal(fps_sample(100, wide[:, ::2], 17), base)
    assert np.array_equal(fps_sample(100, HArray.from_numpy(X), 17), base)
    tensor = torch.from_numpy(X).cuda()
    assert np.array_equal(fps_sample(100, tensor, 17), base)
    assert np.array_equal(fps_sample(100, torch.from_numpy(wide).cuda()[:, ::2], 17), base)
    assert np.array_equal(fps_sample(100, torch.from_numpy(X32).cuda(), 17), base)
    picks, distance = fps_sample(100, tensor, 17, return_distance=True)
    assert np.array_equal(picks, base) and np.array_equal(distance, np.sqrt(_fps_ref.fps_squared(100, X, 17)[1]))


# ---- 7. non-finite input
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_value_that_is_not_finite_is_refused(value):
    from mdapy_amd.potential_tool import fps_sample

    X = table("continuous", 70001, 5).copy()
    X[-1, 4] = value
    with pytest.raises(ValueError, match="not finite"):
        fps_sample(50, X)
    small = np.ones((300, 8))
    small[299, 7] = value
    for path in PATHS:
        with pytest.raises(ValueError, match="not finite"):
            device(small, 10, 0, path)
    # and the next call is a clean one
    assert np.array_equal(fps_sample(50, table("continuous", 70001, 5)), want("continuous", 70001, 5, 50, 0)[0])


# ---- 8. other streams
def test_on_another_stream():
    import torch

    from mdapy_amd.potential_tool import fps_sample

    X = table("continuous", 70001, 5)
    tensor = torch.from_numpy(X.copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = fps_sample(50, tensor, 70000)
        small = fps_sample(257, torch.from_numpy(table("integer", 257, 3).copy()).cuda(), 85)
    assert np.array_equal(got, want("continuous", 70001, 5, 50, 70000)[0])
    assert np.array_equal(small, want("integer", 257, 3, 257, 85)[0])


# ---- PCA
PCA_SHAPES = [(2, 1), (100, 20), (1000, 33), (70001, 5)]


@functools.lru_cache(maxsize=None)
def pca_table(N, D):
    rng = np.random.default_rng(77 * D + N)
    X = rng.normal(0.0, 1.0, (N, D)) * rng.uniform(0.1, 3.0, D) + rng.uniform(-5.0, 5.0, D)
    X.setflags(write=False)
    return X


def device_moments(X):
    from mdapy_amd import kernels

    D = X.shape[1]
    mean, cov = np.full(D, np.nan), np.full((D, D), np.nan)
    kernels.sample.moments(X, mean, cov)
    return mean, cov


def device_project(X, mean, components):
    from mdapy_amd import kernels

    out = np.full((X.shape[0], components.shape[1]), np.nan)
    kernels.sample.project(X, mean, components, out)
    return out


@pytest.mark.parametrize("N, D", PCA_SHAPES)
def test_pca_moments_within_the_bound_of_a_sum(N, D):
    X = pca_table(N, D)
    mean, cov = device_moments(X)
    means, mass, exact, exact_mass = _fps_ref.exact_moments(X, mean)
    assert np.all(np.abs(mean - means) <= 2 * N * EPS * mass / N)
    assert np.all(np.abs(cov - exact) <= 2 * N * EPS * exact_mass / (N - 1))
    assert np.array_equal(cov, cov.T)
    again = device_moments(X)
    assert np.array_equal(again[0], mean) and np.array_equal(again[1], cov)


@pytest.mark.parametrize("N, D", PCA_SHAPES)
def test_pca_projection_within_the_bound_of_a_sum(N, D):
    X = pca_table(N, D)
    rng = np.random.default_rng(N + D)
    mean = X.mean(axis=0)
    for C in sorted({1, min(D, 3), min(D, 11)}):  # (11: more than the eight components of one walk over a row)
        components = rng.normal(0.0, 1.0, (D, C))
        got = device_project(X, mean, components)
        exact, mass = _fps_ref.exact_projection(X, mean, components)
        assert np.all(np.abs(got - exact) <= 2 * D * EPS * mass), C
        assert np.array_equal(device_project(X, mean, components), got)


def test_a_constant_column_has_exactly_no_variance():
    """2.5 N is exact in binary64: the column sum, the mean and every centred value are, whatever the order of the sum"""
    X = pca_table(1000, 33).copy()
    X[:, 2] = 2.5
    mean, cov = device_moments(X)
    assert mean[2] == 2.5
    assert np.all(cov[2, :] == 0.0) and np.all(cov[:, 2] == 0.0) and np.all(np.diag(cov)[[0, 1, 3]] > 0)


def test_fit_transform_meets_the_recorded_result():
    import torch

    from mdapy_amd.potential_tool import PCA

    data = np.load(GOLDEN)
    np.random.seed(int(data["seed"]))
    X = np.random.random((int(data["n_samples"]), int(data["n_features"])))
    model = PCA(n_components=int(data["n_components"]))
    got = model.fit_transform(X)
    assert isinstance(got, np.ndarray) and np.allclose(got, data["transformed"])
    assert np.allclose(model.explained_variance, data["explained_variance"])
    assert model.explained_variance_ratio.sum() <= 1.0
    assert np.array_equal(PCA(3).fit_transform(torch.from_numpy(X).cuda()), got)
    assert np.array_equal(PCA(3).fit_transform(X.astype(np.float32).astype(np.float64)), PCA(3).fit_transform(X.astype(np.float32)))
    everything = PCA(50).fit_transform(X)
    assert everything.shape == (100, 20) and np.array_equal(everything[:, :3], got)
    with pytest.raises(ValueError):
        PCA(2).fit_transform(np.ones((1, 4)))
    with pytest.raises(ValueError):
        PCA(2).fit_transform(np.ones((10, 129)))
