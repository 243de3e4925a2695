"""The values the number formatter is pinned on, shared by the host test (test_text_format.py) and the GPU test
(test_gpu_text_format.py): generated from seeds, never from what the formatter returns."""
import math

import numpy as np


def tie_values():
    """every +-(b + j / 2048), j odd below 4096: the eleventh decimal is a 5 followed by zeros, so each is an exact tie"""
    j = np.arange(1, 4096, 2, dtype=np.float64) / 2048.0
    pos = np.concatenate([b + j for b in (0.0, 1.0, 7.0, 123456.0, float(2 ** 40))])
    return np.concatenate([pos, -pos])


SPECIAL = [0.99999999995, 9.99999999995, 99999.99999999999, -0.0, -1e-12, 4.99999999995e-11, 5e-11, 5e-324, 1e-300,
           float(2 ** 53 + 1), float(2 ** 53 - 1), float(2 ** 63), math.nextafter(float(2 ** 64), 0.0), 0.0, 1.0, -1.0, 0.5, -123456789.25]


def random_bit_patterns(n=100_000, seed=11):
    """doubles with random sign and mantissa and a binary exponent drawn from -63 .. 63"""
    rng = np.random.default_rng(seed)
    bits = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) | ((rng.integers(-63, 64, n) + 1023).astype(np.uint64) << np.uint64(52)) \
        | rng.integers(0, 2 ** 52, n, dtype=np.uint64)
    return bits.view(np.float64)


def uniform_values(n=100_000, seed=12):
    return np.random.default_rng(seed).uniform(-200.0, 200.0, n)


def value_classes():
    """all the finite doubles the formatter is pinned on, in one array (shared with the GPU test)"""
    return np.concatenate([tie_values(), np.array(SPECIAL), random_bit_patterns(), uniform_values()])


def int_classes():
    out = [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 63 - 1, -2 ** 63]
    for k in range(19):
        out += [10 ** k, -(10 ** k), 10 ** k - 1, -(10 ** k - 1)]
    return out
