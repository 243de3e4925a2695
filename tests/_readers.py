"""One file through both tokenizers of load_save.read_file — the device's (whatever the file's size) and the host's — for
the GPU tests that compare them (test_gpu_load_save.py, test_gpu_text.py)."""
import numpy as np

import mdapy_amd.load_save as LS


def both(path, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(LS, "DEVICE_MIN_BYTES", 0)
        dev = LS.read_file(path)
    with monkeypatch.context() as m:
        m.setattr(LS, "have_gpu", lambda: False)
        host = LS.read_file(path)
    return dev, host


def same(dev, host):
    assert dev[0].columns == host[0].columns and dev[2] == host[2]
    assert np.array_equal(dev[1].box, host[1].box) and np.array_equal(dev[1].origin, host[1].origin)
    for c in dev[0].columns:
        a, b = dev[0][c].to_numpy(), host[0][c].to_numpy()
        if a.dtype == object or b.dtype == object:
            assert list(a) == list(b), c
        else:
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), c
