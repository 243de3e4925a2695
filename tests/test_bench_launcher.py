"""bench.py's own rank launcher (no GPU needed for what is checked here): `python bench.py --gpus N` must never exit without
ONE JSON line on stdout — a result, or an "error".  The last test (-m gpu) runs the plain single-GPU line and its --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MDH_BENCH_SHARED_GPU")}
    env.update(extra)
    return env


def _json_lines(text):
    return [json.loads(ln) for ln in text.splitlines() if ln.startswith("{")]


def test_more_ranks_than_gpus_is_an_error_line():
    import torch

    n = torch.cuda.device_count() + 2
    run = subprocess.run([sys.executable, "bench.py", "--gpus", str(n), "--steps", "1", "--warmup", "0", "--cells", "8"], cwd=ROOT, env=_clean_env(),
                         capture_output=True, text=True, timeout=300)
    got = _json_lines(run.stdout)
    assert run.returncode != 0 and len(got) == 1
    assert got[0]["n_gpus"] == n and got[0]["value"] is None and "visible GPU" in got[0]["error"]


def test_a_failing_rank_becomes_an_error_line_and_the_others_are_stopped():
    """two ranks are started (shared-GPU switch: no device count check in the launcher); without a GPU each of them fails when it
    selects its device — the launcher must report the first failure with that rank's stderr and exit non-zero"""
    import torch

    if torch.cuda.is_available():
        import pytest

        pytest.skip("the ranks would run; the failing-rank case on a GPU box is in tests/test_gpu_distributed.py")
    run = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0", "--cells", "8"], cwd=ROOT,
                         env=_clean_env(MDH_BENCH_SHARED_GPU="1", MDH_BENCH_LAUNCH_TIMEOUT="240"), capture_output=True, text=True, timeout=400)
    got = _json_lines(run.stdout)
    assert run.returncode != 0 and len(got) == 1
    assert got[0]["error"].startswith("rank ") and " of 2 ended with " in got[0]["error"]


def test_world_size_and_gpus_must_agree():
    run = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0", "--cells", "8"], cwd=ROOT,
                         env=_clean_env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "must agree" in (run.stdout + run.stderr)


@pytest.mark.gpu
def test_plain_line_times_the_step_only_and_dumps_what_it_computed(tmp_path):
    """a plain run prints the headline without the --full figures; --dump-outputs writes the last timed step's arrays in
    float64, the same ones from run to run, and they are the perfect lattice's answer (12 neighbours, FCC, distance a / sqrt 2)"""
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--cells", "30", "--dump-outputs", str(d)],
                             cwd=ROOT, env=_clean_env(), capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
        got = _json_lines(run.stdout)
        assert len(got) == 1
        res = got[0]
        assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["higher_is_better"] is True
        assert abs(res["value"] - 4 * 30 ** 3 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]
        assert not {"roofline", "kernels_ms", "extra", "cpu_baseline"} & set(res)
        dumps.append({p.stem: np.load(p) for p in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) == {"atom_index", "neighbor_number", "cna", "verlet_list", "distance_list"}
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    n = 4 * 30 ** 3  # (below DUMP_ROWS: every atom is dumped)
    assert np.array_equal(a["atom_index"], np.arange(n)) and a["verlet_list"].shape == (n, 16)
    assert (a["neighbor_number"] == 12).all() and (a["cna"] == 1).all()
    assert np.allclose(a["distance_list"][:, :12], 3.615 / np.sqrt(2.0))
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    # the same plain line at two ranks (both on this GPU, gloo): no exchange or strong-scaling figures without --full
    run = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--cells", "20"], cwd=ROOT,
                         env=_clean_env(MDH_BENCH_SHARED_GPU="1"), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    res = _json_lines(run.stdout)[0]
    assert res["n_gpus"] == 2 and res["value"] > 0 and "strong" not in res["config"] and "exchange_ms" not in res["config"]
