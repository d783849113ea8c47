"""``bench.py`` command line: a plain run's result line, ``--dump-outputs`` and
``--full`` (on whatever device the process finds; tiny CIFAR ResNets)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--batch", "4", "DISTILLER.STUDENT", "resnet8", "DISTILLER.TEACHER", "resnet20"]


def _bench(*args):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, *TINY],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """Two plain runs with the same arguments, each with its own dump folder."""
    dirs = [str(tmp_path_factory.mktemp(f"dump{i}")) for i in range(2)]
    return [(_bench("--steps", "2", "--warmup", "1", "--dump-outputs", d), d) for d in dirs]


def test_plain_run_result_line(dumped):
    r, _ = dumped[0]
    assert r["steps"] == 2 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["unit"] == "images/s" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps (both are rounded)
    assert r["value"] == pytest.approx(4 * 1000.0 / r["ms_per_step"], rel=1e-3)
    # what only --full measures is absent from a plain run
    assert r["host_idle_ms_per_step"] is None and r["replicas_identical"] is None


def test_dump_outputs_files_and_repeatability(dumped):
    (r0, d0), (r1, d1) = dumped
    names = sorted(f[:-4] for f in os.listdir(d0) if f.endswith(".npy"))
    assert names == r0["outputs"] == r1["outputs"]
    assert "preds" in names and any(n.startswith("loss") for n in names)
    total = 0
    for n in names:
        a, b = np.load(os.path.join(d0, n + ".npy")), np.load(os.path.join(d1, n + ".npy"))
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all()
        total += a.nbytes
        # same seeded data and weights in both runs.  3 steps of a bf16 step whose
        # backward sums with atomics: a few bf16 ulps (2^-8 relative) of O(1) values
        np.testing.assert_allclose(a, b, rtol=4 * 2.0 ** -8, atol=4 * 2.0 ** -8)
    assert np.load(os.path.join(d0, "preds.npy")).shape == (4, 100)
    assert total <= 64 << 20


def test_full_run_adds_host_idle():
    r = _bench("--steps", "1", "--warmup", "1", "--full")
    assert r["ms_per_step"] > 0 and r["host_idle_ms_per_step"] > 0
    assert "outputs" not in r
