"""MI355X: bench.py's captured multi-step replay -- G training steps per hipGraph launch, each
with its own batch gather and update -- follows exactly the trajectory of one step per replay
(bit-identical final loss), across an epoch boundary too."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, diag=False):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mlp-dims", "1024,512,512",
           "--dataset", "640", "--batch", "32", "--device-warmup-ms", "0", *args]
    if diag:
        cmd.append("--full")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])


@pytest.fixture(scope="module")
def graph_runs(tmp_path_factory):
    """Plain runs with one and four steps per replay: {G: (record, {file name: dumped array})}.
    20 steps per epoch: warm-up 3 + 30 timed steps cross an epoch boundary mid-group."""
    import numpy as np

    runs = {}
    for g in (1, 4):
        d = tmp_path_factory.mktemp(f"dump_g{g}")
        rec = _bench("--steps", "30", "--warmup", "3", "--graph-steps", str(g),
                     "--dump-outputs", str(d))
        runs[g] = (rec, {f.name: np.load(f) for f in sorted(d.glob("*.npy"))})
    return runs


def test_graph_steps_trajectory_is_bit_identical(graph_runs):
    recs = {g: graph_runs[g][0] for g in (1, 4)}
    assert recs[1]["config"]["graph_steps"] == 1 and recs[4]["config"]["graph_steps"] == 4
    assert recs[1]["config"]["final_loss"] == recs[4]["config"]["final_loss"], recs


def test_rehearsal_diagnostic_replays_the_timed_form():
    """The one-GPU rehearsal of the W > 1 schedule (diagnostics) is captured and timed in the
    measured step's replay form -- G training steps per graph launch -- so rehearsal_over_dp1
    compares schedules, not graph-launch counts."""
    rec = _bench("--steps", "12", "--warmup", "2", diag=True)
    d = rec["diagnostics"]
    assert d["mode"] == "graph"
    assert d["rehearsal_graph_steps"] == rec["config"]["graph_steps"] == 4, d
    assert d["rehearsal_ms"] > 0 and d["rehearsal_schedule_ms"] > 0, d
    assert d["rehearsal_buckets"] >= 1, d


def test_dump_outputs_of_the_last_timed_step(graph_runs):
    """--dump-outputs: the last timed step's loss and the parameters it left, float32 and whole
    at this size; the two replay forms run the same trajectory from the same inputs, so their
    dumps are equal bit for bit. A plain run (no --full) carries no diagnostics."""
    import numpy as np

    (rec1, d1), (rec4, d4) = graph_runs[1], graph_runs[4]
    for rec, d in ((rec1, d1), (rec4, d4)):
        assert rec["steps"] == 30 and rec["ms_per_step"] > 0 and "diagnostics" not in rec
        assert float(d["loss.npy"]) == pytest.approx(rec["config"]["final_loss"], abs=1e-5)
    assert set(d1) == {"loss.npy"} | {f"module.fc{k}.{w}.npy" for k in (1, 2, 3)
                                      for w in ("weight", "bias")}
    assert d1["module.fc1.weight.npy"].shape == (512, 1024)
    for name, arr in d1.items():
        assert arr.dtype == np.float32 and np.isfinite(arr).all(), name
        assert np.array_equal(arr, d4[name]), name
