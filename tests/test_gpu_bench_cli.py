"""GPU: bench.py's command line.  A plain run (no --full) times --steps steps,
prints the headline line without the legs of --full, and --dump-outputs writes the
last timed step's outputs and the reduced statistics as float64 .npy files whose
sampled chains / steps -- proper subsets here, gathered on the device -- are the ones
the index files name (one small child run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_headline_and_dumped_outputs(tmp_path):
    # 16384 chains x 16 steps at d = 128: the dump samples 8192 of the chains (2048 of
    # them for v) and 8 of the steps, so every gather on the device is a proper subset
    nc, T, steps, warmup, d = 16384, 16, 3, 1, 128
    env = {k: v for k, v in os.environ.items() if k not in ("MASTER_ADDR", "RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--config", "C2_qary128", "--chains", str(nc),
                        "--imhk-steps", str(T), "--no-dist", "--dump-outputs", str(tmp_path / "o")],
                       env=env, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == steps and out["warmup"] == warmup and out["full"] is False
    assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    # value = proposals / elapsed and ms_per_step = elapsed / steps are one measurement
    assert out["ms_per_step"] > 0
    assert out["value"] * out["ms_per_step"] / 1e3 == pytest.approx(nc * T, rel=1e-3)
    assert not {"cpu_baseline", "wang_ling", "roofline", "parity_check"} & set(out)

    a = {f[:-4]: np.load(tmp_path / "o" / f) for f in os.listdir(tmp_path / "o")}
    assert all(x.dtype == np.float64 for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    ch, vch, st = (a[k].astype(int) for k in ("sample_chains", "sample_chains_v", "sample_steps"))
    assert a["z_state"].shape == (len(ch), d) and a["v_last_step"].shape == (len(vch), len(st), d)
    assert (len(ch), len(vch), len(st)) == (8192, 2048, 8) and st[-1] == T - 1
    assert np.array_equal(ch[:len(vch)], vch) and len(set(ch)) == len(ch) and len(set(st)) == len(st)
    assert 0 <= ch.min() and ch.max() < nc and np.all(np.diff(ch) > 0) and np.all(np.diff(st) > 0)
    # reference-mode weights: every proposal accepted
    assert out["imhk_acceptance"] == 1.0 and a["accepts"].tolist() == [steps * nc * T]
    assert np.array_equal(a["accepts_per_chain"], np.full(len(ch), steps * T))
    assert a["log_weight"].shape == (len(ch),) and np.isfinite(a["log_weight"]).all()
    # the sampled lattice points belong to the chains and steps named: their norms are
    # the library's ||v||^2 series, and the last kept state is the chain's final state
    v = a["v_last_step"]
    # (the two series cover the leading 1024 chains, at the sampled steps)
    lead = vch < 1024
    assert lead.sum() > 16 and a["zk_last_step"].shape == a["vnorm2_last_step"].shape == (1024, len(st))
    assert np.array_equal((v * v).sum(-1)[lead], a["vnorm2_last_step"][vch[lead]])
    assert np.array_equal(a["zk_last_step"][vch[lead], -1], a["z_state"][:len(vch)][lead, d - 1])
    assert a["gram_sum_zzT"].shape == (d, d) and a["gram_states"].tolist() == [steps * nc]
