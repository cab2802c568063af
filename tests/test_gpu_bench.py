"""GPU: bench.py end to end at a toy size - a plain run times exactly --steps steps and prints the contract line
alone; --dump-outputs writes what the LAST timed step computed, the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

B, V, STEPS, ROT = 4096, 1000, 6, 3
ARGS = ["--workload", "deepfm", "--batch", str(B), "--vocab", str(V), "--steps", str(STEPS), "--warmup", "2",
        "--rotate", str(ROT), "--prewarm", "0"]


def _run(out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_contract_line_and_dumps_the_last_step(hip_lib, tmp_path):
    recs = [_run(tmp_path / d) for d in "ab"]
    for rec in recs:
        assert rec["metric"] == bench.METRIC and rec["unit"] == "examples/s" and rec["dtype"] == "f32"
        assert rec["higher_is_better"] is True and rec["steps"] == STEPS and rec["warmup"] == 2
        assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(B / (rec["ms_per_step"] * 1e-3), rel=1e-2)
        for k in ("roofline", "cpu_baseline", "parity_check", "optimizer_step", "train_step", "workloads", "zipf",
                  "pmc_passes", "step_hbm"):
            assert k not in rec, k  # measured with --full only
    a, b = tmp_path / "a", tmp_path / "b"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"loss.npy", "logit.npy", "pred.npy", "dlogit.npy", "d_rows.npy"} <= set(names)
    assert any(n.startswith("grad_dnn_layer_") for n in names)
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-7, err_msg=n)  # same arguments, same inputs
    logit, pred = np.load(a / "logit.npy"), np.load(a / "pred.npy")
    assert logit.shape == (B,) and np.load(a / "d_rows.npy").shape == (B, 26, 16)
    np.testing.assert_allclose(pred, 1.0 / (1.0 + np.exp(-logit.astype(np.float64))), rtol=1e-4, atol=1e-6)

    # the last of STEPS timed steps ran batch (STEPS - 1) % ROT of the rotation: recompute it here
    args = bench.parse(ARGS)
    w = bench.WORKLOADS["deepfm"]
    dev = torch.device("cuda", 0)
    engine, idx0, dense0, y0, _ = bench.make_engine(args, w, B, V, dev, 0, 1, False)
    k = (STEPS - 1) % ROT
    assert k != 0
    loss = engine.fwd_bwd(*bench.synth_inputs(w, B, V, dev, 2019 + 1000 * k))
    torch.cuda.synchronize()
    np.testing.assert_allclose(engine.logit.cpu().numpy(), logit, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss.cpu().numpy(), np.load(a / "loss.npy"), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(engine.d_rows.cpu().numpy(), np.load(a / "d_rows.npy"), rtol=1e-5, atol=1e-8)
    engine.fwd_bwd(idx0, dense0, y0)
    torch.cuda.synchronize()
    assert not np.allclose(engine.logit.cpu().numpy(), logit)  # batch 0 would have given other logits
