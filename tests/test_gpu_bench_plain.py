"""bench.py as the driver runs it (no --full): the timed steps and the one line, nothing behind them — no roofline, CPU baseline or
extras, no side file — and --dump-outputs, whose files must hold exactly what the last timed step computed: every MSM of it against
the closed form (sum s_i * (i+1)) * G through an independent kernel path (scalarMul), like the check --full runs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_module_plain", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    steps, per_step, logn = 3, 4, 16
    dump = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR",
                                                             "MASTER_PORT", "ZG_SHARDS", "ZG_SHARD_EXCHANGE")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                          "--logn", str(logn), "--msms-per-step", str(per_step), "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-1500:])
    last = out.stdout.rstrip("\n").splitlines()[-1]
    line = json.loads(last)
    assert line["metric"] == "BN254 G1 MSM/sec" and line["unit"] == "MSM/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 * per_step / line["ms_per_step"], rel=1e-4)  # MSMs per second of the timed steps
    assert line["config"]["workload"] == f"msm_g1_2^{logn}" and line["config"]["msms_per_step"] == per_step
    for k in ("roofline", "cpu_baseline", "also", "errors"):
        assert k not in line, k
    assert line["extra_file"] is None and line["config"]["bit_exact_check"] is None
    assert sorted(os.listdir(tmp_path)) == ["outputs"], "a plain run writes no side file"

    xy, inf = np.load(dump / "msm_xy_u32.npy"), np.load(dump / "msm_infinity.npy")
    assert sorted(os.listdir(dump)) == ["msm_infinity.npy", "msm_xy_u32.npy"]
    assert xy.dtype == np.float64 and xy.shape == (per_step, 16) and inf.dtype == np.float64 and inf.shape == (per_step,)
    limbs = xy[:, 0::2].astype(np.uint64) | (xy[:, 1::2].astype(np.uint64) << np.uint64(32))

    bench = _bench_module()
    from zolt_amd import api, lib
    lib.init(0)
    g, n = api.generator(), 1 << logn
    want = [api.MSM.scalarMul(g, api.fr_from_int(bench.closed_form_scalar(bench.raw_scalars(bench.SEED + s, 0, n), 0)))
            for s in range(bench.N_SCALAR_SETS)]
    for b in range(per_step):
        wxy, winf = want[((steps - 1) * per_step + b) % bench.N_SCALAR_SETS]
        assert int(inf[b]) == winf and np.array_equal(limbs[b], wxy), f"dumped MSM {b} of the last step"
