# SPDX-License-Identifier: BSD-3-Clause
"""bench.py's plain run and --dump-outputs on the GPU: the result line holds
the headline leg alone, and the arrays written are what the timed path left
for the sampled packets, bit for bit the oracle's answer on the same seeded
stream (so two builds can be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_its_outputs(tmp_path):
    import bench
    import oracle
    from grout_amd import abi
    from grout_amd import synth as S
    from grout_amd import topology as T

    # more than one read-back chunk (2^20 packets), the last one partial, and
    # more packets than the sample holds
    n = (1 << 21) - 5
    assert n > bench.DUMP_SAMPLE
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "single64",
           "--batch", str(n), "--candidates", "1", "--settle-ms", "5", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "Mpps" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["roofline"]["kernel_launches_timed"] >= 1
    assert abs(d["value"] - n / (d["ms_per_step"] / 1e3) / 1e6) <= 0.01 * d["value"]
    # the legs beside the headline figure belong to --full
    for leg in ("plain_placement", "value_plain_placement", "contiguous_unplaced", "prefix32", "host_path",
                "cpu_baseline"):
        assert leg not in d, leg

    assert sorted(os.listdir(out)) == ["out_lines.npy", "sample_index.npy", "verdicts.npy"]
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    k = bench.DUMP_SAMPLE
    assert got["out_lines"].dtype == np.float32 and got["out_lines"].shape == (k, abi.LINE)
    assert got["verdicts"].dtype == np.float64 and got["verdicts"].shape == (k, len(abi.VERDICT_DT.names))
    assert got["sample_index"].dtype == np.float64 and got["sample_index"].shape == (k,)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    idx = got["sample_index"].astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
    assert idx[0] < 1 << 20 <= idx[-1]  # both chunks sampled

    # the same stream (rank 0's seed), through the oracle
    frames, meta = S.stream(n, S.SEED_GPU_BASE, dst_range=(T.ip4("16.1.0.0"), T.ip4("16.1.255.255")))
    o = oracle.Oracle(T.config_single_route())
    o_lines, o_v, _ = o.process(frames, meta)
    o.close()
    assert np.array_equal(got["out_lines"], o_lines[idx].astype(np.float32))
    for j, f in enumerate(abi.VERDICT_DT.names):
        assert np.array_equal(got["verdicts"][:, j], o_v[f][idx].astype(np.float64)), f
    assert (got["verdicts"][:, 0] == abi.EDGE["port_output"]).all()
