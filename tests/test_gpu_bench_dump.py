"""bench.py --dump-outputs and the plain / --full split, on the GPU.

One small plain run (two rotated batches, three timed steps): the line carries
the steps asked for and ms_per_step and none of the --full legs, and the dumped
arrays are what the oracle computes for the batch the last timed step
classified.  The sampling of outputs longer than DUMP_SAMPLE is checked on
dump_outputs itself.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_dumps_last_step(tmp_path, oracle_mod):
    n, steps, warmup, nbat = 5001, 3, 2, 2
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", str(warmup), "--pkts", str(n), "--batches",
                        str(nbat), "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Mpkt/s"
    # ms_per_step is the timed steps' own time: printed to 1e-4 ms, and a step
    # of this size takes microseconds, so the two agree to a few percent
    assert d["value"] == pytest.approx(n / d["ms_per_step"] / 1e3, rel=5e-2)
    for leg in ("configs_extra", "cpu_baseline", "pcie_inclusive", "pcie_fanout", "check"):
        assert d[leg] is None, leg
    assert d["roofline"]["probe"] is None
    # the batch of the last timed step, from the generator's host twin
    k = (warmup + steps - 1) % nbat
    win, lens = oracle_mod.synth(bench.PROFILES["udp4"], n, k * n, bench.SEED,
                                 bench.NFLOWS["udp4"], 64)
    q_ref, h_ref = oracle_mod.dispatch_windows(win, 64, lens, oracle_mod.cfg(3, 3, 1, 1))
    qi_ref, qs_ref = oracle_mod.process_burst(q_ref, 3)
    got = {p.stem: np.load(p) for p in (tmp_path / "dump").glob("*.npy")}
    assert sorted(got) == ["hash", "q", "qidx", "qstart"]
    assert got["q"].dtype == np.float32 and got["hash"].dtype == np.float64
    assert np.array_equal(got["q"], q_ref.astype(np.float32))
    assert np.array_equal(got["hash"], h_ref.astype(np.float64))
    assert np.array_equal(got["qidx"], qi_ref.astype(np.float64))
    assert np.array_equal(got["qstart"], qs_ref.astype(np.float64))


def test_dump_samples_long_outputs(tmp_path):
    from yastack_amd.dispatch import DispatchResult

    n = bench.DUMP_SAMPLE + 4097
    dev = torch.device("cuda", 0)
    q = (torch.arange(n, device=dev) % 7 - 2).to(torch.int16)
    h = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % (1 << 32))
    h32 = torch.where(h >= (1 << 31), h - (1 << 32), h).to(torch.int32)
    qi = torch.arange(n - 1, -1, -1, device=dev, dtype=torch.int32)
    qs = torch.tensor([0, 5, 9, n, n], dtype=torch.int32, device=dev)
    out = DispatchResult(q, h32, qi, qs)
    for sub in ("a", "b"):
        bench.dump_outputs(tmp_path / sub, out, n, 0)
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    b = {p.stem: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert sorted(a) == ["hash", "q", "qidx", "qstart"]
    assert all(np.array_equal(a[k], b[k]) for k in a)          # the same sample every time
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    pos = n - 1 - a["qidx"].astype(np.int64)                    # qidx[i] = n - 1 - i
    assert pos.size == bench.DUMP_SAMPLE and np.all(np.diff(pos) >= 0)
    assert pos.min() < n // 64 and pos.max() > n - n // 64      # spread over the whole output
    assert np.array_equal(a["q"], (pos % 7 - 2).astype(np.float32))
    assert np.array_equal(a["hash"], (pos * 2654435761 % (1 << 32)).astype(np.float64))
    assert np.array_equal(a["qstart"], np.array([0, 5, 9, n, n], np.float64))
    # two ranks share the bound: half the positions each, rank 1 under its own names
    bench.dump_outputs(tmp_path / "c", out, n, 1, world=2)
    c = {p.name: np.load(p) for p in (tmp_path / "c").glob("*.npy")}
    assert sorted(c) == ["hash.rank1.npy", "q.rank1.npy", "qidx.rank1.npy", "qstart.rank1.npy"]
    assert c["q.rank1.npy"].size == c["qidx.rank1.npy"].size == bench.DUMP_SAMPLE // 2
    pos = n - 1 - c["qidx.rank1.npy"].astype(np.int64)
    assert np.array_equal(c["q.rank1.npy"], (pos % 7 - 2).astype(np.float32))
