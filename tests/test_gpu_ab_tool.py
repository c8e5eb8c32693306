"""tools/ab.py on the GPU: every form and leg kind runs clean and is reported.
No time is compared.  n = 70001 is past the 4096-packet one-launch path, so
the grid launches (parse, line scatter and, where it is not fused into the
scatter, scan) and their events are the ones read."""
import importlib.util
import json
import math
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ab():
    spec = importlib.util.spec_from_file_location("ab_tool", ROOT / "tools" / "ab.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_samples(res, want, rounds, maybe=()):
    """Every leg reports the metrics of want (and at most those of maybe
    besides), each with one finite, positive sample a round."""
    assert sorted(res) == sorted(want)
    for name, v in res.items():
        assert set(want[name]) <= set(v) <= set(want[name]) | set(maybe), (name, sorted(v))
        for metric, x in v.items():
            assert len(x) == rounds, (name, metric, x)
            assert all(math.isfinite(t) and t > 0 for t in x), (name, metric, x)


def test_dev_every_form_and_two_libraries(ab, tmp_path, monkeypatch):
    libs, real = [], ab.SoftRss

    def spy(*a, **kw):
        e = real(*a, **kw)
        libs.append(e._lib._name)
        return e

    monkeypatch.setattr(ab, "SoftRss", spy)
    out = tmp_path / "dev.json"
    assert ab.main(["dev", "--legs", "a=cur,b=test,c=cur:seg,d=cur:seg-filter,e=cur:route",
                    "--pkts", "70001", "--batches", "2", "--rounds", "2", "--steps", "2",
                    "--nb-procs", "3", "--profiles", "imix", "--json", str(out)]) == 0
    got = json.loads(out.read_text())
    assert list(got) == ["imix"]
    # the global form launches the scan kernel only where the line scatter does not
    # scan in its prologue (it does at 3 buckets): a kernel that never ran has no
    # sample, so "scan" may be absent, and where it is present it is positive
    full, parse = ["parse", "scatter", "step"], ["parse", "step"]
    check_samples(got["imix"], {"a": full, "b": full, "c": parse, "d": parse, "e": parse}, 2,
                  maybe=["scan"])
    # two libraries lived in one process: ten contexts, two of them on libyrss_test.so
    assert len(libs) == 10 and len(set(libs)) == 2
    assert sorted(Path(x).name for x in set(libs)) == ["libyrss.so", "libyrss_test.so"]
    assert sum(Path(x).name == "libyrss_test.so" for x in libs) == 2


def test_worker_plain_and_route(ab, tmp_path):
    out = tmp_path / "worker.json"
    assert ab.main(["worker", "--rounds", "2", "--bursts", "100", "--sizes", "32",
                    "--nslots", "8", "--nblocks", "2", "--json", str(out)]) == 0
    got = json.loads(out.read_text())
    assert list(got) == ["32"]
    check_samples(got["32"], {"plain": ["us_burst"], "route": ["us_burst"]}, 2)
