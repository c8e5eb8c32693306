"""tools/ab.py without a GPU: the leg grammar, the schedule (the same seed
shuffles the legs and draws the spacers as the four tools it replaces did) and
the report's statistics."""
import importlib.util
import json
import random
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ab():
    spec = importlib.util.spec_from_file_location("ab_tool", ROOT / "tools" / "ab.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_mapping_lines_parse(ab):
    forms = tuple(ab.DEV_FORMS)
    assert forms[0] == "global"
    assert ab.parse_legs("cur,ab/lib/x.so", forms) == [
        ("cur", "cur", {}, "global"), ("ab/lib/x.so", "ab/lib/x.so", {}, "global")]
    assert ab.parse_legs("parent-global=P,new-global=cur,new-seg=cur:seg", forms) == [
        ("parent-global", "P", {}, "global"), ("new-global", "cur", {}, "global"),
        ("new-seg", "cur", {}, "seg")]
    assert ab.parse_legs("seg-filter=cur:seg-filter,route=cur:route", forms) == [
        ("seg-filter", "cur", {}, "seg-filter"), ("route", "cur", {}, "route")]
    for line in ("--legs cur,ab/lib/x.so",
                 "--legs parent-global=P,new-global=cur,new-seg=cur:seg",
                 "--legs seg-filter=cur:seg-filter,route=cur:route"):
        assert line in ab.__doc__


def test_tuning_default_name_and_libraries(ab):
    forms = tuple(ab.DEV_FORMS)
    text = "cur@side=1;chunk_tiles=8:seg"
    assert ab.parse_legs(text, forms) == [(text, "cur", {"side": 1, "chunk_tiles": 8}, "seg")]
    assert ab.parse_legs("a=test@dbg_merge=1", forms) == [("a", "test", {"dbg_merge": 1}, "global")]
    assert ab.parse_legs("/x/lib.so:route", forms)[0][:2] == ("/x/lib.so:route", "/x/lib.so")
    assert ab.lib_path("cur") is None
    assert ab.lib_path("test") == str(ab.abi.TEST_LIB_PATH)
    assert ab.lib_path("ab/lib/x.so") == str(ROOT / "ab/lib/x.so")
    assert ab.lib_path("/x/lib.so") == "/x/lib.so"
    assert ab.parse_legs("plain=cur:plain,route=cur:route,p=ab/lib/p.so", ab.WORKER_FORMS) == [
        ("plain", "cur", {}, "plain"), ("route", "cur", {}, "route"),
        ("p", "ab/lib/p.so", {}, "plain")]


@pytest.mark.parametrize("cmd, legs", [
    ("dev", "cur:segg"),            # unknown form
    ("dev", "cur:plain"),           # the worker's form
    ("dev", "a=cur,a=test"),        # a name twice
    ("dev", "cur,cur"),             # ... by default
    ("dev", ""),                    # no leg
    ("dev", ","),
    ("dev", "cur@side=x"),
    ("worker", "cur:seg"),
    ("worker", "cur@side=1:route"),
    ("worker", ""),
])
def test_bad_legs_are_argparse_errors(ab, cmd, legs, capsys):
    with pytest.raises(SystemExit) as e:
        ab.main([cmd, "--legs", legs])
    assert e.value.code == 2
    assert "--legs" in capsys.readouterr().err


def reference_schedule(seed, nlegs, rounds):
    """What the four former tools did with their generator."""
    rng = random.Random(seed)
    got = []
    for r in range(rounds):
        order = list(range(nlegs))
        rng.shuffle(order)
        for i in order:
            got.append((i, rng.randrange(0, 64)))
    return got


@pytest.mark.parametrize("nlegs", [3, 2])
def test_schedule_is_the_former_tools(ab, nlegs, capsys):
    legs = ab.parse_legs("a=cur,b=test,c=cur:seg", tuple(ab.DEV_FORMS))[:nlegs]
    seen = []

    def run_leg(leg, rng):
        seen.append((legs.index(leg), rng.randrange(0, 64)))
        return {"step": float(len(seen)), "parse": 2.0 * len(seen)}

    res = ab.alternate(legs, 7, 1, run_leg, "imix")
    assert seen == reference_schedule(1, nlegs, 7)
    assert len({tuple(i for i, _ in seen[r * nlegs:(r + 1) * nlegs]) for r in range(7)}) > 1
    assert list(res) == [leg.name for leg in legs]
    for k, leg in enumerate(legs):
        at = [j + 1 for j, (i, _) in enumerate(seen) if i == k]
        assert res[leg.name] == {"step": [float(j) for j in at], "parse": [2.0 * j for j in at]}
    assert capsys.readouterr().out.splitlines() == [f"imix round {r} done" for r in range(1, 8)]
    # a generator passed as the seed is continued, as the former tools continued
    # theirs from one profile or burst size to the next
    rng, seen2 = random.Random(1), []
    for tag in ("udp4", "imix"):
        ab.alternate(legs, 3, rng, lambda leg, g: seen2.append(
            (legs.index(leg), g.randrange(0, 64))) or {}, tag)
    assert seen2 == reference_schedule(1, nlegs, 6)


def test_report_statistics(ab, capsys):
    base = [10.0, 12.0, 11.0, 14.0]          # median 11.5, spread 4
    assert ab.verdict([15.5, 15.5, 99.0, 1.0], base) == (4.0, 4.0, "inside")     # exactly the spread
    assert ab.verdict([7.5, 7.5, 7.5], base) == (-4.0, 4.0, "inside")
    assert ab.verdict([15.75, 15.75], base) == (4.25, 4.0, "outside")
    assert ab.verdict([7.0], base) == (-4.5, 4.0, "outside")
    res = {"plain": {"us_burst": base, "only_plain": [1.0]},
           "route": {"us_burst": [15.5, 15.5, 99.0, 1.0]},
           "far": {"us_burst": [20.0, 30.0, 40.0]}}
    ab.report(res, "plain", ("us_burst", "only_plain"), "burst   32", ("us_burst", 32, "Mpkt/s"))
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 5
    assert out[0].startswith("burst   32 plain") and \
        "us_burst us median 11.50 [10.00-14.00]" in out[0] and "2.78 Mpkt/s" in out[0]
    assert "only_plain us median 1.00 [1.00-1.00]" in out[0]
    assert "us_burst us median 15.50 [1.00-99.00]" in out[1] and "only_plain" not in out[1]
    assert "us_burst us median 30.00 [20.00-40.00]" in out[2]
    assert out[3] == ("burst   32 route - plain, us_burst: +4.00 us (plain spread over its "
                      "repeats: 4.00 us): inside that spread")
    assert out[4] == ("burst   32 far - plain, us_burst: +18.50 us (plain spread over its "
                      "repeats: 4.00 us): outside that spread")
    # the step time is in ms, four decimals
    ab.report({"a": {"step": [0.25, 0.26]}, "b": {"step": [0.2358]}}, "a", ("step",), "imix  q3")
    out = capsys.readouterr().out.splitlines()
    assert "step ms median 0.2550 [0.2500-0.2600]" in out[0]
    assert out[2].startswith("imix  q3 b - a, step: -0.0192 ms (a spread over its repeats: 0.0100 ms)")
    assert out[2].endswith("outside that spread")


def test_json_round_trips(ab, tmp_path):
    legs = ab.parse_legs("a=cur,b=cur:seg", tuple(ab.DEV_FORMS))
    res = {"imix": ab.alternate(legs, 3, 5, lambda leg, rng: {"step": rng.random(), "parse": 1.5})}
    path = tmp_path / "sub" / "ab.json"
    ab.write_json(str(path), res)
    assert json.loads(path.read_text()) == res
    assert list(res["imix"]) == ["a", "b"] and len(res["imix"]["b"]["step"]) == 3
    ab.write_json("", res)   # no --json: nothing written
