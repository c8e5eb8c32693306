"""fs/lib config ingestion on CPU.

* The INI reader (yastack_amd/ffconfig.ini_parse) against the reference's own
  parser, fs/lib/ff_ini_parser.c: the five shipped fs/config/*.ini files
  (settings only, kept byte for byte in golden/ff_config) and 400 generated files
  with the syntax edge cases inih handles (inline ';' comments, continuation
  lines, ':' pairs, a BOM, lines past INI_MAX_LINE, broken sections), event for
  event and error line: against its recorded answers (golden/ref_ini_events.json)
  and, where oracle/_ref is built, the parser compiled where it lies as well.
* The knobs the soft-RSS path reads from those five files, against values
  derived by hand from fs/lib/ff_config.c:73-136 (nb_procs = bits of
  lcore_mask), :440-451 (soft_dispatch, dispatch_only_core), :355-367 and
  ff_dpdk_if.c:420 (a port's nb_queues = its lcore_list length).
* [kni] keys (ff_config.c:442-449) and ff_check_config's rules (:538-604).
"""
import json
from pathlib import Path

import numpy as np
import pytest

from yastack_amd import ffconfig as F

GOLDEN = Path(__file__).resolve().parent / "golden"
REF_CFG = GOLDEN / "ff_config"

# hand-derived: lcore_mask -> nb_procs; [port0] lcore_list -> nb_queues
EXPECT = {
    "config.ini": dict(nb_procs=3, soft=1, only=1, nbq={0: 3}, lcores={0: [0, 1, 2]}),
    "config_1_core.ini": dict(nb_procs=1, soft=1, only=0, nbq={0: 1}, lcores={0: [0]}),
    "config_1_core_ena5.ini": dict(nb_procs=1, soft=1, only=0, nbq={0: 1}, lcores={0: [0]}),
    "config_2_core_ena5.ini": dict(nb_procs=2, soft=1, only=0, nbq={0: 2}, lcores={0: [0, 1]}),
    "config_3_core_ena5.ini": dict(nb_procs=3, soft=1, only=0, nbq={0: 3},
                                   lcores={0: [0, 1, 2]}),
}


def _recorded(rec):
    """(events, error) as ref_ini_events gives them, from ref_ini_events.json."""
    return [tuple(e) for e in rec["events"]], rec["error"]


@pytest.fixture(scope="module")
def ref_recorded():
    return json.loads((GOLDEN / "ref_ini_events.json").read_text())


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_reference_configs(name, oracle_mod, ref_recorded):
    path = REF_CFG / name
    ours = F.ini_events(path.read_bytes())
    assert ours == _recorded(ref_recorded["configs"][name])
    ref = oracle_mod.ref_ini_events(path)
    if ref is not None:
        assert ours == ref
    fc = F.load_ff_config(str(path))
    e = EXPECT[name]
    assert (fc.nb_procs, fc.soft_dispatch, fc.dispatch_only_core) == \
        (e["nb_procs"], e["soft"], e["only"])
    assert fc.nb_queues == e["nbq"] and fc.lcore_list == e["lcores"]
    assert fc.kni_enable == 0          # the shipped [kni] sections are commented out


def _random_ini(rng) -> bytes:
    names = ["lcore_mask", "port_list", "soft_dispatch", "enable", "method", "tcp_port", "a",
             "kern.ipc.maxsockets", "Name With Space", "x"]
    vals = ["7", "0,1", "1", "accept", "80,443 ; web", "80;443", "  spaced  ", "", "a:b",
            "v ;c", "=eq", "0x1f", "long" * 60]
    out = []
    if rng.random() < 0.2:
        out.append(b"\xef\xbb\xbf")
    for _ in range(int(rng.integers(3, 25))):
        k = rng.random()
        if k < 0.12:
            out.append(f"[{rng.choice(['dpdk', 'kni', 'port0', 'freebsd.boot', 's' * 70])}]")
        elif k < 0.16:
            out.append("[broken")
        elif k < 0.2:
            out.append(f"[sec] ; c")
        elif k < 0.28:
            out.append(rng.choice(["; comment", "# comment", "   ; indented comment", ""]))
        elif k < 0.36:
            out.append("   continued " + str(rng.choice(vals)))
        elif k < 0.4:
            out.append("no separator here")
        elif k < 0.44:
            out.append("x" * int(rng.integers(190, 420)) + "=tail")
        else:
            sep = rng.choice(["=", ":", " = ", "\t=\t"])
            out.append(f"{rng.choice(names)}{sep}{rng.choice(vals)}")
    eol = rng.choice(["\n", "\r\n"])
    text = eol.join(x if isinstance(x, str) else "" for x in out)
    head = out[0] if isinstance(out[0], bytes) else b""
    return head + text.encode("latin-1") + (eol.encode() if rng.random() < 0.7 else b"")


def generated_inis():
    """The files of test_reader_vs_reference_generated, in the order
    golden/ref_ini_events.json holds the reference's answers (make_golden.py ref)."""
    rng = np.random.default_rng(642)
    return [_random_ini(rng) for _ in range(400)]


def test_reader_vs_reference_generated(tmp_path, oracle_mod, ref_recorded):
    live = oracle_mod.ref_ini_events(Path(__file__)) is not None
    files, want = generated_inis(), ref_recorded["generated"]
    assert len(files) == len(want) == 400
    for i, (data, rec) in enumerate(zip(files, want)):
        assert F.ini_events(data) == _recorded(rec), data[:200]
        if live:
            p = tmp_path / f"g{i}.ini"
            p.write_bytes(data)
            assert oracle_mod.ref_ini_events(p) == _recorded(rec), data[:200]


def test_list_and_mask_rules():
    # __parse_config_list over rte_strsplit (ff_config.c:246-308)
    assert F.parse_list("1-3,0,7") == [0, 1, 2, 3, 7]
    assert F.parse_list("1,,2") == [0, 1, 2]          # an empty field is strtol("") = 0
    assert F.parse_list("1,2,") == [1, 2]             # a trailing ',' opens no token
    assert F.parse_list("-5") == [0, 1, 2, 3, 4, 5]   # lbound "" = 0
    assert F.parse_list(" 3 - 5 , 1") == [1, 3, 4, 5]
    assert F.parse_list("5-3,1") == [1]               # empty range adds nothing
    for bad in ("1a", "1-2-3", "a-2", "x", "1,\t2\t"):
        with pytest.raises(ValueError):
            F.parse_list(bad)
    assert len(F.parse_list("0-128", 128)) == 129     # the reference admits max + 1
    with pytest.raises(ValueError):
        F.parse_list("0-129", 128)
    # parse_lcore_mask (:73-136)
    assert F.parse_lcore_mask("f0") == [4, 5, 6, 7]
    assert F.parse_lcore_mask(" 0X1 ") == [0]
    assert F.parse_lcore_mask("0" * 40 + "3") == [0, 1]
    for bad in ("xyz", "", "0x", "1" + "0" * 32, "0"):
        with pytest.raises(ValueError):
            F.parse_lcore_mask(bad)
    with pytest.raises(ValueError):                   # proc_id >= count
        F.parse_lcore_mask("3", proc_id=2)
    assert F.c_atoi("  12ab") == 12 and F.c_atoi("-3") == -3 and F.c_atoi("x") == 0


PORT = """[port0]
addr=192.168.1.2
netmask=255.255.255.0
broadcast=192.168.1.255
gateway=192.168.1.1
"""


def _write(tmp_path, text, name="c.ini"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_kni_keys(tmp_path):
    text = ("[dpdk]\nlcore_mask=7\nsoft_dispatch=1\nport_list=0\n[kni]\nenable=1\n"
            "method=Accept ; inline comment\ntcp_port=80,443\nudp_port=53\n" + PORT)
    fc = F.load_ff_config(_write(tmp_path, text))
    assert fc.kni_enable == 1 and fc.kni_method == "Accept" and fc.kni_accept
    assert fc.kni_tcp_port == "80,443" and fc.kni_udp_port == "53"
    assert fc.nb_queues == {0: 3}                      # no lcore_list: all nb_procs lcores


def test_check_config_rules(tmp_path):
    base = "[dpdk]\nlcore_mask=3\nport_list=0\n"
    with pytest.raises(ValueError, match="method is necessary"):
        F.load_ff_config(_write(tmp_path, base + "[kni]\nenable=1\n" + PORT))
    with pytest.raises(ValueError, match="kni.method"):
        F.load_ff_config(_write(tmp_path, base + "[kni]\nmethod=drop\n" + PORT))
    with pytest.raises(ValueError, match="no gateway"):
        F.load_ff_config(_write(tmp_path, base + PORT.replace("gateway=192.168.1.1\n", "")))
    with pytest.raises(ValueError, match="not enabled"):
        F.load_ff_config(_write(tmp_path, base + PORT + "lcore_list=0-2\n"))
    with pytest.raises(ValueError, match="primary lcore"):
        F.load_ff_config(_write(tmp_path, base + "[kni]\nenable=1\nmethod=reject\n" + PORT +
                                "lcore_list=1\n"))
    with pytest.raises(ValueError, match="line 4"):   # a port key before port_list
        F.load_ff_config(_write(tmp_path, "[dpdk]\nlcore_mask=3\n[port0]\naddr=1\n"))
    with pytest.raises(ValueError, match="line 2"):   # bad mask stops the parse there
        F.load_ff_config(_write(tmp_path, "[dpdk]\nlcore_mask=zz\nport_list=0\n" + PORT))
    fc = F.load_ff_config(_write(tmp_path, base + PORT + "lcore_list=1\n"))
    assert fc.nb_queues == {0: 1} and fc.lcore_list == {0: [1]}
