"""The extended mode's entry points for the persistent worker, the helper
process and the fan-out (yrss_worker_start_flags, yrss_remote_set_extended,
yrss_fanout_set_extended): declared, bound, exported, and their argument
checks.  No GPU: the helper runs in its fake mode (YRSS_HELPER_INJECT=1, as
in test_remote.py), which comes up and never completes a burst."""
import errno
import re
import subprocess

import pytest

from yastack_amd import abi, remote
from yastack_amd.remote import RemoteRss

# the helper client's extended call has a header of its own: yrss_remote.h
# stays the six calls that compute the reference's results (test_abi.py)
REMOTE_HEADER = abi.REPO_DIR / "include" / "yrss_remote_ext.h"


def _flat(path):
    text = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_three_functions():
    h = _flat(abi.HEADER_PATH)
    assert ("int yrss_worker_start_flags(yrss_ctx *ctx, uint32_t nslots, uint32_t nblocks, "
            "uint32_t flags, uint16_t queue_id);") in h
    assert "int yrss_fanout_set_extended(yrss_fanout *f, uint32_t flags);" in h
    assert "int yrss_remote_set_extended(yrss_remote *r, uint32_t flags);" in _flat(REMOTE_HEADER)
    consts = dict(re.findall(r"#define (YRSS_WORKER_F_\w+)\s+(0x[0-9a-f]+)u", h))
    assert consts == {"YRSS_WORKER_F_ROUTE": "0x1", "YRSS_WORKER_F_EXTENDED": "0x2"}
    assert (abi.WORKER_F_ROUTE, abi.WORKER_F_EXTENDED) == (1, 2)


def test_no_new_ext_constant():
    names = re.findall(r"#define (YRSS_EXT_\w+)", abi.HEADER_PATH.read_text())
    assert names == ["YRSS_EXT_VLAN", "YRSS_EXT_IPV6", "YRSS_EXT_UDP", "YRSS_EXT_ALL"]
    assert not re.findall(r"#define (YRSS_EXT_\w+)", REMOTE_HEADER.read_text())


def test_bound_and_exported():
    lib, rlib = abi.load(), remote.load()
    own = {"yrss_worker_start_flags": (abi.header_functions(), lib, abi.LIB_PATH),
           "yrss_fanout_set_extended": (abi.header_functions(), lib, abi.LIB_PATH),
           "yrss_remote_set_extended": (abi.header_functions(REMOTE_HEADER), rlib,
                                        remote.LIB_PATH)}
    for name, (declared, handle, path) in own.items():
        assert name in declared, name
        assert getattr(handle, name).argtypes, name
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        assert re.search(rf"\bT {name}\b", out), (name, path)


def test_null_handles_and_unknown_bits_are_einval():
    """Checked before any GPU call: this machine has no GPU to call."""
    lib, rlib = abi.load(), remote.load()
    for flags in (0, abi.WORKER_F_EXTENDED, abi.WORKER_F_ROUTE | abi.WORKER_F_EXTENDED, 4,
                  0xFFFFFFFF):
        assert lib.yrss_worker_start_flags(None, 4, 2, flags, 0) == -errno.EINVAL
    for flags in (0, abi.EXT_UDP, abi.EXT_ALL, 8, 0xFFFFFFFF):
        assert lib.yrss_fanout_set_extended(None, flags) == -errno.EINVAL
        assert rlib.yrss_remote_set_extended(None, flags) == -errno.EINVAL


def _cfg(nq=3):
    c = abi.default_config()
    c.nb_procs = nq
    c.nb_queues = nq
    return c


def _frames(n):
    from frames import ipv4_frame
    return [ipv4_frame("10.0.0.1", 1000 + i, "10.0.0.2", 80) for i in range(n)]


@pytest.fixture
def inject(monkeypatch):
    monkeypatch.setenv("YRSS_HELPER_INJECT", "1")


def test_remote_set_extended_replaces_the_helper(inject):
    with RemoteRss(_cfg(), nslots=4, max_burst=32, nblocks=1, timeout_ms=2000) as r:
        pid = r.pid
        assert pid > 0
        assert r._lib.yrss_remote_set_extended(r._r, 8) == -errno.EINVAL
        assert r._lib.yrss_remote_set_extended(r._r, 0xFFFFFFFF) == -errno.EINVAL
        assert r.pid == pid                   # a refused call replaces nothing
        r.set_extended(udp=True)
        assert r.ext_flags == abi.EXT_UDP
        pid2 = r.pid
        assert pid2 > 0 and pid2 != pid
        r.restart()                           # (the flags stay in the ring: GPU test)
        assert r.pid not in (pid, pid2)
        r.set_extended()
        assert r.ext_flags == 0


def test_remote_set_extended_is_ebusy_while_a_ticket_is_unpolled(inject):
    with RemoteRss(_cfg(), nslots=4, max_burst=32, nblocks=1, timeout_ms=300) as r:
        pid = r.pid
        t = r.submit(_frames(8))
        assert r._lib.yrss_remote_set_extended(r._r, abi.EXT_UDP) == -errno.EBUSY
        with pytest.raises(abi.YrssError) as e:
            r.set_extended(vlan=True, ipv6=True)
        assert e.value.errno == errno.EBUSY
        assert r.pid == pid
        assert r.poll(t, wait=False)[0] == -errno.EAGAIN    # the fake helper never completes
