#!/usr/bin/env python3
"""Generate the committed golden fixtures under tests/golden/.

Run here (where /root/reference and oracle/_ref exist):
    python tests/golden/make_golden.py

Produces:
  survey_kat.json     the dispatch known answers SURVEY.md §8(a) recorded by
                      running the reference toeplitz_dispatch (built from
                      fs/lib/ff_dpdk_if.c) in the survey container, with the
                      frames rebuilt by tests/frames.py.
  thash_82599.json    Intel 82599 RSS verification suite as held by the
                      reference's own test, dpdk/test/test/test_thash.c:60-104
                      (key default_rss_key :98-104), L3+L4 hashes.
  synth_<name>.npz    first 1024 packets of every synthetic profile (80-byte
                      windows + data_len) and the expected {q, hash} for two
                      configs.  For every hashed packet the hash is computed
                      by the REFERENCE's own toeplitz_hash (oracle/_ref,
                      compiled from ff_dpdk_if.c:1881-1902) on the tuple
                      extracted per ff_dpdk_if.c:1994-2021, and the script
                      asserts the oracle restatement agrees.
  ref_*.npz, ref_ini_events.json
                      (`make_golden.py ref`, only these) what the reference's
                      compiled code answers on the tests' seeded inputs, see
                      ref_recorded().
No reference source is copied: the fixtures are data (inputs and outputs).
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE.parent))

from frames import ipv4_frame, ethertype_frame  # noqa: E402
from oracle import oracle  # noqa: E402

SEED = 0x9E3779B97F4A7C15
NFIX = 1024
STRIDE = 80
PROFILES = {0: "udp4_1flow", 1: "udp4", 2: "imix", 3: "vlan6_tcp", 4: "jumbo_tcp4", 5: "tcp4",
            6: "fuzz"}
NFLOWS = {0: 1, 1: 1 << 20, 2: 1 << 20, 3: 1 << 22, 4: 1 << 24, 5: 1 << 20, 6: 1}
CONFIGS = {"np8": (8, 8, 1, 0), "ini": (3, 3, 1, 1)}  # nb_procs, nb_queues, soft, only


def survey_kat():
    # frame (64 B, IHL=5, TCP) -> hash, q(8), q(3), q(3, doc=1)
    main = [
        ("10.0.0.1", 12345, "10.0.0.2", 80, 0x0AD63BA6, 6, 2, 1),
        ("66.9.149.187", 2794, "161.142.100.80", 1766, 0x238A8D41, 1, 1, 2),
        ("192.168.1.100", 40000, "172.31.27.43", 10000, 0x89C5F1CB, 3, 1, 2),
        ("1.2.3.4", 1, "5.6.7.8", 65535, 0x93047E89, 1, 0, 2),
    ]
    cases = []
    for s, sp, d, dp, h, q8, q3, q3d in main:
        f = ipv4_frame(s, sp, d, dp)
        cases.append({"name": f"{s}:{sp}->{d}:{dp}", "frame": f.hex(), "len": 64,
                      "expect": {"hash": h, "np8": q8, "np3": q3, "np3_doc": q3d}})
    base = ("10.0.0.1", 12345, "10.0.0.2", 80)
    # edge cases, all at nb_procs=8 (SURVEY.md §8(a) "Edge cases")
    edges = [
        ("ihl0_len64", ipv4_frame(*base, ihl=0, total_len=0), 64, 6),
        ("len13", ipv4_frame(*base), 13, 2),
        ("len33", ipv4_frame(*base), 33, 2),
        ("len34_ihl5", ipv4_frame(*base), 34, 2),
        ("ihl15_len64", ipv4_frame(*base, ihl=15), 64, 2),
        ("arp", ethertype_frame(0x0806), 64, 0),
        ("rarp", ethertype_frame(0x8035), 64, 0),
        ("ipv6", ethertype_frame(0x86DD), 64, 2),
        ("vlan", ethertype_frame(0x8100), 64, 2),
        ("version6_ihl5_tcp", ipv4_frame(*base, version=6), 64, 6),
    ]
    for name, f, L, q8 in edges:
        cases.append({"name": name, "frame": f.hex(), "len": L, "expect": {"np8": q8}})
    # IHL=15, len 80 -> hashed, hash 0xc65b1882.  The survey did
    # not record bytes 74..77 (the L4 ports at 14 + 4*15).  The hash is GF(2)-
    # linear in the tuple bits, so with the edge cases' addresses (10.0.0.1 ->
    # 10.0.0.2) the port bits follow from one linear solve (rank 31 of 32); its
    # natural solution, sport 1 -> dport 2 (bytes 00 01 00 02), reproduces the
    # recorded hash through the reference's own toeplitz_hash (asserted below).
    f15 = ipv4_frame("10.0.0.1", 1, "10.0.0.2", 2, ihl=15, length=80)
    R = oracle.ref()
    if R is not None:
        t = tuple_of(np.frombuffer(f15, np.uint8))
        assert R.ref_toeplitz_hash(40, oracle.MLX_KEY, 12, t) == 0xC65B1882
    cases.append({"name": "ihl15_len80", "frame": f15.hex(), "len": 80,
                  "expect": {"hash": 0xC65B1882, "np8": 0xC65B1882 % 8}})
    return {
        "source": "SURVEY.md §8(a) known answers: reference toeplitz_dispatch "
                  "(fs/lib/ff_dpdk_if.c:1945-2113) run in the survey container, key "
                  "default_rsskey_40bytes (:113-119). Frames rebuilt by tests/frames.py.",
        "reconstructed": "IHL=15 len=80 hash 0xc65b1882: bytes 74..77 (not recorded by the "
                         "survey) solved from the hash's GF(2)-linearity; ports 1 -> 2 "
                         "reproduce it through the reference toeplitz_hash.",
        "configs": {"np8": [8, 8, 1, 0], "np3": [3, 3, 0, 0], "np3_doc": [3, 3, 1, 1]},
        "cases": cases,
    }


def thash_82599():
    # dpdk/test/test/test_thash.c:60-71 (v4_tbl) — dst, src, dport, sport, l3, l3l4
    v4 = [
        ("161.142.100.80", "66.9.149.187", 1766, 2794, 0x323E8FC2, 0x51CCC178),
        ("65.69.140.83", "199.92.111.2", 4739, 14230, 0xD718262A, 0xC626B0EA),
        ("12.22.207.184", "24.19.198.95", 38024, 12898, 0xD2D0A5DE, 0x5C2B394A),
        ("209.142.163.6", "38.27.205.30", 2217, 48228, 0x82989176, 0xAFC7327F),
        ("202.188.127.2", "153.39.163.191", 1303, 44251, 0x5D1809C5, 0x10E828A2),
    ]
    # :73-96 (v6_tbl)
    v6 = [
        ("3ffe25010200000300000000000000" "01", "3ffe250102001fff00000000000000" "07",
         1766, 2794, 0x2CC18CD5, 0x40207D3D),
        ("ff02000000000000000000000000" "0001", "3ffe050100080000026097fffe40" "efab",
         4739, 14230, 0x0F0C461C, 0xDDE51BBF),
        ("fe80000000000000020" "0f8fffe2167cf", "3ffe19004545000302" "00f8fffe2167cf",
         38024, 44251, 0x4B61E985, 0x02D1FEEF),
    ]
    import socket
    import struct

    out4 = []
    for dst, src, dport, sport, l3, l34 in v4:
        t = socket.inet_aton(src) + socket.inet_aton(dst)
        out4.append({"l3": t.hex(), "l3l4": (t + struct.pack(">HH", sport, dport)).hex(),
                     "hash_l3": l3, "hash_l3l4": l34})
    out6 = []
    for dst, src, dport, sport, l3, l34 in v6:
        t = bytes.fromhex(src) + bytes.fromhex(dst)
        out6.append({"l3": t.hex(), "l3l4": (t + struct.pack(">HH", sport, dport)).hex(),
                     "hash_l3": l3, "hash_l3l4": l34})
    return {
        "source": "Intel 82599 RSS verification suite as held by dpdk/test/test/test_thash.c:60-104",
        "key": "6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b477cb2da38030f20c"
               "6a42b73bbeac01fa",
        "v4": out4, "v6": out6,
    }


def tuple_of(w: np.ndarray) -> bytes:
    ihl4 = (int(w[14]) & 0xF) * 4
    p = 14 + ihl4
    b = w.tobytes()
    return bytes([b[29], b[28], b[27], b[26], b[33], b[32], b[31], b[30],
                  b[p + 1], b[p], b[p + 3], b[p + 2]])


def synth_fixture(profile: int):
    win, lens = oracle.synth(profile, NFIX, 0, SEED, NFLOWS[profile], STRIDE)
    out = {"win": win.reshape(NFIX, STRIDE), "len": lens,
           "meta": np.array([SEED, profile, NFLOWS[profile], STRIDE], dtype=np.uint64)}
    R = oracle.ref()
    for name, (npr, nq, soft, only) in CONFIGS.items():
        c = oracle.cfg(npr, nq, soft, only)
        q, h = oracle.dispatch_windows(win, STRIDE, lens, c, fast=False)
        if R is not None:
            w2 = win.reshape(NFIX, STRIDE)
            for i in np.nonzero(h)[0]:
                t = tuple_of(w2[i])
                assert R.ref_toeplitz_hash(40, oracle.MLX_KEY, 12, t) == int(h[i]), i
        qi, qs = oracle.process_burst(q, nq)
        out[f"q_{name}"] = q
        out[f"hash_{name}"] = h
        out[f"qidx_{name}"] = qi
        out[f"qstart_{name}"] = qs
    return out


def ref_recorded():
    """Answers of the reference's own compiled code (oracle/_ref) on the seeded
    inputs of the tests that pin the oracle and the INI reader to it, so those
    tests hold where oracle/_ref cannot be built:
      ref_thash.npz        default key, toeplitz_hash over test_oracle.thash_cases()
      ref_kni.npz          kni_set_bitmap over test_kni_oracle.bitmap_specs(), and
                           get_bitmap over test_kni_oracle.lookup_cases()
      ref_ini_events.json  ini_parse over ff_config/*.ini (the five shipped
                           fs/config files, settings only, copied byte for
                           byte) and over test_ffconfig.generated_inis()
    The inputs come from the tests' own generators; only outputs are stored."""
    import tempfile

    import test_ffconfig
    import test_kni_oracle
    import test_oracle

    R, K = oracle.ref(), oracle.ref_kni()
    assert R is not None and K is not None, "oracle/_ref is not built"
    key = np.array([R.ref_default_rsskey()[i] for i in range(40)], np.uint8)
    hashes = np.array([R.ref_toeplitz_hash(kl, k, len(d), d)
                       for kl, k, d in test_oracle.thash_cases()], np.uint32)
    np.savez_compressed(HERE / "ref_thash.npz", key=key, hashes=hashes)

    bitmaps = np.stack([oracle.ref_kni_bitmap(s) for s in test_kni_oracle.bitmap_specs()])
    hits = np.array([bool(K.ref_get_bitmap(raw, bm.ctypes.data))
                     for raw, bm, *_ in test_kni_oracle.lookup_cases(oracle)], np.uint8)
    np.savez_compressed(HERE / "ref_kni.npz", bitmaps=bitmaps, hits=hits)

    def rec(path):
        ev, err = oracle.ref_ini_events(path)
        return {"events": [list(e) for e in ev], "error": err}

    out = {"configs": {p.name: rec(p) for p in sorted((HERE / "ff_config").glob("*.ini"))},
           "generated": []}
    with tempfile.TemporaryDirectory() as tmp:
        for i, data in enumerate(test_ffconfig.generated_inis()):
            p = Path(tmp) / f"g{i}.ini"
            p.write_bytes(data)
            out["generated"].append(rec(p))
    (HERE / "ref_ini_events.json").write_text(json.dumps(out, separators=(",", ":")) + "\n")


def main():
    if sys.argv[1:] == ["ref"]:     # only the reference's recorded answers
        ref_recorded()
        print("reference recordings written to", HERE)
        return
    (HERE / "survey_kat.json").write_text(json.dumps(survey_kat(), indent=1) + "\n")
    (HERE / "thash_82599.json").write_text(json.dumps(thash_82599(), indent=1) + "\n")
    if oracle.ref() is None:
        print("warning: oracle/_ref absent; synth hashes checked by the oracle only")
    for p, name in PROFILES.items():
        np.savez_compressed(HERE / f"synth_{name}.npz", **synth_fixture(p))
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
