# SPDX-License-Identifier: BSD-3-Clause
"""Static NAT44 without a GPU: the reference (nat44_ref.py) against grout's
formula and a full recomputation, the new entry points, the node hand-back's
view of the verdict flags, the Topology helpers, and that the reference
accepts every batch the GPU tests hand it."""
import ctypes
import itertools

import numpy as np
import pytest

import nat44_cases as C
import nat44_ref as R
import oracle
import scenarios as SC
from grout_amd import abi
from grout_amd import synth as S
from grout_amd import topology as T
from test_node_shim import apply, compare_mbufs, mbufs_for

E = abi.EDGE
CORNERS = [0, 1, 0xFFFE, 0xFFFF, 0x8000, 0x7FFF]


def _fold(s):
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def _same(a, b):
    """Equal as one's complement numbers (0x0000 and 0xffff are both zero)."""
    return a == b or {a, b} == {0, 0xFFFF}


def test_fixup32_equals_full_recomputation():
    """Over the corner values of the checksum and of both halves of the old
    and new datum (carries in neither, either and both halves): the fix-up
    equals the checksum recomputed over the changed data."""
    for ck, ol, oh, nl, nh in itertools.product(CORNERS, repeat=5):
        old, new = ol | (oh << 16), nl | (nh << 16)
        # data whose checksum is ck: one word d beside the datum's two halves
        d = (_fold((~ck & 0xFFFF) + (~ol & 0xFFFF) + (~oh & 0xFFFF))) % 0xFFFF
        assert _same(~_fold(d + ol + oh) & 0xFFFF, ck)
        want = ~_fold(d + nl + nh) & 0xFFFF
        got = R.fixup32(ck, old, new)
        assert _same(got, want), (hex(ck), hex(old), hex(new), hex(got), hex(want))


@pytest.mark.parametrize("ck,old,new,want", [
    # worked by hand from nat_datapath.h:33-46: sum = ~ck + ~old.lo + new.lo + ~old.hi + new.hi,
    # two folds, complement
    (0x0000, 0x00000000, 0x00000000, 0x0000),  # ffff + ffff + ffff = 2fffd -> ffff -> 0000
    (0xFFFF, 0x00000000, 0x00000000, 0x0000),  # 0 + ffff + ffff = 1fffe -> ffff -> 0000: ffff is not kept
    (0xFFFF, 0xFFFFFFFF, 0x00000000, 0xFFFF),  # every term 0: the only way to ffff
    (0x1234, 0x0A000001, 0x0A000002, 0x1233),  # edcb + (fffe + 0002) + (f5ff + 0a00) = 2edca -> edcc
    (0x0001, 0x00010001, 0xFFFFFFFF, 0x0003),  # fffe + 1fffd + 1fffd = 4fff8 -> fffc: carries in both halves
    (0xBEEF, 0x0100A8C0, 0x010011AC, 0x5604),  # 192.168.0.1 -> 172.17.0.1 as stored:
                                               # 4110 + (573f + 11ac) + (feff + 0100) = 1a9fa -> a9fb
])
def test_fixup32_hand_vectors(ck, old, new, want):
    assert R.fixup32(ck, old, new) == want


def _ip_ok(line):
    ihl = int(line[14]) & 0xF
    return _fold(sum(int.from_bytes(bytes(line[14 + i:16 + i]), "big") for i in range(0, 4 * ihl, 2))) == 0xFFFF


def test_rewrite_keeps_the_header_checksum_and_follows_the_l4_rules():
    for which, new, pfx in (("dst", "16.1.0.77", "dnat"), ("src", C.SNAT_TO, "snat")):
        a = 30 if which == "dst" else 26
        for lab, f, _kw in C.crafted("10.68.1.1", C.SRC, "10.68.1.1" if which == "dst" else C.SRC, new, pfx):
            line = np.frombuffer(f[:64].ljust(64, b"\0"), np.uint8).copy()
            before = line.copy()
            assert _ip_ok(line), lab
            assert R.rewrite_row(line, which, T.ip4(new)), lab
            assert _ip_ok(line), lab
            assert bytes(line[a:a + 4]) == T.ip4(new).to_bytes(4, "big")
            changed = set(np.flatnonzero(line != before))
            off = R.l4_cksum_off(before)
            allowed = {24, 25} | set(range(a, a + 4)) | ({off, off + 1} if off is not None else set())
            assert changed <= allowed, (lab, changed)
            if "frag non-first" in lab or "offset" in lab or "icmp" in lab:
                assert off is None and changed <= {24, 25} | set(range(a, a + 4)), lab
            if lab.endswith("udp cksum 0"):
                assert bytes(line[40:42]) == b"\0\0"
            if lab.endswith("udp cksum -> 0"):
                assert bytes(line[40:42]) == b"\xff\xff"
            if lab.endswith(" tcp cksum 0"):  # TCP has no zero rule
                assert bytes(line[50:52]) != b"\0\0"
    for lab, f, _kw in C.crafted_out_of_line("10.68.1.1", C.SRC, "x"):
        line = np.frombuffer(f[:64], np.uint8).copy()
        before = line.copy()
        assert not R.rewrite_row(line, "dst", 1) and np.array_equal(line, before), lab
    # rows together: the out-of-line ones are refused, the others rewritten
    F = C.crafted_out_of_line("10.68.1.1", C.SRC, "x") + C.crafted("10.68.1.1", C.SRC, "10.68.1.1", "16.1.0.77", "y")[:3]
    lines = np.stack([np.frombuffer(f[:64].ljust(64, b"\0"), np.uint8) for _lab, f, _kw in F]).copy()
    assert list(R.rewrite(lines, "dst", [T.ip4("16.1.0.77")] * len(F))) == [False] * 3 + [True] * 3


def test_library_exports_the_nat44_entry_points():
    lib = ctypes.CDLL(abi.LIB_HIP)
    for name in ("gr_hip_nat44_set", "gr_hip_nat44_get", "gr_hip_snat44_static_add", "gr_hip_snat44_static_del",
                 "gr_hip_snat44_static_clear"):
        assert hasattr(lib, name), name
        assert name in abi.HIP_API
    assert lib.gr_hip_abi_version() == abi.ABI_VERSION == 3
    assert abi.E_COUNT == 51
    # without a context: an error, not a crash
    abi.hip()
    assert abi.hip().gr_hip_nat44_set(None, 3) == -22 and abi.hip().gr_hip_nat44_get(None) == -22
    assert abi.hip().gr_hip_snat44_static_add(None, 2, 1, 2) == -22
    assert abi.hip().gr_hip_snat44_static_del(None, 2, 1) == -22
    assert abi.hip().gr_hip_snat44_static_clear(None) == -22


def test_node_hand_back_ignores_the_nat_flags():
    """A verdict with GR_HIP_VERDICT_DNAT | _SNAT in its domain leaves the
    mbuf (eth_input_mbuf_data.domain among it) and the node counters as the
    same verdict without them."""
    t, _ = SC.corpus_topology()
    fr, me, lab = SC.corpus_arrays()
    lines, v, _, want, ns_want = oracle.Oracle(t).process_mbufs(fr, me)
    assert (v["domain"] == abi.DOMAIN["LOCAL"]).sum() > 50
    flagged = v.copy()
    flagged["domain"] |= abi.VERDICT_DNAT | abi.VERDICT_SNAT
    assert (flagged["domain"] == (2 | 0x80 | 0x40)).sum() > 50
    bufs, m = mbufs_for(fr, me)
    ns = apply(m, lines, flagged, t)
    compare_mbufs(m, want, bufs, lines, lab)
    assert m["domain"].max() <= 5
    assert np.array_equal(ns["packets"], ns_want["packets"]) and np.array_equal(ns["calls"], ns_want["calls"])
    L = abi.hip()
    for e in range(abi.E_COUNT):  # the edge -> node table never sees the domain
        assert L.gr_hip_edge_node(e, 7, 0) >= -1


def test_topology_nat_helpers():
    t = T.base_ports()
    a = t.add_nexthop(T.PORT_IFACE[0], nh_type="DNAT")
    assert t.nh[a]["ipv4"] == 0  # the default stays 0
    b = t.add_nexthop(T.PORT_IFACE[0], ipv4="10.1.1.1", nh_type="DNAT")
    assert t.nh[b]["ipv4"] == T.ip4("10.1.1.1") and t.nh[b]["af"] == abi.AF_UNSPEC
    assert bytes(t.nh[b:b + 1].tobytes()[8:12]) == bytes([10, 1, 1, 1])  # network order in memory
    n_routes = len(t.route_array())
    s = t.add_dnat44(T.PORT_IFACE[1], "192.0.2.1", "10.9.9.9")
    assert t.nh[s]["type"] == abi.NH_T["DNAT"] and t.nh[s]["ipv4"] == T.ip4("10.9.9.9")
    r = t.route_array()[n_routes:]
    assert len(r) == 1 and r[0]["ip"] == T.ip4("192.0.2.1") and r[0]["prefixlen"] == 32 and r[0]["nh"] == s
    assert t.snat44_static == [(T.PORT_IFACE[1], T.ip4("10.9.9.9"), T.ip4("192.0.2.1"))]
    assert t.ifaces[T.PORT_IFACE[1]]["flags"] & abi.IFACE_F_SNAT_STATIC
    with pytest.raises(ValueError):
        t.add_snat44_static(T.PORT_IFACE[1], "10.9.9.9", "192.0.2.2")


def test_dnat44_pair_round_trip():
    """add_dnat44's two halves undo each other: a packet DNATed on the way in
    and its reply SNATed on the way out (both through the reference)."""
    t = T.base_ports()
    t.add_address(T.PORT_IFACE[0], "172.16.0.1/24")
    t.add_route(1, "10.9.9.0/24", t.add_nexthop(T.PORT_IFACE[1], "172.16.1.2", "02:00:00:01:00:2d"))
    t.add_route(1, "198.18.0.0/16", t.add_nexthop(T.PORT_IFACE[0], "172.16.0.2", "02:00:00:01:00:2e"))
    t.add_dnat44(T.PORT_IFACE[0], "192.0.2.1", "10.9.9.9")
    req = C.with_l4(S.frame(dst="192.0.2.1", src="198.18.0.1"), 40, 0xBEEF)
    rep = C.with_l4(S.frame(dst="198.18.0.1", src="10.9.9.9", dst_mac=T.PORT_MAC[1]), 40, 0xBEEF)
    fr, me = S.pack([req, rep], iface=[T.PORT_IFACE[0], T.PORT_IFACE[1]])
    out, v, _ = R.expect(t, t.snat44_static, fr, me)
    assert list(v["edge"]) == [E["port_output"]] * 2
    assert list(v["domain"]) == [2 | abi.VERDICT_DNAT, 2 | abi.VERDICT_SNAT]
    assert bytes(out[0, 30:34]) == bytes([10, 9, 9, 9]) and bytes(out[1, 26:30]) == bytes([192, 0, 2, 1])
    assert _ip_ok(out[0]) and _ip_ok(out[1])
    # mask off: today's two CPU edges
    out0, v0, _ = R.expect(t, t.snat44_static, fr, me, dnat=False, snat=False)
    assert list(v0["edge"]) == [E["dnat44_static"], E["ip_output_snat"]] and (v0["domain"] == 2).all()


def test_reference_accepts_the_gpu_batches():
    """expect() raises on none of the batches the GPU tests compare against,
    marks the rows it should, and refuses the out-of-line SNAT hits."""
    t, nh, rules = C.topology()
    fr, me, lab = C.batch()
    out, v, st = R.expect(t, rules, fr, me)
    dn, sn = (v["domain"] & abi.VERDICT_DNAT) != 0, (v["domain"] & abi.VERDICT_SNAT) != 0
    by = {l: i for i, l in enumerate(lab)}
    name = lambda i: abi.EDGE_NAMES[v["edge"][i]]
    assert dn[by["dnat"]] and name(by["dnat"]) == "port_output" and v["nh"][by["dnat"]] == nh["fwd"]
    assert not dn[by["dnat tcp ihl 9"]] and name(by["dnat tcp ihl 9"]) == "dnat44_static"
    assert not dn[by["dnat udp ihl 11"]] and name(by["dnat udp ihl 11"]) == "dnat44_static"
    assert np.array_equal(out[by["dnat tcp ihl 9"]], fr[by["dnat tcp ihl 9"], :64])
    assert dn[by["dnat tcp ihl 8"]] and dn[by["dnat udp ihl 10"]] and dn[by["dnat frag non-first"]]
    assert dn[by["dnat ttl 1"]] and name(by["dnat ttl 1"]) == "ip_error_ttl_exceeded"
    assert sn[by["snat tcp"]] and name(by["snat tcp"]) == "port_output" and not dn[by["snat tcp"]]
    assert not sn[by["snat miss tcp"]] and name(by["snat miss tcp"]) == "port_output"
    assert np.array_equal(out[by["snat miss tcp"], 26:64], fr[by["snat miss tcp"], 26:64])
    assert not sn[by["snat miss tcp ihl 9"]] and name(by["snat miss tcp ihl 9"]) == "port_output"
    assert dn[by["dnat+snat udp"]] and sn[by["dnat+snat udp"]]
    assert dn[by["dnat+snat vlan 100 ingress"]] and sn[by["dnat+snat vlan 100 ingress"]]
    want = {"plain": "port_output", "local": "ip_input_local", "noroute": "ip_error_dest_unreach",
            "link": "ip_hold", "unres": "ip_hold", "vlan": "port_output", "snat_dyn": "ip_output_snat"}
    for k, e in want.items():
        i = by["dnat to " + k]
        assert dn[i] and name(i) == e, (k, name(i))
    assert v["nh"][by["dnat to noroute"]] == 0
    assert len({int(v["nh"][by["dnat to group rss %d" % r]]) for r in range(8)}) == 4
    assert name(by["dnat to mtu frag"]) == "ip_fragment" and name(by["dnat to mtu DF"]) == "ip_error_frag_needed"
    assert not dn[by["dnat other host mac"]] and not dn[by["dnat bad cksum"]]
    assert name(by["snat port20 no rule"]) == "port_output" and not sn[by["snat port20 no rule"]]
    assert not dn[by["dnat"] - 1] and name(by["snat egress"]) == "port_output"  # the corpus' own rows
    assert bytes(out[by["snat udp cksum -> 0"], 40:42]) == b"\xff\xff"
    assert bytes(out[by["dnat udp cksum -> 0"], 40:42]) == b"\xff\xff"
    assert bytes(out[by["snat udp cksum 0"], 40:42]) == b"\0\0"
    for i in np.flatnonzero(dn | sn):
        assert _ip_ok(out[i]), lab[i]
    # the sub-masks and the lines-only view
    for kw in (dict(dnat=False), dict(snat=False), dict(dnat=False, snat=False), dict(lines_only=True)):
        R.expect(t, rules, fr, me, **kw)
    o_plain = oracle.Oracle(t).process(fr, me)
    o_off = R.expect(t, rules, fr, me, dnat=False, snat=False)
    assert all(np.array_equal(a, b) for a, b in zip(o_plain, o_off))
    # the out-of-line SNAT hits are refused
    rf, rm, _ = C.refused_batch()
    with pytest.raises(ValueError):
        R.expect(t, rules, rf, rm)
    _, rv, _ = oracle.Oracle(t).process(rf, rm)
    assert (rv["edge"] == E["ip_output_snat"]).all()
    # the streams
    ts = C.stream_topology()
    for n, seed in ((64 * 3 + 7, 0xA11), (4096, 0xA12)):
        sf, sm = C.stream(n, seed)
        _, sv, _ = R.expect(ts, ts.snat44_static, sf, sm)
        d, s = (sv["domain"] & abi.VERDICT_DNAT) != 0, (sv["domain"] & abi.VERDICT_SNAT) != 0
        assert d.sum() > n // 5 and s.sum() > n // 12 and (d & s).sum() > 0
    # the rule tables
    for rl in C.table_rule_sets():
        R.expect(t, rl, *C.table_batch())
