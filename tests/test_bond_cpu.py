# SPDX-License-Identifier: BSD-3-Clause
"""bond_output without a GPU: the reference's hash (bond_ref.py) against the
anchor values and the algebra of rte_softrss_be, Topology.add_bond's tables,
the new entry points, the RSS flag in the staged metadata, the node hand-back
of a member-port verdict, and that the cases exercise what they claim."""
import ctypes
import ipaddress

import numpy as np
import pytest

import bond_cases as C
import bond_ref as R
import oracle
import scenarios as SC
from grout_amd import abi
from grout_amd import topology as T
from test_node_shim import GROUT_LAYOUT, GROUT_STAGE, RX_DATA_OFF, Layout, apply_counting, mbufs_for

E = abi.EDGE
ip = lambda s: int(ipaddress.IPv4Address(s))


def test_hash_anchor_values():
    """The four values the feature was specified with (computed from rte_thash.h's
    definition of rte_softrss_be over grout's raw key)."""
    assert R.softrss_be(R.tuple_v4(ip("10.0.0.1"), ip("10.78.0.1"), 53, 40000)) == 0x54A72281
    assert R.softrss_be(R.tuple_v4(ip("10.0.0.1"), ip("10.78.0.1"), 0, 0)) == 0x35C99D49
    assert R.softrss_be(bytes.fromhex("02000001001b") + b"\0\0") == 0x6B0540BF
    v6 = bytes(range(1, 33)) + (443).to_bytes(2, "big") + (1234).to_bytes(2, "big")
    assert R.softrss_be(v6) == 0x1092EE3A
    assert [h % 256 for h in (0x54A72281, 0x35C99D49, 0x6B0540BF, 0x1092EE3A)] == [129, 73, 191, 58]


@pytest.mark.parametrize("length", [8, 12, 36])
def test_hash_is_linear(length):
    rng = np.random.default_rng(length)
    for _ in range(1000):
        a, b = rng.integers(0, 256, length, dtype=np.uint8), rng.integers(0, 256, length, dtype=np.uint8)
        assert R.softrss_be(bytes(a ^ b)) == R.softrss_be(bytes(a)) ^ R.softrss_be(bytes(b))
    assert R.softrss_be(bytes(length)) == 0


def test_dport_comes_before_sport():
    a = R.tuple_v4(ip("10.0.0.1"), ip("10.78.0.1"), 53, 40000)
    b = R.tuple_v4(ip("10.0.0.1"), ip("10.78.0.1"), 40000, 53)
    assert a[8:10] == (53).to_bytes(2, "big") and R.softrss_be(a) != R.softrss_be(b)
    # and the tuple read from a frame puts the packet's second port first
    f = np.frombuffer(C.ports(C.S.frame(dst="10.78.0.1", src="10.0.0.1"), 34, 40000, 53)[:64].ljust(64, b"\0"), np.uint8)
    assert R.tuple_of(f, False) == a
    f6 = np.frombuffer(C.ports(C.S.frame6(), 54, 1234, 443)[:64], np.uint8)
    assert R.tuple_of(f6, False)[32:] == (443).to_bytes(2, "big") + (1234).to_bytes(2, "big")


def test_tuple_rules():
    fr = C.S.frame
    line = lambda f: np.frombuffer(f[:64].ljust(64, b"\0"), np.uint8)
    zero = lambda f: R.tuple_of(line(f), False)[8:] == b"\0\0\0\0"
    assert not zero(C.ports(fr(proto=6), 34, 1, 2)) and not zero(C.ports(fr(), 34, 1, 2))
    assert zero(C.ports(fr(proto=1), 34, 1, 2))
    for frag in (0x4000, 0x2000, 0x0010, 0x6000):  # DF alone already: the whole field is compared
        assert zero(C.ports(fr(flags_frag=frag), 34, 1, 2)), hex(frag)
    assert R.tuple_of(line(C.ports(fr(proto=6, ihl=11, options=b"\1" * 24, length=80), 58, 7, 9)), False)[8:] \
        == b"\0\x09\0\x07"
    assert R.tuple_of(line(fr(ihl=12, options=b"\1" * 28, length=80)), False) is R.KEEP
    assert R.tuple_of(line(fr(ihl=12, options=b"\1" * 28, length=80, proto=1)), False) is not R.KEEP
    assert R.tuple_of(line(fr(ihl=12, options=b"\1" * 28, length=80, flags_frag=0x4000)), False) is not R.KEEP
    assert R.tuple_of(line(fr(dst_mac="02:00:00:01:00:1b")), True) == bytes.fromhex("02000001001b0000")
    f6 = C.S.frame6
    assert R.tuple_of(line(C.ports(f6(next_header=0), 54, 1, 2)), False)[32:] == b"\0\0\0\0"
    assert len(R.tuple_of(line(f6()), False)) == 36


def test_add_bond_tables():
    ports = list(range(30, 38))
    t = T.Topology()
    for n in (1, 2, 3, 8):
        b = t.add_bond(60, "LACP", "L3_L4", ports, active=ports[8 - n:])
        ids = list(range(8 - n, 8))
        assert list(b["reta"]) == [ids[i % n] for i in range(256)] and b["n_members"] == 8
    b = t.add_bond(60, "LACP", "RSS", ports[:3], active=[])
    assert (b["reta"] == 0xFF).all() and b["mode"] == 2 and b["algo"] == 1 and list(b["members"][:3]) == ports[:3]
    b = t.add_bond(61, "ACTIVE_BACKUP", "L2", ports[:3], active=ports[1:3])
    assert b["active_member"] == 1 and (b["reta"] == 1).all() and b["mode"] == 1
    assert t.add_bond(61, "ACTIVE_BACKUP", "L2", ports[:3], primary=ports[2])["active_member"] == 2
    assert t.add_bond(61, "ACTIVE_BACKUP", "L2", ports[:3], active=ports[:2], primary=ports[2])["active_member"] == 0
    b = t.add_bond(61, "ACTIVE_BACKUP", "L2", ports[:3], active=[])
    assert b["active_member"] == 0xFF and (b["reta"] == 0xFF).all()
    assert set(t.bonds) == {60, 61}
    with pytest.raises(ValueError):
        t.add_bond(62, "LACP", "L2", list(range(9)))


def test_library_exports_the_bond_entry_points():
    lib = ctypes.CDLL(abi.LIB_HIP)
    for name in ("gr_hip_bond_set", "gr_hip_bond_del", "gr_hip_bond_output_set", "gr_hip_bond_output_get"):
        assert hasattr(lib, name), name
        assert name in abi.HIP_API
    # additive: no version, edge count or mirrored struct size moved
    assert lib.gr_hip_abi_version() == abi.ABI_VERSION == 3
    assert abi.E_COUNT == 51
    assert (abi.IFACE_DT.itemsize, abi.NH_DT.itemsize, abi.META_DT.itemsize, abi.VERDICT_DT.itemsize) == (32, 48, 8, 8)
    assert abi.MBUF_DT.itemsize == 40 and abi.STATS_DT.itemsize == 32 and abi.BOND_DT.itemsize == 280
    assert abi.META_RSS_HASH == 0x8000 and abi.META_RSS_HASH & (0xFFF | (3 << 12) | abi.META_WALK) == 0
    # without a context: an error, not a crash (with one: test_bond_gpu.py)
    H = abi.hip()
    b = np.zeros(1, dtype=abi.BOND_DT)
    assert H.gr_hip_bond_set(None, 60, b.ctypes.data) == -22 and H.gr_hip_bond_del(None, 60) == -22
    assert H.gr_hip_bond_output_set(None, 1) == -22 and H.gr_hip_bond_output_get(None) == -22


def test_staging_sets_the_rss_flag_from_ol_flags():
    """gr_hip_node_append_mbufs' staging: RTE_MBUF_F_RX_RSS_HASH (ol_flags bit
    1) becomes bit 15 of vlan_ck, and nothing else of the metadata changes."""
    fr, me, _ = SC.corpus_arrays()
    keep = ((me["vlan_ck"] >> 12) & 3) != 3
    fr, me = fr[keep][:64], me[keep][:64]
    n = len(me)
    bufs, ref = mbufs_for(fr, me)
    L, G = GROUT_LAYOUT, GROUT_STAGE
    ifobj = np.zeros((1024, 64), dtype=np.uint8)
    ifobj.view(np.uint16)[:, G["iface_id"] // 2] = np.arange(1024)
    lay = Layout(**L, **G, n_ifaces=0, n_nh=0, ifaces=None, nh=None)
    fn = ctypes.CDLL(abi.LIB_HIP).gr_node_stage_mbufs
    P = ctypes.c_void_p
    fn.argtypes = [P, ctypes.c_uint32, P, ctypes.c_uint32, ctypes.c_uint64, P, P, P]
    fn.restype = ctypes.c_uint64
    ck_bits = np.array([0, G["ck_bad"], G["ck_good"]], dtype=np.uint64)
    flag = (np.arange(n) % 3 == 0)
    out = {}
    for name, extra in (("off", np.uint64(1 << 40) | np.uint64(1)), ("on", np.uint64(1 << 40) | np.uint64(1) | np.uint64(2))):
        mem = np.zeros((n, 256), dtype=np.uint8)
        U16, U32, U64 = mem.view(np.uint16), mem.view(np.uint32), mem.view(np.uint64)
        U64[:, G["buf_addr"] // 8] = ref["frame"] - RX_DATA_OFF
        U16[:, L["data_off"] // 2] = RX_DATA_OFF
        U16[:, L["data_len"] // 2] = ref["data_len"]
        U32[:, L["pkt_len"] // 4] = ref["pkt_len"]
        U32[:, G["rss"] // 4] = 0xABCD0000 + np.arange(n)
        U64[:, G["ol_flags"] // 8] = ck_bits[ref["ck"]] | np.where(flag, extra, np.uint64(1 << 40) | np.uint64(1))
        U64[:, (L["priv"] + L["priv_iface"]) // 8] = np.where(
            ref["iface"] != 0, ifobj.ctypes.data + 64 * ref["iface"].astype(np.uint64), 0).astype(np.uint64)
        U16[:, (L["priv"] + L["priv_vlan_id"]) // 2] = ref["vlan_id"]
        ptrs = (mem.ctypes.data + np.arange(n, dtype=np.uint64) * 256).astype(np.uint64)
        pos = np.zeros(n, dtype=np.uint32)
        meta = np.zeros(n, dtype=abi.META_DT)
        assert fn(ptrs.ctypes.data, n, ctypes.addressof(lay), 64, 0, pos.ctypes.data, None, meta.ctypes.data) == n
        out[name] = meta
    off, on = out["off"], out["on"]
    assert not (off["vlan_ck"] & abi.META_RSS_HASH).any()  # ol_flags bit 0 (RX_VLAN) and bit 40 are not the flag
    assert np.array_equal((on["vlan_ck"] & abi.META_RSS_HASH) != 0, flag)
    assert np.array_equal(on["vlan_ck"] & 0x7FFF, off["vlan_ck"])
    for f in ("iface", "pkt_len", "rss"):
        assert np.array_equal(on[f], off[f])
    assert np.array_equal(off["rss"], (np.arange(n) & 0xFFFF).astype(np.uint16))


@pytest.fixture(scope="module")
def corpus():
    t, nh = C.topology()
    fr, me, lab = C.batch()
    return t, nh, fr, me, lab, R.expect(t, fr, me)


def test_cases_cover_what_they_claim(corpus):
    t, nh, fr, me, lab, want = corpus
    lines, v, st, members = want
    plain = oracle.Oracle(t).process(fr, me)
    off = R.expect(t, fr, me, on=False)
    assert all(np.array_equal(a, b) for a, b in zip(plain, off[:3])) and not off[3].any()
    assert np.array_equal(lines, plain[0])  # the step only reads the line
    by = {l: i for i, l in enumerate(lab)}
    name = lambda l: abi.EDGE_NAMES[v["edge"][by[l]]]
    hit = C.members_hit(t, want)
    for b in C.LACP3:  # every member of every three-port LACP bond gets a packet
        assert hit[b] == set(C.MEMBERS[b]), (b, hit.get(b))
    assert hit[C.B_AB] == {C.MEMBERS[C.B_AB][1]} and hit[C.B_BADRETA] == {C.MEMBERS[C.B_BADRETA][0]}
    at_bond = plain[1]["edge"] == E["bond_output"]
    assert ((members != 0) == (at_bond & (v["edge"] == E["port_output"]))).all()
    assert (v["edge"][~at_bond] == plain[1]["edge"][~at_bond]).all()
    for p in ("noact", "empty", "mode", "algo"):  # no member: the bond edge, the bond as iface
        assert name(p + " udp") == "bond_output" and name(p + " udp6") == "bond_output", p
    assert v["iface"][by["empty udp"]] == C.B_EMPTY
    assert name("corpus bond (no entry)") == "bond_output" and name("bond") == "bond_output"
    kept = [l for l in lab if l.startswith("badreta") and v["edge"][by[l]] == E["bond_output"]]
    assert 5 < len(kept) < 40  # half of the table names index 5
    for p in ("rss", "l34", "vlan/l34", "group"):
        assert name(p + " icmp ihl 12") == "port_output" and name(p + " udp ihl 12 DF") == "port_output", p
    assert name("l34 udp ihl 12") == "bond_output" and name("rss udp ihl 12") == "bond_output"
    assert name("l2 udp ihl 12") == "port_output" and name("ab udp ihl 12") == "port_output"
    assert name("l34 tcp ihl 11") == "port_output" and name("l34 ttl 1") == "ip_error_ttl_exceeded"
    # the RSS bond follows meta.rss only with the flag; the L3_L4 bond never does
    i, j = by["rss rss flag on"], by["rss rss flag off"]
    assert members[i] == C.MEMBERS[C.B_RSS][int(t.bonds[C.B_RSS]["reta"][0x1234 % 256])]
    assert members[j] == R.select(t.bonds[C.B_L34], lines[j]) - C.MEMBERS[C.B_L34][0] + C.MEMBERS[C.B_RSS][0]
    assert members[by["l34 rss flag on"]] == members[by["l34 rss flag off"]]
    # VLAN over a bond: the member as iface, the sub-interface, the bond and the member all counted
    i = by["vlan/l34 udp"]
    assert v["iface"][i] in C.MEMBERS[C.B_L34] and t.nh[v["nh"][i]]["iface_id"] == C.VLAN_B
    n_vlan = sum(1 for l in lab if l.startswith("vlan/l34") and v["edge"][by[l]] in (E["port_output"], E["bond_output"]))
    assert st["tx_packets"][C.VLAN_B] == n_vlan
    # per bond: the members' tx counters = the bond's minus the packets that kept the bond edge
    for b, mem in C.MEMBERS.items():
        kept = ((v["edge"] == E["bond_output"]) & (v["iface"] == b)).sum()
        for f in ("tx_packets", "tx_bytes"):
            k = kept if f == "tx_packets" else me["pkt_len"][(v["edge"] == E["bond_output"]) & (v["iface"] == b)].sum()
            assert st[f][mem].sum() == st[f][b] - k, (b, f)
    assert st["tx_packets"][C.MEMBERS[C.B_L34]].sum() > 60 and st["tx_packets"][C.MEMBERS[C.B_NOACT]].sum() == 0
    # the fuzz batches reach every algo
    f, m = C.fuzz(3)
    hit = C.members_hit(t, R.expect(t, f, m))
    assert all(hit.get(b) for b in C.LACP3)


def test_node_hand_back_of_a_member_port_verdict(corpus):
    """A port_output verdict whose iface is a bond's member port hands back
    like any port_output: the member as the mbuf's iface, the VLAN id of the
    sub-interface the nexthop leaves through, and per-iface counters equal to
    the kernel's (the sub-interface, the bond above it and the member)."""
    t, nh, fr, me, lab, want = corpus
    lines, v, st, members = want
    _, v0, _, mb0, _ = oracle.Oracle(t).process_mbufs(fr, me)
    assert np.array_equal(v0, R.expect(t, fr, me, on=False)[1])
    bufs, m = mbufs_for(fr, me)
    _ns, got_st = apply_counting(m, lines, v, t)
    sel = members != 0
    assert sel.sum() > 300
    assert (m["edge"][sel] == E["port_output"]).all() and np.array_equal(m["iface"][sel], members[sel])
    # everything else of those mbufs as at the bond edge; the others untouched by the change
    for f in ("pkt_len", "data_len", "data_off", "packet_type", "vlan_id", "domain", "nh"):
        assert np.array_equal(m[f], mb0[f]), f
    assert np.array_equal(m["edge"][~sel], mb0["edge"][~sel]) and np.array_equal(m["iface"][~sel], mb0["iface"][~sel])
    by = {l: i for i, l in enumerate(lab)}
    i = by["vlan/l34 tcp"]
    assert m["vlan_id"][i] == 300 and m["iface"][i] in C.MEMBERS[C.B_L34] and m["edge"][i] == E["port_output"]
    assert m["vlan_id"][by["l34 tcp"]] == 0
    for f in st.dtype.names:
        assert np.array_equal(got_st[f], st[f]), (f, np.flatnonzero(got_st[f] != st[f]).tolist())
