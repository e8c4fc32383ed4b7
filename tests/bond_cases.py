# SPDX-License-Identifier: BSD-3-Clause
"""Topology and frames of the bond_output tests (test_bond_cpu.py,
test_bond_gpu.py): the exception corpus plus bonds of every kind bond_output
distinguishes, and frames for each rule of its tuple."""
import functools

import numpy as np

import scenarios as SC
from grout_amd import abi
from grout_amd import synth as S
from grout_amd import topology as T

# bond ifaces (the corpus' own SC.BOND keeps no gr_hip_bond: the CPU node's)
B_RSS, B_L2, B_L34, B_AB, B_NOACT, B_EMPTY, B_MODE, B_ALGO, B_BADRETA, B_SNAT = range(60, 70)
VLAN_B = 70  # VLAN 300 over B_L34
LACP3 = (B_RSS, B_L2, B_L34)  # the LACP bonds over three member ports
# member ports (ids the corpus topology does not name, as a VLAN's missing parent for instance)
MEMBERS = {B_RSS: [100, 101, 102], B_L2: [103, 104, 105], B_L34: [106, 107, 108], B_AB: [109, 110],
           B_NOACT: [111, 112], B_EMPTY: [], B_MODE: [113], B_ALGO: [114], B_BADRETA: [115, 116], B_SNAT: [117, 118]}
# routes: 10.<net>.0.0/16 and 2001:db8:<net>::/48 leave through ...
NET = {B_RSS: 110, B_L2: 111, B_L34: 112, VLAN_B: 113, B_AB: 114, B_NOACT: 115, B_EMPTY: 116, B_MODE: 117,
       B_ALGO: 118, B_BADRETA: 119, B_SNAT: 120}
NET_GROUP = 121  # an ECMP group over nexthops on B_RSS, B_L2 and B_L34
L2_NH = 8  # nexthops (destination MACs) on B_L2, 10.111.<k>.0/24 each: the L2 hash sees nothing else
SRC = "198.18.0.1"
DNAT_MATCH, DNAT_TO = "10.68.3.1", "10.112.0.77"  # DNATed towards B_L34
SNAT_TO = "203.0.113.9"  # SRC leaving through B_SNAT


def topology():
    """The corpus topology with the bonds; -> (topo, nh names)."""
    t, nh = SC.corpus_topology()
    for b, mem in MEMBERS.items():
        for m in mem:
            t.add_port(m, m, "02:00:00:00:01:%02x" % m)
        t.add_iface(b, "BOND", mac="02:00:00:00:02:%02x" % b, flags=abi.IFACE_F_SNAT_STATIC if b == B_SNAT else 0)
    t.add_vlan(VLAN_B, B_L34, 300, mac="02:00:00:00:03:01")
    t.add_bond(B_RSS, "LACP", "RSS", MEMBERS[B_RSS])
    t.add_bond(B_L2, "LACP", "L2", MEMBERS[B_L2])
    t.add_bond(B_L34, "LACP", "L3_L4", MEMBERS[B_L34])
    t.add_bond(B_AB, "ACTIVE_BACKUP", "L3_L4", MEMBERS[B_AB], primary=MEMBERS[B_AB][1])
    t.add_bond(B_NOACT, "LACP", "L3_L4", MEMBERS[B_NOACT], active=[])
    t.add_bond(B_EMPTY, "LACP", "L3_L4", [])
    t.add_bond(B_MODE, 7, "L3_L4", MEMBERS[B_MODE])
    t.add_bond(B_ALGO, "LACP", 9, MEMBERS[B_ALGO])
    t.add_bond(B_BADRETA, "LACP", "L3_L4", MEMBERS[B_BADRETA])["reta"][1::2] = 5  # an index >= n_members
    t.add_bond(B_SNAT, "LACP", "L3_L4", MEMBERS[B_SNAT])
    for i, n in NET.items():
        if i == B_L2:
            continue
        nh["b%d" % i] = t.add_nexthop(i, "100.65.%d.2" % n, "02:00:00:02:%02x:02" % n)
        t.add_route(1, "10.%d.0.0/16" % n, nh["b%d" % i])
        nh["b6_%d" % i] = t.add_nexthop(i, "2001:db8:b:%x::2" % n, "02:00:00:06:%02x:02" % n)
        t.add_route6(1, "2001:db8:%d::/48" % n, nh["b6_%d" % i])
    for k in range(L2_NH):
        s = t.add_nexthop(B_L2, "100.65.111.%d" % (2 + k), "02:00:00:02:6f:%02x" % (0x10 + 7 * k))
        t.add_route(1, "10.111.%d.0/24" % k, s)
        s6 = t.add_nexthop(B_L2, "2001:db8:b:6f::%x" % (2 + k), "02:00:00:06:6f:%02x" % (0x10 + 7 * k))
        t.add_route6(1, "2001:db8:111:%x::/64" % k, s6)
        nh.setdefault("b%d" % B_L2, s)
        nh.setdefault("b6_%d" % B_L2, s6)
    nh["bgrp"] = t.add_group([nh["b%d" % b] for b in LACP3], reta_size=8)
    t.add_route(1, "10.%d.0.0/16" % NET_GROUP, nh["bgrp"])
    nh["bgrp6"] = t.add_group([nh["b6_%d" % b] for b in LACP3], reta_size=8)
    t.add_route6(1, "2001:db8:%d::/48" % NET_GROUP, nh["bgrp6"])
    t.nh[nh["dnat"]]["ipv4"] = T.ip4("16.1.0.77")  # the corpus' DNAT nexthop: behind the plain nexthop "fwd"
    nh["bdnat"] = t.add_nexthop(SC.P0, ipv4=DNAT_TO, nh_type="DNAT")
    t.add_route(1, DNAT_MATCH + "/32", nh["bdnat"])
    t.add_snat44_static(B_SNAT, SRC, SNAT_TO)
    return t, nh


def ports(f, off, sport, dport):
    """Frame bytes with the L4 ports at byte `off` (sport first, as TCP and UDP store them)."""
    b = bytearray(f)
    b[off:off + 4] = sport.to_bytes(2, "big") + dport.to_bytes(2, "big")
    return bytes(b)


def crafted4(net, pfx, k0=0):
    """[(label, frame, meta kw)] towards 10.<net>.0.0/16: one frame per rule of the IPv4 tuple."""
    F = []
    d = lambda k: "10.%d.%d.%d" % (net, (k0 + k) % L2_NH, 1 + k)
    add = lambda lab, f, **kw: F.append((pfx + " " + lab, f, kw))
    fr = S.frame
    add("tcp", ports(fr(dst=d(0), proto=6), 34, 40000, 443))
    add("tcp ports swapped", ports(fr(dst=d(0), proto=6), 34, 443, 40000))
    add("udp", ports(fr(dst=d(1)), 34, 40000, 53))
    add("icmp", ports(fr(dst=d(2), proto=1), 34, 0x0800, 0x1234))  # not ports: ignored
    add("udp DF", ports(fr(dst=d(3), flags_frag=0x4000), 34, 40000, 53))  # the whole field != 0: ports 0
    add("udp MF", ports(fr(dst=d(4), flags_frag=0x2000), 34, 40000, 53))
    add("udp later fragment", ports(fr(dst=d(5), flags_frag=0x0010), 34, 40000, 53))
    add("tcp DF", ports(fr(dst=d(6), proto=6, flags_frag=0x4000), 34, 40000, 443))
    add("udp ihl 6", ports(fr(dst=d(7), ihl=6, options=b"\x01" * 4, length=80), 38, 40001, 53))
    add("tcp ihl 11", ports(fr(dst=d(8), proto=6, ihl=11, options=b"\x01" * 24, length=80), 58, 40002, 443))
    add("udp ihl 12", ports(fr(dst=d(9), ihl=12, options=b"\x01" * 28, length=80), 62, 40003, 53))  # ports 62-65
    add("icmp ihl 12", fr(dst=d(10), proto=1, ihl=12, options=b"\x01" * 28, length=80))  # no ports read
    add("udp ihl 12 DF", ports(fr(dst=d(11), ihl=12, options=b"\x01" * 28, length=80, flags_frag=0x4000), 62, 40003, 53))
    add("rss flag on", ports(fr(dst=d(12)), 34, 40004, 53), rss=0x1234, flag=True)
    add("rss flag off", ports(fr(dst=d(12)), 34, 40004, 53), rss=0x1234)
    add("ttl 1", ports(fr(dst=d(13), ttl=1), 34, 40005, 53))
    add("vlan 100 ingress", ports(fr(dst=d(14)), 34, 40006, 53), vlan=100)
    for j in range(24):  # a spread of flows: every member gets some
        add("flow %d" % j, ports(fr(dst=d(20 + j), src="198.18.%d.%d" % (j, 3 * j + 1)), 34, 1024 + 37 * j, 80 + j),
            rss=0x0101 * j + 5, flag=j % 2 == 0)
    return F


def crafted6(net, pfx):
    """The same for 2001:db8:<net>::/48."""
    F = []
    d = lambda k: "2001:db8:%d:%x::%x" % (net, k % L2_NH, 1 + k)
    add = lambda lab, f, **kw: F.append((pfx + " " + lab, f, kw))
    f6 = S.frame6
    add("tcp6", ports(f6(dst=d(0), next_header=6), 54, 40000, 443))
    add("tcp6 ports swapped", ports(f6(dst=d(0), next_header=6), 54, 443, 40000))
    add("udp6", ports(f6(dst=d(1)), 54, 40000, 53))
    add("icmp6", ports(f6(dst=d(2), next_header=58), 54, 0x8000, 0x1234))
    add("hop-by-hop", ports(f6(dst=d(3), next_header=0), 54, 0x1100, 0x0000))  # the UDP header is further on
    add("fragment header", ports(f6(dst=d(4), next_header=44), 54, 0x1100, 0x0001))
    add("rss6 flag on", ports(f6(dst=d(5)), 54, 40004, 53), rss=0x4321, flag=True)
    add("rss6 flag off", ports(f6(dst=d(5)), 54, 40004, 53), rss=0x4321)
    add("hop 1", ports(f6(dst=d(6), hop=1), 54, 40005, 53))
    for j in range(16):
        add("flow6 %d" % j, ports(f6(dst=d(10 + j), src="2001:db8:ff::%x" % (j * j + 1)), 54, 1024 + 41 * j, 80 + j),
            rss=0x0101 * j + 9, flag=j % 2 == 0)
    return F


def arrays(F, stride=SC.STRIDE):
    n = len(F)
    frames = np.zeros((n, stride), dtype=np.uint8)
    meta = np.zeros(n, dtype=abi.META_DT)
    for i, (_lab, f, kw) in enumerate(F):
        b = np.frombuffer(f[:stride], np.uint8)
        frames[i, :len(b)] = b
        meta[i]["iface"] = kw.get("iface", SC.P0)
        meta[i]["vlan_ck"] = ((kw.get("vlan", 0) & 0xFFF) | (abi.CKSUM_UNKNOWN << 12)
                              | (abi.META_RSS_HASH if kw.get("flag") else 0))
        meta[i]["pkt_len"] = kw.get("pkt_len", len(f))
        meta[i]["rss"] = kw.get("rss", 0)
    return frames, meta, [lab for lab, _f, _kw in F]


@functools.lru_cache(maxsize=None)
def batch():
    """The corpus plus the bond frames; -> (frames, meta, labels). Read-only."""
    name = {B_RSS: "rss", B_L2: "l2", B_L34: "l34", VLAN_B: "vlan/l34", B_AB: "ab", B_NOACT: "noact",
            B_EMPTY: "empty", B_MODE: "mode", B_ALGO: "algo", B_BADRETA: "badreta", B_SNAT: "snat"}
    F = []
    for i, n in NET.items():
        if i == B_SNAT:  # IPv4 only, and no SNAT hit whose L4 checksum lies past the line (nat44_ref refuses those)
            F += [x for x in crafted4(n, name[i]) if "ihl 1" not in x[0]]
            continue
        F += crafted4(n, name[i])
        F += crafted6(n, name[i])
    F += crafted4(NET_GROUP, "group")
    F += crafted6(NET_GROUP, "group")
    udp = lambda d, **kw: ports(S.frame(dst=d, src=SRC, **kw), 34, 40000, 53)
    for k in range(6):  # DNATed towards B_L34: the tuple has the new destination
        F.append(("dnat to l34 %d" % k, ports(S.frame(dst=DNAT_MATCH, src="198.18.1.%d" % k), 34, 2000 + k, 53), {}))
    F.append(("dnat to l34 tcp", ports(S.frame(dst=DNAT_MATCH, src=SRC, proto=6), 34, 40000, 443), {}))
    F.append(("corpus bond (no entry)", udp("10.78.0.9"), {}))
    f2, m2, l2 = arrays(F)
    f1, m1, l1 = SC.corpus_arrays()
    frames, meta = np.concatenate([f1, f2]), np.concatenate([m1, m2])
    frames.setflags(write=False)
    meta.setflags(write=False)
    return frames, meta, l1 + l2


def cycled(n):
    """n packets cycling through batch()'s frames."""
    fr, me, _ = batch()
    idx = np.arange(n) % len(me)
    return np.ascontiguousarray(fr[idx]), np.ascontiguousarray(me[idx])


def fuzz(seed, n=256):
    """n random packets from p0 towards random bonds: random protocol, IHL,
    fragment field, ports, addresses, rss and RSS flag; a valid header checksum."""
    rng = np.random.default_rng(0xB0D0000 + seed)
    nets = list(NET.values()) + [NET_GROUP]
    frames = np.zeros((n, SC.STRIDE), dtype=np.uint8)
    meta = np.zeros(n, dtype=abi.META_DT)
    for i in range(n):
        net = int(rng.choice(nets))
        proto = int(rng.choice([6, 17, 17, 1, 47, int(rng.integers(0, 256))]))
        if rng.integers(0, 4) == 0:
            f = bytearray(S.frame6(dst="2001:db8:%d:%x::%x" % (net, rng.integers(0, L2_NH), rng.integers(1, 1 << 16)),
                                   src="2001:db8:ff::%x" % rng.integers(1, 1 << 16), next_header=proto,
                                   hop=int(rng.integers(1, 65)), length=80))
            f[54:80] = rng.integers(0, 256, 26, dtype=np.uint8).tobytes()
        else:
            ihl = int(rng.choice([5, 5, 5, 6, 8, 11, 12, 13, 15]))
            frag = int(rng.choice([0, 0, 0, 0x4000, 0x2000, 0x0001, 0x1FFF, 0x6000, int(rng.integers(0, 65536))]))
            f = bytearray(S.frame(dst="10.%d.%d.%d" % (net, rng.integers(0, L2_NH), rng.integers(1, 255)),
                                  src="198.%d.%d.%d" % tuple(rng.integers(1, 255, 3)), proto=proto, ihl=ihl,
                                  options=bytes(rng.integers(0, 256, 4 * (ihl - 5), dtype=np.uint8)),
                                  flags_frag=frag, ttl=int(rng.integers(1, 65)), length=SC.STRIDE))
            hl = 14 + 4 * ihl
            f[hl:] = rng.integers(0, 256, SC.STRIDE - hl, dtype=np.uint8).tobytes()
        frames[i, :len(f)] = np.frombuffer(bytes(f), np.uint8)
        meta[i]["iface"] = SC.P0
        meta[i]["vlan_ck"] = (abi.CKSUM_UNKNOWN << 12) | (abi.META_RSS_HASH if rng.integers(0, 2) else 0)
        meta[i]["pkt_len"] = len(f)
        meta[i]["rss"] = int(rng.integers(0, 65536))
    return frames, meta


def members_hit(topo, want):
    """{bond: set of members chosen} from an expect() result's verdicts and members."""
    _l, v, _s, members = want
    hit = {}
    for i in np.flatnonzero(members):
        slot = int(v["nh"][i])
        oif = int(topo.nh[slot]["iface_id"])
        if topo.ifaces[oif]["type"] == abi.IFACE_TYPE["VLAN"]:
            oif = int(topo.ifaces[oif]["parent_id"])
        hit.setdefault(oif, set()).add(int(members[i]))
    return hit

