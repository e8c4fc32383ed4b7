# SPDX-License-Identifier: BSD-3-Clause
"""Reference for the kernel's bond_output (gr_hip_bond_output_set): a plain
Python restatement of grout's node (modules/infra/datapath/bond_output.c:35-237)
applied where the unchanged oracle stops at bond_output.

* softrss_be: rte_softrss_be as DPDK publishes it in rte_thash.h, the plain
  loop over the set bits of each tuple word, over the raw key of
  bond_output.c:37-41 (grout does not convert it). DPDK is not part of this
  repository: parity with it rests on the published definition.
* tuple_of / select: hash_tx_member and bond_select_tx_member on the 64-byte
  header line as eth_output left it.
* apply / expect: what the kernel must give for a batch.

A bond is one abi.BOND_DT record (Topology.add_bond, Topology.bonds).
"""
import numpy as np

import oracle
from grout_amd import abi

E = abi.EDGE
KEY = bytes([
    0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3,
    0x8f, 0xb0, 0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3,
    0x80, 0x30, 0xf2, 0x0c, 0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa,
])
M32 = 0xFFFFFFFF
KEEP = "keep"  # select(): the kernel cannot decide from the line, the packet keeps the bond edge


def _words(b):
    return [int.from_bytes(bytes(b[i:i + 4]), "little") for i in range(0, len(b), 4)]


def softrss_be(tup):
    """rte_softrss_be(input_tuple, len(tup) / 4, KEY): K[j] and in[j] are the
    uint32_t a little-endian CPU loads from the key and tuple bytes."""
    assert len(tup) % 4 == 0 and len(tup) + 4 <= len(KEY)
    k, ret = _words(KEY), 0
    for j, w in enumerate(_words(tup)):
        for i in range(32):
            if w & (1 << i):
                ret ^= ((k[j] << (31 - i)) & M32) | (k[j + 1] >> (i + 1))  # i = 31: a 64-bit shift by 32, 0
    return ret


def tuple_v4(src, dst, dport, sport):
    """struct rte_ipv4_tuple from host-order values: addresses, then dport, then sport, as stored."""
    return src.to_bytes(4, "big") + dst.to_bytes(4, "big") + dport.to_bytes(2, "big") + sport.to_bytes(2, "big")


def tuple_of(line, l2):
    """The bytes hash_tx_member hashes for `line` (:69-171), or KEEP when an
    IPv4 packet's ports lie past byte 63. After eth_output the ether type is
    IPv4 or IPv6 and untagged (port_tx inserts the tag), so the TCI is 0."""
    line = bytes(line)
    if l2:
        return line[0:6] + b"\0\0"
    if line[12:14] == b"\x08\x00":
        ports = b"\0\0\0\0"
        if line[23] in (6, 17) and line[20:22] == b"\0\0":  # fragment_offset == 0: DF and MF included
            l4 = 14 + 4 * (line[14] & 0xF)
            if l4 + 4 > abi.LINE:
                return KEEP
            ports = line[l4 + 2:l4 + 4] + line[l4:l4 + 2]  # dport, then sport
        return line[26:34] + ports
    assert line[12:14] == b"\x86\xdd", "after eth_output the frame is IPv4 or IPv6"
    ports = line[56:58] + line[54:56] if line[20] in (6, 17) else b"\0\0\0\0"  # no fragment test
    return line[22:54] + ports


def select(bond, line, vlan_ck=0, rss=0):
    """bond_select_tx_member: the member's iface id, None (bond_no_member) or KEEP."""
    mode, algo, n = int(bond["mode"]), int(bond["algo"]), int(bond["n_members"])
    if mode == abi.BOND_MODE["ACTIVE_BACKUP"]:
        idx = int(bond["active_member"])
    elif mode == abi.BOND_MODE["LACP"]:
        if n == 0:
            return None
        if algo == abi.BOND_ALGO["RSS"] and (vlan_ck & abi.META_RSS_HASH):
            h = int(rss)
        elif algo in (abi.BOND_ALGO["RSS"], abi.BOND_ALGO["L2"], abi.BOND_ALGO["L3_L4"]):
            t = tuple_of(line, algo == abi.BOND_ALGO["L2"])
            if t is KEEP:
                return KEEP
            h = softrss_be(t)
        else:
            return None
        idx = int(bond["reta"][h % abi.BOND_RETA])
    else:
        return None
    return int(bond["members"][idx]) if idx < n else None


def apply(topo, result, meta, on=True):
    """bond_output over a pass's (lines, verdicts, iface stats): a packet at
    bond_output whose bond (Topology.bonds) selects a member leaves at
    port_output with the member as iface, the member's tx counters
    incremented (:227); everything else is left alone. -> (lines, verdicts,
    stats, members): members[i] = the member chosen for row i, 0 = none."""
    lines, v, st = result
    v, st = v.copy(), st.copy()
    members = np.zeros(len(v), dtype=np.uint16)
    if not on:
        return lines, v, st, members
    for i in np.flatnonzero(v["edge"] == E["bond_output"]):
        bond = topo.bonds.get(int(v["iface"][i]))
        if bond is None:
            continue
        m = select(bond, lines[i], int(meta["vlan_ck"][i]), int(meta["rss"][i]))
        if m is None or m is KEEP:
            continue
        v["edge"][i] = E["port_output"]
        v["iface"][i] = m
        st["tx_packets"][m] += 1
        st["tx_bytes"][m] += int(meta["pkt_len"][i])
        members[i] = m
    return lines, v, st, members


def expect(topo, frames, meta, lines_only=False, on=True):
    """(lines, verdicts, iface stats, members) of the kernel with the switch on."""
    return apply(topo, oracle.Oracle(topo).process(np.ascontiguousarray(frames), meta, lines_only), meta, on)
