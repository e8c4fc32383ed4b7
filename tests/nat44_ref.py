# SPDX-License-Identifier: BSD-3-Clause
"""Reference for the kernel's static NAT44 (gr_hip_nat44_set): a numpy
restatement of grout's two functions, composed with the unchanged oracle.

* fixup32: fixup_checksum_32 (modules/policy/datapath/nat_datapath.h:33-46).
* rewrite: the body of dnat44_static_process (modules/policy/datapath/
  dnat44_static.c:20-89) / snat44_static_process (snat44_static.c:10-54) on
  the 64-byte header line the kernel sees.
* expect: what the kernel must give for a batch, from three oracle passes.

Addresses are host-order ints, as in grout_amd.topology.
"""
import copy

import numpy as np

import oracle
from grout_amd import abi

E = abi.EDGE
STATIC, DYNAMIC = abi.IFACE_F_SNAT_STATIC, abi.IFACE_F_SNAT_DYNAMIC


def fixup32(ck, old, new):
    """fixup_checksum_32(old_cksum, old_addr, new_addr): every value as the
    CPU loads it from the packet (a little-endian load of network-order bytes;
    the one's complement sum is byte-order independent, RFC 1071)."""
    s = ~ck & 0xFFFF
    s += (~old & 0xFFFF) + (new & 0xFFFF)
    s += ((~old & 0xFFFFFFFF) >> 16) + (new >> 16)
    s = (s >> 16) + (s & 0xFFFF)
    s += s >> 16
    return ~s & 0xFFFF


def l4_cksum_off(line):
    """Offset in the frame of the L4 checksum field the NAT nodes fix up, None
    when they fix none (not a first fragment, neither TCP nor UDP)."""
    ihl = int(line[14]) & 0xF
    if ((int(line[20]) & 0x1F) << 8 | int(line[21])) != 0:  # fragment_offset & RTE_IPV4_HDR_OFFSET_MASK
        return None
    if line[23] == 6:
        return 14 + 4 * ihl + 16  # rte_tcp_hdr.cksum
    if line[23] == 17:
        return 14 + 4 * ihl + 6  # rte_udp_hdr.dgram_cksum
    return None


def in_line(line):
    """The checksum field to fix lies wholly inside bytes 0-63 (or there is none)."""
    off = l4_cksum_off(line)
    return off is None or off + 2 <= abi.LINE


def _le(b):
    return int.from_bytes(bytes(b), "little")


def rewrite_row(line, which, replace):
    """Rewrite the destination ("dst") or source ("src") of one line in place.
    Returns False, leaving the line alone, when the L4 checksum field lies
    outside the line (the packet stays with the CPU node)."""
    if not in_line(line):
        return False
    a = 30 if which == "dst" else 26
    old = _le(line[a:a + 4])
    new = _le(int(replace).to_bytes(4, "big"))
    line[24:26] = np.frombuffer(fixup32(_le(line[24:26]), old, new).to_bytes(2, "little"), np.uint8)
    off = l4_cksum_off(line)
    if off is not None:
        ck = _le(line[off:off + 2])
        if line[23] == 6 or ck != 0:
            ck = fixup32(ck, old, new)
            if line[23] == 17 and ck == 0:
                ck = 0xFFFF  # RFC 768
            line[off:off + 2] = np.frombuffer(ck.to_bytes(2, "little"), np.uint8)
    line[a:a + 4] = np.frombuffer(int(replace).to_bytes(4, "big"), np.uint8)
    return True


def rewrite(lines, which, replace):
    """rewrite_row over rows; replace: one address per row. -> bool per row."""
    return np.array([rewrite_row(lines[i], which, replace[i]) for i in range(len(lines))], dtype=bool)


def static_only(topo):
    """ifaces whose egress runs the static SNAT lookup alone (ip_output.c:112)."""
    f = topo.ifaces["flags"]
    return set(int(i) for i in topo.ifaces["id"][(topo.ifaces["id"] != 0) & ((f & STATIC) != 0) & ((f & DYNAMIC) == 0)])


def expect(topo, rules, frames, meta, lines_only=False, dnat=True, snat=True):
    """(lines, verdicts, iface stats) of the kernel with the DNAT / SNAT steps
    on, for the whole batch (walk composition is the oracle's).

    rules: [(iface_id, match, replace)]. Raises where a second oracle pass is
    not dnat44_static's semantics, rather than approximate.
    """
    frames = np.ascontiguousarray(frames)
    n = len(meta)
    so = static_only(topo)
    topo0 = copy.deepcopy(topo)
    for i in so:
        topo0.ifaces[i]["flags"] &= 0xFFFF ^ STATIC
    o0, o1 = oracle.Oracle(topo0), oracle.Oracle(topo)
    rule = {(int(i), int(m)): int(r) for i, m, r in rules}

    # D rows: at dnat44_static, checksum field in line
    d_rows = np.zeros(n, dtype=bool)
    frames2 = frames.copy()
    if dnat:
        _, v_a, _ = o0.process(frames, meta, lines_only)
        for i in np.flatnonzero(v_a["edge"] == E["dnat44_static"]):
            nh = topo.nh[int(v_a["nh"][i])]
            assert nh["type"] == abi.NH_T["DNAT"]
            d_rows[i] = rewrite_row(frames2[i, :abi.LINE], "dst", int(nh["ipv4"]))

    # S rows: at ip_output_snat of a static-only iface, a rule for the source
    s_rows = {}
    if snat:
        out_b, v_b, _ = o1.process(frames2, meta, lines_only)
        for i in np.flatnonzero(v_b["edge"] == E["ip_output_snat"]):
            if int(v_b["iface"][i]) not in so:
                continue
            r = rule.get((int(v_b["iface"][i]), int.from_bytes(bytes(out_b[i, 26:30]), "big")))
            if r is None:
                continue
            if not in_line(out_b[i]):
                raise ValueError(f"row {i}: SNAT hit with its checksum field outside the line")
            s_rows[int(i)] = r

    out, v, st = (o0 if snat else o1).process(frames2, meta, lines_only)
    for i in np.flatnonzero(d_rows):
        if v["edge"][i] == E["ip_input_local_ct"]:
            raise ValueError(f"row {i}: DNATed packet at ip_input_local_ct (dnat44_static's LOCAL is ip_input_local)")
        if v["nh"][i] != 0 and topo.nh[int(v["nh"][i])]["type"] != abi.NH_T["L3"]:
            raise ValueError(f"row {i}: DNATed packet resolves to a nexthop that is not L3")
        if v["nh"][i] == 0 and v["edge"][i] != E["ip_error_dest_unreach"]:
            raise ValueError(f"row {i}: DNATed packet without a nexthop at edge {v['edge'][i]}")
    for i, r in s_rows.items():
        assert rewrite_row(out[i], "src", r)
    v = v.copy()
    v["domain"][d_rows] |= abi.VERDICT_DNAT
    v["domain"][list(s_rows)] |= abi.VERDICT_SNAT
    return out, v, st
