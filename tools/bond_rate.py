#!/usr/bin/env python3
# SPDX-License-Identifier: BSD-3-Clause
"""Rate of the kernel's bond_output on the full-view workload (a measurement,
no threshold): one device-resident stream of --batch 64-byte packets over the
1M-route FIB, every nexthop leaving through one of three bonds of three member
ports each, on the same buffers:

  off     the switch off: every packet leaves at bond_output for the CPU node;
  l3_l4   LACP, algo L3_L4: a 12-byte tuple hashed per packet;
  l2      LACP, algo L2: the 6 bytes of the destination MAC;
  rss     LACP, algo RSS, every packet flagged RTE_MBUF_F_RX_RSS_HASH: no hash;
  rss_nf  the same without the flag: falls through to L3_L4;
  ab      active-backup: no hash, no table read.

--plain adds bench.py's own topology (no bond) as a first leg. Prints one JSON
line: per leg the kernel time per launch (HIP events), the wall-clock Mpps over
--steps submits and the share of packets at port_output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--plain", action="store_true")
    a = ap.parse_args()

    import torch

    from grout_amd import abi
    from grout_amd import synth as S
    from grout_amd import topology as T
    from grout_amd.fwd import FastPath, shared_stream

    dev = torch.device("cuda", 0)
    n = a.batch
    base = T.config_fullview()
    frames, meta = S.stream(n, S.SEED_FULLVIEW, routes=base.route_array())
    d_in = torch.from_numpy(frames.reshape(-1)).to(dev)
    d_out = torch.empty(n * abi.LINE, dtype=torch.uint8, device=dev)
    d_v = torch.empty(n * 8, dtype=torch.uint8, device=dev)
    flagged = meta.copy()
    flagged["vlan_ck"] |= abi.META_RSS_HASH
    d_me = {False: torch.from_numpy(meta.view(np.uint8)).to(dev), True: torch.from_numpy(flagged.view(np.uint8)).to(dev)}

    def measure(fp, name, flag=False):
        q = fp.queue(shared_stream(dev))
        step = lambda: q.submit(d_in, d_out, d_me[flag], d_v, n)
        fp.tune("untimed", 1)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.settle_ms / 1e3:  # the clock ramps up after idle
            for _ in range(4):
                step()
            torch.cuda.synchronize()
        fp.tune("untimed", 0)
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        q.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        q.sync()
        ms, cnt = q.kernel_ms(a.steps)
        v = d_v.cpu().numpy().view(abi.VERDICT_DT)
        edges = np.bincount(v["edge"], minlength=abi.E_COUNT)
        out = dict(leg=name, kernel_ms=round(ms / max(cnt, 1), 4), mpps_kernel=round(n / (ms / max(cnt, 1)) / 1e3, 1),
                   mpps_wall=round(n * a.steps / el / 1e6, 1), timed_launches=cnt,
                   port_output=float(edges[abi.EDGE["port_output"]] / n),
                   bond_output=float(edges[abi.EDGE["bond_output"]] / n),
                   members=int(len(np.unique(v["iface"][v["edge"] == abi.EDGE["port_output"]]))))
        print(json.dumps(out), file=sys.stderr, flush=True)
        q.close()
        return out

    res = []
    if a.plain:
        fp = FastPath(0)
        fp.load(base)
        res.append(measure(fp, "plain"))
        fp.close()

    # every egress port becomes a bond over three new member ports
    t = T.config_fullview()
    bond_of, members = {}, {}
    for k, p in enumerate(T.PORT_IFACE[1:]):
        b = 100 + k
        members[b] = [200 + 3 * k + j for j in range(3)]
        for m in members[b]:
            t.add_port(m, m, "02:00:00:00:01:%02x" % (m & 255))
        t.add_iface(b, "BOND", mac="02:00:00:00:02:%02x" % b)
        bond_of[p] = b
    nh = t.nh[1:t.n_nh + 1]
    for p, b in bond_of.items():
        nh["iface_id"][(nh["iface_id"] == p) & ((nh["flags"] & abi.NH_F_LOCAL) == 0)] = b
    legs = [("off", "LACP", "L3_L4", False, False), ("l3_l4", "LACP", "L3_L4", True, False),
            ("l2", "LACP", "L2", True, False), ("rss", "LACP", "RSS", True, True),
            ("rss_nf", "LACP", "RSS", True, False), ("ab", "ACTIVE_BACKUP", "L3_L4", True, False)]
    for b in members:
        t.add_bond(b, "LACP", "L3_L4", members[b])
    fp = FastPath(0)
    fp.load(t)
    for name, mode, algo, on, flag in legs:
        for b in members:
            fp.bond_set(b, t.add_bond(b, mode, algo, members[b]))
        fp.bond_output_set(on)
        res.append(measure(fp, name, flag))
    fp.close()
    print(json.dumps(dict(tool="bond_rate", batch=n, steps=a.steps, toeplitz=os.environ.get("BOND_FORM", "table"),
                          legs=res)))


if __name__ == "__main__":
    main()
