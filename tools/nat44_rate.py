#!/usr/bin/env python3
# SPDX-License-Identifier: BSD-3-Clause
"""Rate of the kernel's static NAT44 steps on the full-view workload (a
measurement, no threshold): one device-resident stream of --batch 64-byte
packets over the 1M-route FIB, three legs on the same buffers:

  off   NAT off on the plain full-view topology (bench.py's workload);
  dnat  every packet's destination is one of --dnat DNAT /32s whose translated
        address is a full-view destination (a second FIB gather per packet);
  snat  the full-view stream towards ports flagged SNAT_STATIC, every source
        one of --rules static rules (a table probe and a source rewrite per
        packet; without the step every one of these packets leaves to the CPU).

Prints one JSON line: per leg the wall-clock Mpps over --steps submits, the
kernel time per launch (HIP events) and the share of packets that carry the
verdict flag.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ip_checksums(frames):
    """Recompute the IPv4 header checksum (IHL 5) of every frame in place."""
    w = frames[:, 14:34].astype(np.uint32)
    w[:, 10:12] = 0
    s = (w[:, 0::2] << 8 | w[:, 1::2]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    c = ~s & 0xFFFF
    frames[:, 24] = c >> 8
    frames[:, 25] = c & 0xFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dnat", type=int, default=16384, help="DNAT /32s (10.68.0.0 on)")
    ap.add_argument("--rules", type=int, default=1024, help="SNAT sources with a rule on each port")
    ap.add_argument("--settle-ms", type=float, default=100.0)
    a = ap.parse_args()

    import torch

    from grout_amd import abi
    from grout_amd import synth as S
    from grout_amd import topology as T
    from grout_amd.fwd import FastPath, shared_stream

    dev = torch.device("cuda", 0)
    n = a.batch
    rng = np.random.default_rng(0x4E41)
    base = T.config_fullview()
    frames, meta = S.stream(n, S.SEED_FULLVIEW, routes=base.route_array())

    def leg(name, topo, fr, mask, flag):
        fp = FastPath(0)
        fp.load(topo)
        fp.nat44_set(dnat=bool(mask & 1), snat=bool(mask & 2))
        q = fp.queue(shared_stream(dev))
        d_in = torch.from_numpy(fr.reshape(-1)).to(dev)
        d_me = torch.from_numpy(meta.view(np.uint8)).to(dev)
        d_out = torch.empty(n * abi.LINE, dtype=torch.uint8, device=dev)
        d_v = torch.empty(n * 8, dtype=torch.uint8, device=dev)
        step = lambda: q.submit(d_in, d_out, d_me, d_v, n)
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
        out = dict(leg=name, mpps_wall=round(n * a.steps / el / 1e6, 1), kernel_ms=round(ms / max(cnt, 1), 4),
                   mpps_kernel=round(n / (ms / max(cnt, 1)) / 1e3, 1), timed_launches=cnt,
                   flagged=float(((v["domain"] & flag) != 0).mean()) if flag else 0.0,
                   port_output=float(edges[abi.EDGE["port_output"]] / n))
        print(json.dumps(out), file=sys.stderr, flush=True)
        q.close()
        fp.close()
        del d_in, d_me, d_out, d_v
        return out

    res = [leg("off", base, frames, 0, 0)]

    # dnat: --dnat /32s, each translated to a destination drawn from the stream
    t = T.config_fullview()
    first = t.n_nh + 1
    repl = frames[rng.integers(0, n, a.dnat), 30:34]
    match0 = T.ip4("10.68.0.0")
    routes = np.zeros(a.dnat, dtype=abi.ROUTE_DT)
    for j in range(a.dnat):
        t.add_nexthop(T.PORT_IFACE[0], ipv4=int.from_bytes(bytes(repl[j]), "big"), nh_type="DNAT", slot=first + j)
    routes["ip"], routes["prefixlen"], routes["vrf_id"] = match0 + np.arange(a.dnat), 32, T.VRF_MAIN
    routes["nh"] = first + np.arange(a.dnat)
    t.add_routes(routes)
    t.fibs[T.VRF_MAIN] = (t.fibs[T.VRF_MAIN][0] + a.dnat, t.fibs[T.VRF_MAIN][1])
    fr = frames.copy()
    pick = (match0 + rng.integers(0, a.dnat, n)).astype(">u4")
    fr[:, 30:34] = pick.view(np.uint8).reshape(n, 4)
    ip_checksums(fr)
    res.append(leg("dnat", t, fr, abi.NAT44_DNAT_STATIC, abi.VERDICT_DNAT))
    del fr, t

    # snat: every egress port SNAT_STATIC, every source one with a rule
    t = T.config_fullview()
    src0 = T.ip4("198.18.0.0")
    for p in T.PORT_IFACE[1:]:
        t.ifaces[p]["flags"] |= abi.IFACE_F_SNAT_STATIC
        for s in range(a.rules):
            t.add_snat44_static(p, src0 + s, T.ip4("203.0.0.0") + (p << 16) + s)
    fr = frames.copy()
    fr[:, 26:30] = (src0 + rng.integers(0, a.rules, n)).astype(">u4").view(np.uint8).reshape(n, 4)
    ip_checksums(fr)
    res.append(leg("snat", t, fr, abi.NAT44_SNAT_STATIC, abi.VERDICT_SNAT))
    print(json.dumps(dict(tool="nat44_rate", batch=n, steps=a.steps, dnat_routes=a.dnat, snat_rules=a.rules * 3,
                          legs=res)))


if __name__ == "__main__":
    main()
