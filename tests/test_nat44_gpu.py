# SPDX-License-Identifier: BSD-3-Clause
"""Static NAT44 in the kernel (gr_hip_nat44_set) against nat44_ref.expect():
verdicts, all 64 bytes of every line and the per-iface counters, on a context
of its own (the session's shared one never has NAT on)."""
import ctypes

import numpy as np
import pytest

import nat44_cases as C
import nat44_ref as R
import oracle
from golden_util import fresh_fastpath_state
from grout_amd import abi
from test_node_shim import mbufs_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    """(FastPath, its fresh_fastpath_state dict): a private context, closed at the end."""
    from grout_amd.fwd import FastPath
    fp = FastPath(0)
    yield fp, {}
    fp.close()


@pytest.fixture(scope="module")
def corpus():
    t, nh, rules = C.topology()
    fr, me, lab = C.batch()
    return t, rules, fr, me, lab


@pytest.fixture(scope="module")
def want_both(corpus):
    """expect() for the corpus batch with both steps on, per lines_only. Read-only."""
    t, rules, fr, me, _ = corpus
    return {lo: R.expect(t, rules, fr, me, lines_only=lo) for lo in (False, True)}


def run(fp, frames, meta, mode="full", prefix32=False):
    """One submit on a queue of its own; -> (lines, verdicts, iface stats).
    mode: full | lines_only | inplace | ptrs_inplace."""
    import torch
    dev = torch.device("cuda")
    n, stride = frames.shape
    d_in = torch.from_numpy(np.array(frames).reshape(-1)).to(dev)  # copies: the shared batches are read-only
    d_me = torch.from_numpy(np.array(meta).view(np.uint8)).to(dev)
    d_v = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
    ow = abi.PREFIX if prefix32 else abi.LINE
    d_out = torch.zeros(n * ow, dtype=torch.uint8, device=dev)
    q = fp.queue()
    try:
        torch.cuda.synchronize()
        q.stats(reset=True)
        if mode == "ptrs_inplace":
            ptrs = torch.from_numpy((d_in.data_ptr() + np.arange(n, dtype=np.uint64) * stride).view(np.int64)).to(dev)
            torch.cuda.synchronize()
            b = abi.Batch(ptrs.data_ptr(), None, d_me.data_ptr(), d_v.data_ptr(), n, 0, abi.LINE,
                          abi.BATCH_F_FRAME_PTRS)
            abi.check("gr_hip_fwd4_submit", fp.lib.gr_hip_fwd4_submit(q._h, ctypes.byref(b)))
        elif mode == "inplace":
            q.submit(d_in, d_in, d_me, d_v, n, in_stride=stride, out_stride=stride)
        else:
            q.submit(d_in, d_out, d_me, d_v, n, in_stride=stride, lines_only=mode == "lines_only", prefix32=prefix32)
        q.sync()
        st = q.stats(reset=True)
    finally:
        q.close()
    if mode in ("inplace", "ptrs_inplace"):
        after = d_in.cpu().numpy().reshape(n, stride)
        assert np.array_equal(after[:, abi.LINE:], frames[:, abi.LINE:])  # nothing past the line moved
        lines = after[:, :abi.LINE].copy()
    else:
        lines = d_out.cpu().numpy().reshape(n, ow).copy()
    return lines, d_v.cpu().numpy().view(abi.VERDICT_DT).copy(), st


def same(want, got, labels=None, stats=True):
    wl, wv, ws = want
    gl, gv, gs = got
    name = lambda i: labels[i] if labels else int(i)
    for f in ("edge", "domain", "iface", "nh"):
        bad = np.flatnonzero(wv[f] != gv[f])
        assert len(bad) == 0, (f, [(name(i), int(gv[f][i]), int(wv[f][i]), abi.EDGE_NAMES[wv["edge"][i]]) for i in bad[:8]])
    bad = np.flatnonzero((wl != gl).any(axis=1))
    assert len(bad) == 0, [(name(i), np.flatnonzero(wl[i] != gl[i]).tolist()) for i in bad[:8]]
    if stats:
        for f in ws.dtype.names:
            assert np.array_equal(ws[f], gs[f]), (f, np.flatnonzero(ws[f] != gs[f]).tolist())


@pytest.mark.parametrize("mode", ["full", "lines_only", "inplace", "ptrs_inplace"])
def test_corpus_both_steps(nat, corpus, want_both, mode):
    """The exception corpus plus a frame per NAT rule, both steps on."""
    fp, state = nat
    t, rules, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    fp.nat44_set(dnat=True, snat=True)
    assert fp.nat44_get() == 3
    try:
        got = run(fp, fr, me, mode)
    finally:
        fp.nat44_set()
    want = want_both[mode == "lines_only"]
    same(want, got, lab)
    v = got[1]
    assert ((v["domain"] & abi.VERDICT_DNAT) != 0).sum() > 30 and ((v["domain"] & abi.VERDICT_SNAT) != 0).sum() > 20


def test_out_of_line_snat_hits_keep_the_cpu_edge(nat, corpus):
    """A SNAT hit whose L4 checksum field lies past byte 63: ip_output_snat,
    no byte changed, as the plain oracle (each in a walk of its own)."""
    fp, state = nat
    t, rules, _fr, _me, _ = corpus
    rf, rm, lab = C.refused_batch()
    fresh_fastpath_state(fp, t, state)
    fp.nat44_set(dnat=True, snat=True)
    try:
        got = run(fp, rf, rm)
    finally:
        fp.nat44_set()
    want = oracle.Oracle(t).process(rf, rm)
    assert (want[1]["edge"] == abi.EDGE["ip_output_snat"]).all()
    same(want, got, lab, stats=False)


@pytest.mark.parametrize("dnat,snat", [(True, False), (False, True), (False, False)], ids=["dnat", "snat", "off"])
def test_corpus_one_step_or_none(nat, corpus, dnat, snat):
    """Each step alone; with the mask 0 (rules and translations still loaded)
    the plain oracle bit for bit."""
    fp, state = nat
    t, rules, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    fp.nat44_set(dnat=dnat, snat=snat)
    try:
        got = run(fp, fr, me)
    finally:
        fp.nat44_set()
    if not dnat and not snat:
        want = oracle.Oracle(t).process(fr, me)
        assert not (got[1]["domain"] & 0xC0).any()
    else:
        want = R.expect(t, rules, fr, me, dnat=dnat, snat=snat)
    same(want, got, lab)


@pytest.mark.parametrize("stats", [1, 0])
@pytest.mark.parametrize("ring", [2, 0])
def test_streams(nat, ring, stats):
    """Seeded streams (a ragged last tile, and 64 tiles): a third of the
    destinations DNATed, a third of the sources SNATed; the default ring
    geometry and another, with and without the kernel's counters."""
    fp, state = nat
    ts = C.stream_topology()
    fresh_fastpath_state(fp, ts, state)
    fp.nat44_set(dnat=True, snat=True)
    fp.tune("ring", ring)
    fp.tune("stats", stats)
    try:
        for n, seed in ((64 * 3 + 7, 0xA11), (4096, 0xA12)):
            fr, me = C.stream(n, seed)
            got = run(fp, fr, me)
            same(R.expect(ts, ts.snat44_static, fr, me), got, stats=bool(stats))
            if not stats:
                assert not got[2]["rx_packets"].any()
    finally:
        fp.tune("ring", 2)
        fp.tune("stats", 1)
        fp.nat44_set()


def test_rule_table(nat, corpus):
    """Rules added and deleted between submits: after each step the result is
    expect() with the rules then loaded; 700 rules on two ifaces whose home
    slots collide in their low bits (probing, and growth from 16 slots)."""
    fp, state = nat
    t, _rules, _fr, _me, _ = corpus
    fr, me = C.table_batch()
    fresh_fastpath_state(fp, t, state)
    fp.nat44_set(dnat=True, snat=True)
    cur = {(i, m): r for i, m, r in t.snat44_static}
    try:
        assert fp.lib.gr_hip_snat44_static_add(fp.h, C.SC.P3, fp._be(C.SRC), 1) == -17  # -EEXIST
        assert fp.lib.gr_hip_snat44_static_del(fp.h, C.SC.P3, fp._be("198.18.0.99")) == -2  # -ENOENT
        hits = []
        for want_rules in C.table_rule_sets():
            w = {(i, m): r for i, m, r in want_rules}
            if not w:
                fp.snat44_static_clear()
            else:
                for k in [k for k in cur if k not in w or w[k] != cur[k]]:
                    fp.snat44_static_del(k[0], k[1])
                    del cur[k]
                for k in [k for k in w if k not in cur]:
                    fp.snat44_static_add(k[0], k[1], w[k])
            cur = dict(w)
            got = run(fp, fr, me)
            same(R.expect(t, want_rules, fr, me), got)
            hits.append(int(((got[1]["domain"] & abi.VERDICT_SNAT) != 0).sum()))
        assert hits[3] == 0 and hits[6] == 0 and hits[0] == 1 and hits[1] == 3 and hits[4] > 90 and hits[5] < hits[4]
    finally:
        fp.nat44_set()
        fp.snat44_static_clear()
        for i, m, r in t.snat44_static:  # as loaded, for the tests after this one
            fp.snat44_static_add(i, m, r)


def test_prefix32_runs_without_nat(nat, corpus):
    """GR_HIP_BATCH_F_PREFIX32 with both steps on: today's output (the
    rewritten bytes lie past the 32 that leave the kernel)."""
    fp, state = nat
    t, rules, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    fp.nat44_set(dnat=True, snat=True)
    try:
        got = run(fp, fr, me, prefix32=True)
    finally:
        fp.nat44_set()
    wl, wv, ws = oracle.Oracle(t).process(fr, me)
    same((wl[:, :abi.PREFIX], wv, ws), got, lab)


def test_resident_kernel(nat, corpus, want_both):
    """One batch through the resident kernel (the node's frames handed over
    by address, rewritten in place), both steps on."""
    fp, state = nat
    t, rules, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    wl, wv, _ = want_both[True]  # the node sees the header lines only (a longer IPv4 header is punted)
    bufs, m = mbufs_for(fr, me)
    L = fp.lib
    abi.check("gr_hip_host_register", L.gr_hip_host_register(fp.h, bufs.ctypes.data, bufs.nbytes))
    q = None
    try:
        fp.nat44_set(dnat=True, snat=True)
        fp.tune("node_ptrs", 1)
        assert fp.tune("resident", 1) == 0
        l0 = fp.tune("resident_launches")
        q = fp.queue()
        q.node_start(m)
        got, _ns = q.node_finish()
        assert got is m and q.unfinished == 0
        assert fp.tune("resident_launches") > l0
    finally:
        fp.tune("resident", 0)
        fp.tune("node_ptrs", 0)
        fp.nat44_set()
        if q is not None:
            q.close()
        abi.check("gr_hip_host_unregister", L.gr_hip_host_unregister(fp.h, bufs.ctypes.data))
    name = lambda i: lab[i]
    punt = wv["edge"] == abi.EDGE["punt"]  # handed back as port_rx left them
    for f, w in (("edge", wv["edge"]), ("nh", wv["nh"]), ("iface", wv["iface"]),
                 ("domain", wv["domain"] & abi.VERDICT_DOMAIN_MASK)):
        bad = np.flatnonzero((m[f] != w) & ~punt)
        assert len(bad) == 0, (f, [(name(i), int(m[f][i]), int(w[i])) for i in bad[:8]])
    bad = np.flatnonzero((bufs[:, :abi.LINE] != wl).any(axis=1))
    assert len(bad) == 0, [(name(i), np.flatnonzero(bufs[i, :abi.LINE] != wl[i]).tolist()) for i in bad[:8]]
    assert np.array_equal(bufs[:, abi.LINE:], fr[:, abi.LINE:])
