# SPDX-License-Identifier: BSD-3-Clause
"""bond_output in the kernel (gr_hip_bond_output_set) against bond_ref:
verdicts, every byte of every line and the per-iface counters, on a context
of its own (the session's shared one never has the switch on)."""

import numpy as np
import pytest

import bond_cases as C
import bond_ref as R
import nat44_ref
import oracle
from golden_util import fresh_fastpath_state
from grout_amd import abi
from test_nat44_gpu import run, same
from test_node_shim import mbufs_for

pytestmark = pytest.mark.gpu
E = abi.EDGE


@pytest.fixture(scope="module")
def bond():
    """(FastPath, its fresh_fastpath_state dict): a private context, closed at the end."""
    from grout_amd.fwd import FastPath
    fp = FastPath(0)
    yield fp, {}
    fp.close()


@pytest.fixture(scope="module")
def corpus():
    t, nh = C.topology()
    fr, me, lab = C.batch()
    return t, nh, fr, me, lab


@pytest.fixture(scope="module")
def want_on(corpus):
    """bond_ref.expect() for the corpus batch, per lines_only. Read-only."""
    t, _nh, fr, me, _ = corpus
    return {lo: R.expect(t, fr, me, lines_only=lo) for lo in (False, True)}


def run_on(fp, frames, meta, mode="full", prefix32=False):
    fp.bond_output_set(True)
    try:
        return run(fp, frames, meta, mode, prefix32)
    finally:
        fp.bond_output_set(False)


@pytest.mark.parametrize("mode", ["full", "lines_only", "inplace", "ptrs_inplace", "prefix32"])
def test_corpus_on(bond, corpus, want_on, mode):
    """The exception corpus plus the bond frames, the switch on."""
    fp, state = bond
    t, _nh, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    assert fp.bond_output_get() == 0
    got = run_on(fp, fr, me, "full" if mode == "prefix32" else mode, prefix32=mode == "prefix32")
    wl, wv, ws, members = want_on[mode == "lines_only"]
    same((wl[:, :abi.PREFIX] if mode == "prefix32" else wl, wv, ws), got, lab)
    hit = C.members_hit(t, (got[0], got[1], got[2], np.where(got[1]["edge"] == E["port_output"], members, 0)))
    for b in C.LACP3:
        assert hit[b] == set(C.MEMBERS[b])
    assert (members != 0).sum() > 300 and ((wv["edge"] == E["bond_output"]).sum()) > 100


def test_corpus_off_and_after_on_off(bond, corpus):
    """Off (bonds loaded): the plain oracle, bond_output edges included; and
    again after the switch went on and off."""
    fp, state = bond
    t, _nh, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    want = oracle.Oracle(t).process(fr, me)
    assert (want[1]["edge"] == E["bond_output"]).sum() > 400
    same(want, run(fp, fr, me), lab)
    fp.bond_output_set(True)
    assert fp.bond_output_get() == 1
    fp.bond_output_set(False)
    assert fp.bond_output_get() == 0
    same(want, run(fp, fr, me), lab)
    same(want, run(fp, fr, me, "inplace"), lab)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 64 * 300])
def test_batch_sizes(bond, corpus, n):
    fp, state = bond
    t = corpus[0]
    fresh_fastpath_state(fp, t, state)
    fr, me = C.cycled(n)
    want = R.expect(t, fr, me)
    same(want[:3], run_on(fp, fr, me))


def test_member_counters_add_up(bond, corpus):
    """Per bond: its members' tx counters = its own minus the packets that kept the bond edge."""
    fp, state = bond
    t, _nh, fr, me, _ = corpus
    fresh_fastpath_state(fp, t, state)
    _l, v, st = run_on(fp, fr, me)
    for b, mem in C.MEMBERS.items():
        kept = (v["edge"] == E["bond_output"]) & (v["iface"] == b)
        assert st["tx_packets"][mem].sum() == st["tx_packets"][b] - kept.sum(), b
        assert st["tx_bytes"][mem].sum() == st["tx_bytes"][b] - me["pkt_len"][kept].sum(), b
    assert st["tx_packets"][C.MEMBERS[C.B_L34]].sum() > 60


@pytest.mark.parametrize("stats", [1, 0])
@pytest.mark.parametrize("ring", [2, 0])
def test_ring_geometries_and_counters_off(bond, corpus, want_on, ring, stats):
    fp, state = bond
    t, _nh, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    fp.tune("ring", ring)
    fp.tune("stats", stats)
    try:
        got = run_on(fp, fr, me)
    finally:
        fp.tune("ring", 2)
        fp.tune("stats", 1)
    same(want_on[False][:3], got, lab, stats=bool(stats))
    if not stats:
        assert not got[2]["tx_packets"].any()


def test_live_change(bond, corpus):
    """An active-backup bond's active member and an LACP bond's redirection
    table change between two submits: each submit follows the table it saw."""
    import copy
    fp, state = bond
    t, _nh, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    first = run_on(fp, fr, me)
    same(R.expect(t, fr, me)[:3], first, lab)
    t2 = copy.deepcopy(t)
    t2.add_bond(C.B_AB, "ACTIVE_BACKUP", "L3_L4", C.MEMBERS[C.B_AB], primary=C.MEMBERS[C.B_AB][0])
    t2.add_bond(C.B_L34, "LACP", "L3_L4", C.MEMBERS[C.B_L34], active=C.MEMBERS[C.B_L34][2:])
    try:
        fp.bond_set(C.B_AB, t2.bonds[C.B_AB])
        fp.bond_set(C.B_L34, t2.bonds[C.B_L34])
        second = run_on(fp, fr, me)
    finally:
        fp.bond_set(C.B_AB, t.bonds[C.B_AB])
        fp.bond_set(C.B_L34, t.bonds[C.B_L34])
    want2 = R.expect(t2, fr, me)
    same(want2[:3], second, lab)
    assert set(second[1]["iface"][want2[3] != 0]) & set(C.MEMBERS[C.B_L34]) == {C.MEMBERS[C.B_L34][2]}
    assert (first[1]["iface"] != second[1]["iface"]).sum() > 50
    same(R.expect(t, fr, me)[:3], run_on(fp, fr, me), lab)  # and back


def test_argument_checks(bond, corpus):
    fp, state = bond
    t = corpus[0]
    fresh_fastpath_state(fp, t, state)
    L, h = fp.lib, fp.h
    b = np.array(t.bonds[C.B_L34]).reshape(1).copy()
    ok = lambda x: L.gr_hip_bond_set(h, C.B_L34, x.ctypes.data)
    assert L.gr_hip_bond_set(h, C.MEMBERS[C.B_L34][0], b.ctypes.data) == -22  # a PORT iface
    assert L.gr_hip_bond_set(h, 900, b.ctypes.data) == -22  # no such iface
    assert L.gr_hip_bond_set(h, C.B_L34, None) == -22
    bad = b.copy()
    bad["n_members"] = 9
    assert ok(bad) == -22
    bad = b.copy()
    bad["members"][0, 1] = C.B_RSS  # a member that is a bond
    assert ok(bad) == -22
    bad["members"][0, 1] = 901  # or missing
    assert ok(bad) == -22
    assert L.gr_hip_bond_del(h, 900) == -2 and L.gr_hip_bond_del(h, C.MEMBERS[C.B_L34][0]) == -2  # -ENOENT
    assert ok(b) == 0
    fp.bond_del(C.B_L34)
    assert L.gr_hip_bond_del(h, C.B_L34) == -2
    try:  # without its entry the bond's packets are the CPU node's again
        fr, me, lab = corpus[2:]
        got = run_on(fp, fr, me)
        at = (got[1]["edge"] == E["bond_output"]) & (got[1]["iface"] == C.B_L34)
        assert at.sum() > 100 and not np.isin(got[1]["iface"], C.MEMBERS[C.B_L34]).any()
    finally:
        fp.bond_set(C.B_L34, t.bonds[C.B_L34])


def test_nat_rewrites_come_first(bond, corpus):
    """With static NAT on: a DNATed packet towards a bond and a SNATed one
    leaving through one hash with the rewritten addresses."""
    fp, state = bond
    t, _nh, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    fp.nat44_set(dnat=True, snat=True)
    try:
        got = run_on(fp, fr, me)
    finally:
        fp.nat44_set()
    nat = nat44_ref.expect(t, t.snat44_static, fr, me)
    want = R.apply(t, nat, me)
    same(want[:3], got, lab)
    by = {l: i for i, l in enumerate(lab)}
    d, s = by["dnat to l34 tcp"], by["snat tcp"]
    assert want[1]["domain"][d] & abi.VERDICT_DNAT and want[3][d] in C.MEMBERS[C.B_L34]
    assert want[1]["domain"][s] & abi.VERDICT_SNAT and want[3][s] in C.MEMBERS[C.B_SNAT]
    # the choice is the rewritten tuple's: over these flows it differs from the original tuple's somewhere
    rows = [i for l, i in by.items() if l.startswith("dnat to l34") or (l.startswith("snat ") and want[3][i])]
    orig = [R.select(t.bonds[C.B_L34 if lab[i].startswith("dnat") else C.B_SNAT], fr[i, :64]) for i in rows]
    assert any(o != int(want[3][i]) for o, i in zip(orig, rows))


def test_resident_kernel_vlan_over_bond(bond, corpus, want_on):
    """One walk through the resident kernel and gr_hip_node_*: a packet
    leaving through the VLAN sub-interface of a bond ends at port_output with
    the member as iface and the sub-interface's vlan_id."""
    fp, state = bond
    t, _nh, fr, me, lab = corpus
    fresh_fastpath_state(fp, t, state)
    rows = sum(([i for i, l in enumerate(lab) if l.startswith(p)][:21] for p in ("vlan/l34 ", "l34 ", "ab ")), [])
    fr, me = np.ascontiguousarray(fr[rows]), np.ascontiguousarray(me[rows])
    me["vlan_ck"] &= 0x7FFF  # the views carry no ol_flags (gr_hip_node_append_mbufs does)
    labs = [lab[i] for i in rows]
    wl, wv, _ws, members = R.expect(t, fr, me, lines_only=True)
    bufs, m = mbufs_for(fr, me)
    L = fp.lib
    abi.check("gr_hip_host_register", L.gr_hip_host_register(fp.h, bufs.ctypes.data, bufs.nbytes))
    q = None
    try:
        fp.bond_output_set(True)
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
        fp.bond_output_set(False)
        if q is not None:
            q.close()
        abi.check("gr_hip_host_unregister", L.gr_hip_host_unregister(fp.h, bufs.ctypes.data))
    for f in ("edge", "nh", "iface"):
        bad = np.flatnonzero(m[f] != wv[f])
        assert len(bad) == 0, (f, [(labs[i], int(m[f][i]), int(wv[f][i])) for i in bad[:8]])
    assert np.array_equal(bufs[:, :abi.LINE], wl)
    i = labs.index("vlan/l34 tcp")
    assert m["edge"][i] == E["port_output"] and m["iface"][i] == members[i] and m["iface"][i] in C.MEMBERS[C.B_L34]
    assert m["vlan_id"][i] == 300 and m["vlan_id"][labs.index("l34 tcp")] == 0
    assert m["edge"][labs.index("l34 udp ihl 12")] == E["bond_output"]


def test_differential_fuzz(bond, corpus):
    """200 seeds x 256 random packets towards random bonds against bond_ref."""
    fp, state = bond
    t = corpus[0]
    fresh_fastpath_state(fp, t, state)
    hit = {}
    for s0 in range(0, 200, 25):
        parts = [C.fuzz(s) for s in range(s0, s0 + 25)]
        fr, me = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        want = R.expect(t, fr, me)
        same(want[:3], run_on(fp, fr, me))
        for b, mem in C.members_hit(t, want).items():
            hit.setdefault(b, set()).update(mem)
    assert all(hit.get(b) for b in C.LACP3)
