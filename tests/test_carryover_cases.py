"""The CPU half of tests/test_gpu_carryover.py: every case of
tests/carryover_util.py is built and its preconditions are checked with the
oracle alone -- batch A differs from the checked batch B in each device-side
decision, the cut capacities cut, the shapes satisfy the inequalities of the
route they are meant to reach (the thresholds read from the sources, the
receive route from cfws_deserialize_pass_kernel, a pure host call)."""
import os

import numpy as np
import pytest

import carryover_util as U
import oracle as O
from coldforce_amd import workloads as W

K = U.code_constants()
DEFAULT_KNOBS = not any(k.startswith("CFWS_") and k != "CFWS_LIB" for k in os.environ)


def test_thresholds_are_the_ones_the_shapes_were_chosen_for():
    assert K["plan_block"] * K["self_scan_blocks"] + 1 == U.BIG_N          # one frame past the self-scan plans
    assert U.blocks(U.BIG_N, K["ser_single_block"]) == 129                 # the send's look-back: > 1 round of 64
    assert U.blocks(U.BIG_N, K["de_single_block"]) > 64
    assert U.blocks(2049, K["fused_block"]) == 2 and U.blocks(133_121, K["fused_block"]) == 66
    assert K["small_frames"] == 1024 and K["small_bytes"] == 4 << 20 and K["fused_avg_max"] == 512


def _ser(case):
    c = case
    tb, ta = c.expect("B")["total"], W.wire_layout(c.inputs("A"))[1]
    assert tb <= c.cap < ta and ta > tb                                    # A above the capacity, B below
    small = c.name.startswith(("ser_small", "ser_one"))     # one launch, no plan flag
    if not small:
        ok_b, ok_a = (U.inreg_ok(c.inputs(v), K["inreg_max"]) for v in "BA")
        assert ok_b.all() != ok_a.all()                                    # the plan's in-region flag flips
        for ok, style in ((ok_b, c.styles[0]), (ok_a, c.styles[1])):
            if not ok.all() and style not in ("mixed", "inreg_one_bad"):
                assert not ok.any()
        if c.styles[0] == "inreg_one_bad":
            assert (~ok_b).sum() == 1
    nb = U.blocks(c.n, K["plan_block"])
    if small:
        assert not c.pe and c.n <= K["small_frames"] and c.cap <= K["small_bytes"]
    else:
        assert c.n > K["small_frames"]
        assert (nb > K["self_scan_blocks"]) == c.name.startswith("ser_single")


def _de(case):
    c = case
    eb = c.expect("B")
    whole_a = c._oracle("A", c.wsize + c.align * c.n + 64)[3]
    assert whole_a > c.whole_b and whole_a > c.cap
    oom = eb["status"] == O.ERROR_OUT_OF_MEMORY
    if c.cut:
        assert c.cap < c.whole_b and oom.any() and eb["total"] == c.cap    # the capacity cuts
    else:
        assert c.whole_b <= c.cap and not oom.any() and eb["total"] == c.whole_b
    ia, ib = c.inputs("A"), c.inputs("B")
    for k in ("bad", "more"):                                              # invalid / incomplete frames elsewhere
        assert len(ib[k]) and len(ia[k]) and not set(ib[k]) & set(ia[k])
    inv = np.setdiff1d(ib["bad"], ib["more"])
    assert (eb["status"][inv] == O.ERROR_INVALID_FRAME).all()
    assert (eb["status"][ib["more"]] == O.PARSE_MORE_DATA).all()
    assert len(ia["wire"]) == len(ib["wire"]) == c.wsize + 16
    nb = U.blocks(c.n, K["plan_block"])
    want = None
    if c.name.startswith("de_small"):
        assert c.n <= K["small_frames"] and c.cap <= K["small_bytes"]
        want = "deserialize_small_kernel"
    elif c.name.startswith("de_fused"):
        assert c.n > K["small_frames"] and c.align >= 16 and c.wsize // c.n <= K["fused_avg_max"]
        want = "deserialize_plan_single_kernel<true>"
    else:
        assert c.n > K["small_frames"] and (c.align < 16 or c.flags)
        assert (nb > K["self_scan_blocks"]) == c.name.startswith("de_single")
        want = "xform_kernel<1>"
    if c.flags:
        ctl = eb["desc"]["opcode"] >= 8
        assert ctl.any() and (~ctl).any()
    if DEFAULT_KNOBS and not c.pe:
        assert c.route() == want


def _relay(case):
    c = case
    assert c.expect("B")["total"] <= c.cap < c.expect("A")["total"]
    st = c.expect("B")["status"]
    assert (st == O.ERROR_INVALID_FRAME).any() and st[-1] == O.PARSE_MORE_DATA
    assert c.expect("A")["status"][-1] != O.PARSE_MORE_DATA
    assert (U.blocks(c.n, K["plan_block"]) > K["self_scan_blocks"]) == (c.n == U.BIG_N)   # a scan_partials launch


def _h2ser(case):
    c = case
    assert c.expect("B")["total"] <= c.caps[1]
    assert W.wire_layout(c.inputs("A"))[1] > c.caps[0] and c.expect("A")["total"] > c.caps[1]
    assert c.n > K["small_frames"]


def _h2de(case):
    c = case
    eb, ea = c.expect("B"), c.expect("A")
    for v in "AB":
        assert len(c.inputs(v)["index"]) == U.H2_DATA_FRAMES
    assert ea["n_msg"] != eb["n_msg"]
    whole_a = c._oracle("A", len(c.inputs("A")["h2"]), None)["total"]
    assert whole_a > c.caps[1] >= eb["total"]
    oom = (eb["h2_status"] == O.ERROR_OUT_OF_MEMORY).any()
    assert oom == (c.mode == "general")
    if c.mode == "open":
        i = c.inputs("B")
        assert not i["h2"][int(i["index"][-1]) + 4] & 1 and eb["n_msg"] < i["messages"] < c.n
    else:
        assert eb["n_msg"] <= c.n
    assert (eb["h2_status"] != 0).any()


def _index(case):
    c = case
    eb, ea = c.expect("B"), c.expect("A")
    assert ea["total"] > c.cap > eb["total"]
    for e in (eb, ea):
        assert (e["counts"] > K["index_slots"]).any() and (e["counts"] == 0).any()
        assert (e["stop"] < 0).any() and (e["stop"] == O.PARSE_MORE_DATA).any() and (e["stop"] == 0).any()
    assert not np.array_equal(ea["counts"], eb["counts"])


def _keys(case):
    c = case
    assert c.inputs("A").sum() > c.inputs("B").sum()
    assert (U.blocks(c.n, 4096) > K["self_scan_blocks"]) == (c.name == "keys_scan_launch")


CHECKS = dict(ser=_ser, de=_de, relay=_relay, h2ser=_h2ser, h2de=_h2de, index=_index, keys=_keys)


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_case_preconditions(name):
    case = U.cases()[name]
    try:
        CHECKS[case.kind](case)
    finally:
        case.release()


def test_scripts_cover_every_entry_point():
    names = [n for n, _ in U.SEQUENCE]
    assert len(names) >= 16 and set(names) <= set(U.CASE_NAMES)
    kinds = {U.cases()[n].kind for n in names}
    assert kinds == set(CHECKS)
    ns = [U.cases()[n].n for n in names]
    ups = sum(b > a for a, b in zip(ns, ns[1:]))
    downs = sum(b < a for a, b in zip(ns, ns[1:]))
    assert ups >= 5 and downs >= 5 and max(ns) == U.BIG_N and min(ns) == 1
    for n in U.GRAPH_CASES:
        assert U.cases()[n].graph and not getattr(U.cases()[n], "pe", False)


def test_count_handoff_streams():
    for k, (m, general) in enumerate([(7, False), (3000, True), (0, False), (7, True), (1, False), (2999, True)]):
        c = U.H2CountCase(f"handoff_{k}", m, general)
        e = c.expect("B")
        assert e["n_msg"] == m and c.n == (m + general if m else 2)
        assert (e["h2_status"] == O.ERROR_OUT_OF_MEMORY).any() == general
