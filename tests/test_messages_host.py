"""Message and control tables of received frames on the host
(cfws_messages_from_frames, include/cfws.h).

* the model (tests/messages_util.py, a per-frame loop written from the rule
  in the header) equals the table config 3's generator keeps of its own batch;
* cfws_messages_from_frames equals the model on the fixed cases (at the
  capacities 0, total - 1 and total, a sentinel behind each) and on seeded
  random tables with and without connections;
* the record is 32 bytes and the symbols are exported;
* the walk, built with -fsanitize=address,undefined into a stand-alone
  program, over exact-size heap arrays.

The device form: tests/test_gpu_messages.py.
"""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import messages_util as U
from conftest import ROOT

from coldforce_amd import cfws
from coldforce_amd import workloads as W


def same(got, exp, what=""):
    """(msgs, conn_first_msg, control) against the model's, whole."""
    assert got[0].tobytes() == exp[0].tobytes(), what
    assert (got[1] is None) == (exp[1] is None), what
    if exp[1] is not None:
        assert np.array_equal(got[1], exp[1]), what
    assert np.array_equal(got[2], exp[2]), what
    assert (got[3], got[4]) == (len(exp[0]), len(exp[2])), what


@pytest.fixture(scope="module")
def zipf():
    d, messages = W.zipf_batch(1 << 20, ping_every=3, max_messages=300)
    # payload_off as CFWS_DESERIALIZE_REASSEMBLE lays the arena out: the data
    # frames back to back in frame order, then the control frames
    ctl = d["opcode"] >= 8
    sizes = d["payload_size"].astype(np.uint64)
    data_off = np.cumsum(np.where(ctl, 0, sizes)) - np.where(ctl, 0, sizes)
    ctl_off = int(sizes[~ctl].sum()) + np.cumsum(np.where(ctl, sizes, 0)) - np.where(ctl, sizes, 0)
    r = d.copy()
    r["payload_off"] = np.where(ctl, ctl_off, data_off)
    return r, messages


def test_model_equals_the_generators_table(zipf):
    d, messages = zipf
    assert messages["pings"] > 5 and (messages["n_frames"] > 2).sum() > 5
    msgs, _, control = U.expect_messages(d)
    assert len(msgs) == len(messages["off"])
    assert np.array_equal(msgs["payload_off"], messages["off"])
    assert np.array_equal(msgs["payload_size"], messages["len"])
    assert np.array_equal(msgs["opcode"], messages["opcode"])
    assert np.array_equal(msgs["first_frame"], messages["first_frame"])
    assert (msgs["flags"] == U.FINAL).all()
    for m, (a, k) in enumerate(zip(messages["first_frame"], messages["n_frames"])):
        assert msgs["n_fragments"][m] == int((d["opcode"][a:a + k] < 8).sum())
    assert np.array_equal(control, np.flatnonzero(d["opcode"] == 9))
    assert not msgs["conn"].any() and not msgs["zero"].any()


def test_host_walk_equals_model_on_generated_batch(zipf):
    d, _ = zipf
    same(cfws.messages_from_frames(d), U.expect_messages(d))


@pytest.mark.parametrize("name", sorted(U.fixed_cases()))
def test_host_walk_fixed_cases(name):
    d, st, cf = U.fixed_cases()[name]
    exp = U.expect_messages(d, st, cf)
    same(cfws.messages_from_frames(d, st, cf), exp, name)
    # clamped capacities: totals unclamped, a sentinel behind each capacity
    L = cfws.lib()
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    cfa = None if cf is None else np.ascontiguousarray(cf, np.uint64)
    for mcap in U.capacities(len(exp[0])):
        for ccap in U.capacities(len(exp[2])):
            msgs = np.full((mcap + 2) * 32, 0xEE, np.uint8)
            control = np.full(ccap + 2, 0xEEEEEEEE, np.uint32)
            cfm = np.full((0 if cf is None else len(cf)) + 2, 0xEEEEEEEEEEEEEEEE, np.uint64)
            nc = ctypes.c_uint64(77)
            m = L.cfws_messages_from_frames(ptr(d), ptr(st), len(d), None if cf is None else cfa.ctypes.data,
                                            0 if cf is None else len(cf), msgs.ctypes.data, mcap,
                                            cfm.ctypes.data, control.ctypes.data, ccap, ctypes.byref(nc))
            assert (m, nc.value) == (len(exp[0]), len(exp[2])), (name, mcap, ccap)
            wm, wc = min(mcap, m), min(ccap, nc.value)
            assert msgs[:wm * 32].tobytes() == exp[0][:wm].tobytes(), (name, mcap)
            assert (msgs[wm * 32:] == 0xEE).all(), (name, mcap)
            assert np.array_equal(control[:wc], exp[2][:wc]) and (control[wc:] == 0xEEEEEEEE).all(), (name, ccap)
            k = 1 if cf is None else len(cf)
            assert cfm[:k].tolist() == ([0] if cf is None else exp[1].tolist()), name
            assert (cfm[k:] == 0xEEEEEEEEEEEEEEEE).all(), name


def test_fixed_cases_cover_what_they_must():
    cs = {k: U.expect_messages(*v) for k, v in U.fixed_cases().items()}
    flags = lambda name: cs[name][0]["flags"].tolist()
    assert len(cs["empty"][0]) == 0 and cs["empty_with_connections"][1].tolist() == [0, 0, 0]
    assert len(cs["only_control"][0]) == 0 and cs["only_control"][2].tolist() == [0, 1, 2]
    assert len(cs["only_ignored"][0]) == 0 and len(cs["only_ignored"][2]) == 0
    assert cs["control_between_fragments"][0]["n_fragments"].tolist() == [3]
    assert flags("cut") == [U.CUT, U.CUT, U.FINAL]
    assert flags("headless_at_start_and_after_final") == [U.HEADLESS | U.FINAL, U.HEADLESS | U.FINAL, U.FINAL,
                                                          U.HEADLESS | U.FINAL]
    assert flags("open_tail") == [U.FINAL, U.OPEN]
    assert flags("open_then_continuation_next_connection") == [U.OPEN, U.HEADLESS | U.FINAL, U.FINAL]
    assert cs["open_then_continuation_next_connection"][0]["conn"].tolist() == [0, 1, 1]
    assert cs["empty_connections"][1].tolist() == [0, 0, 0, 1, 1, 2, 3, 3]
    assert cs["empty_connections"][0]["conn"].tolist() == [2, 4, 5]
    assert flags("oom_fragments") == [U.FINAL | U.LOST, U.FINAL, U.FINAL | U.LOST, U.FINAL | U.LOST]
    assert cs["oom_fragments"][2].tolist() == [5]
    assert cs["opcodes_3_to_7"][0]["opcode"].tolist() == [3, 4, 5, 6, 7]
    assert cs["ignored_statuses"][0]["n_fragments"].tolist() == [2] and len(cs["ignored_statuses"][2]) == 0
    assert cs["conn_first_above_n"][1].tolist() == [0, 1, 2, 2, 2]
    big = cs["across_2_32"][0]
    assert big["payload_size"].tolist() == [3 << 31, 3] and big["payload_off"][0] == (1 << 32) - 5
    assert big["payload_off"][0] + big["payload_size"][0] > 1 << 32


@pytest.mark.parametrize("conns", [None, 1, 7, 40])
def test_host_walk_equals_model_on_random_tables(conns):
    rng = np.random.default_rng(0x6D73 + (conns or 0))
    seen = 0
    for t in range(60):
        n = int(rng.integers(0, 400))
        d, st, cf = U.random_table(rng, n, conns)
        if t % 5 == 4:
            st = None
        exp = U.expect_messages(d, st, cf)
        same(cfws.messages_from_frames(d, st, cf), exp, t)
        seen |= int(np.bitwise_or.reduce(exp[0]["flags"])) if len(exp[0]) else 0
    assert seen == U.FINAL | U.CUT | U.OPEN | U.HEADLESS | U.LOST


def test_record_size_and_exports():
    assert cfws.MESSAGE_DTYPE.itemsize == 32
    src = open(os.path.join(ROOT, "include", "cfws.h")).read()
    assert "typedef struct cfws_message {      /* 32 bytes */" in src
    names = {"cfws_messages_from_frames", "cfws_messages_workspace_size", "cfws_messages_group_frames",
             "cfws_messages_batch"}
    assert names <= set(cfws.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cfws.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert names <= exported
    G = cfws.messages_group_frames()
    assert G >= 64 and G % 64 == 0
    assert cfws.lib().cfws_messages_workspace_size(0, 0) > 0
    assert cfws.lib().cfws_messages_workspace_size(1 << 20, 4097) >= 48 << 20


def fnv1a(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_sanitized_walk_over_exact_size_heap_arrays(tmp_path):
    """The host walk built with AddressSanitizer + UBSan into a stand-alone
    program (make build/messages_asan, which also asserts the record's 32
    bytes), over the fixed cases with every array a heap allocation of
    exactly its size, at the capacities 0, total - 1 and total: no report,
    and every run equals the model."""
    cases = sorted(U.fixed_cases().items())
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, (d, st, cf) in cases:
            f.write(struct.pack("<III", len(d), int(st is not None), 0xFFFFFFFF if cf is None else len(cf)))
            f.write(d.tobytes())
            if st is not None:
                f.write(np.ascontiguousarray(st, np.int32).tobytes())
            if cf is not None:
                f.write(np.ascontiguousarray(cf, np.uint64).tobytes())
    mk = subprocess.run(["make", "-s", "-C", ROOT, "build/messages_asan"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    r = subprocess.run([os.path.join(ROOT, "build", "messages_asan"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) >= 2 * len(cases) and {int(ln[0]) for ln in lines} == set(range(len(cases)))
    for b, mcap, ccap, m, nc, h in lines:
        name, (d, st, cf) = cases[int(b)]
        em, ecfm, ec = U.expect_messages(d, st, cf)
        assert (int(m), int(nc)) == (len(em), len(ec)), name
        cfm = np.zeros(1, np.uint64) if cf is None else ecfm
        want = em[:min(int(mcap), len(em))].tobytes() + cfm.tobytes() + ec[:min(int(ccap), len(ec))].tobytes()
        assert int(h, 16) == fnv1a(want), (name, mcap, ccap)
