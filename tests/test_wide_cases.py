"""The CPU half of tests/test_gpu_wide.py: every case of tests/wide_util.py is
built with the oracle alone and its conditions are checked -- the named
operand crosses 2^32 (frames below, at or above, and across it), the shifted
expectation is the oracle's own output once un-shifted, the route is the one
the case is there for (the three reporters are host functions), and the
device bytes it will hold stay under 24 GiB. These are conditions on the
inputs; the inputs are chosen so that they hold."""
import os

import numpy as np
import pytest

import carryover_util as CU
import oracle as O
import relay_util as RU
import wide_util as U
from coldforce_amd import cfws
from coldforce_amd import workloads as W

K = CU.code_constants()
DEFAULT_KNOBS = not any(k.startswith("CFWS_") and k != "CFWS_LIB" for k in os.environ)
M = U.MARK


def test_deltas():
    for d in (U.DELTAS, U.INDEX_DELTAS):
        assert d["page"] % 4096 == 0 and d["odd16"] % 16 == 0 and (d["odd16"] // 16) % 2 == 1
    assert U.ARENA_BYTES >= M + (4 << 20)


def _crossing(case, inside=True):
    c = case.built()["cross"]
    print(f"{case.name}: {case.operand}: {len(c['below'])} frames below 2^32, {len(c['above'])} at or above, "
          f"across {c['across'][:4].tolist()}")
    assert U.crosses(c), case.msg("does not cross 2^32")
    if inside:
        assert len(c["inside"]), case.msg("no frame starts below 2^32 and ends above it")


def _slots(case):
    from test_gpu_slots import expect_slots
    c, b = case, case.built()
    # slots of 2^31 bytes tile 2^32: no frame can start below it and end above
    _crossing(c, inside=c.slot != 1 << 31)
    if DEFAULT_KNOBS:
        assert c.route() == c.claim
    if c.claim == "deserialize_slots_piece_kernel":
        assert c.piece_form() == c.piece_loop
    st = b["status"]
    assert (st == O.PARSE_COMPLETE).any() and (st == O.ERROR_INVALID_FRAME).any()
    if c.slot <= U.WINDOW_MAX and c.slot < (1 << 20):
        assert (st == O.ERROR_OUT_OF_MEMORY).any()
    if c.relocated:
        assert (st == O.PARSE_MORE_DATA).sum() >= 2 and b["wire_size"] - 1 in b["index"]
        assert b["wire_size"] <= U.ARENA_BYTES and b["base"] + len(b["wire"]) <= U.ARENA_BYTES
    else:
        assert b["wire_size"] >= len(b["wire"])
    # un-shifted, the expectation is the oracle's on the window
    starts = b["index"][:c.K] - np.uint64(b["base"])
    assert np.array_equal(starts, b["starts"])
    if c.scatter:
        obase = M - c.out_delta
        rel = b["dests"] - np.uint64(obase)
        arena, d, s, _ = expect_slots(b["wire"], b["wsize"], starts, b["RW"], b["cap"] - obase, offs=rel)
        for i in (0, c.K // 2, c.K - 1):
            got = np.full(b["RW"], U.SENT, np.uint8)
            part = arena[int(rel[i]):int(rel[i]) + b["RW"]]
            got[:len(part)] = part
            assert np.array_equal(b["rows"][i], got)
        assert obase % 16 == 0 and b["cap"] <= U.ARENA_BYTES
    else:
        arena, d, s, _ = expect_slots(b["wire"], b["wsize"], starts, b["RW"], c.K * b["RW"])
        assert np.array_equal(arena[:c.K * b["RW"]].reshape(c.K, -1), b["rows"])
        assert b["total"] == c.n * c.slot == b["cap"]
    e = b["desc"].copy()
    e["wire_off"] -= np.uint64(b["base"])
    for f in ("wire_off", "payload_size", "mask_key", "fin", "opcode", "mask", "header_size"):
        assert np.array_equal(e[f], d[f]), f
    assert np.array_equal(s, st)
    assert np.array_equal(b["info"]["status"].astype(np.int32), st)


def _index(case):
    c, b = case, case.built()
    _crossing(c)
    assert (b["counts"] > K["index_slots"]).any() and (b["counts"] == 0).any()           # the rest walk
    assert (b["stop"] < 0).any() and (b["stop"] == O.PARSE_MORE_DATA).any() and (b["stop"] == 0).any()
    e = c.inner.expect("B")
    assert np.array_equal(b["starts"] - b["base"], e["starts"]) and np.array_equal(b["consumed"] - b["base"], e["consumed"])
    assert np.array_equal(b["begin"] - b["base"], c.inner.inputs("B")["begin"])
    assert b["base"] + len(b["window"]) <= U.ARENA_BYTES


def _ser(case):
    c, b = case, case.built()
    _crossing(c)
    t = U.ser_tail(c.style)
    assert c.single_pass() == c.style.startswith("single") and c.n > K["small_frames"]
    assert b["shift"] == M - c.delta == 14 + b["b0"] and O.header_size(b["b0"], True) == 14
    e = b["e_desc"][1:].copy()
    e["wire_off"] -= np.uint64(b["shift"])
    assert np.array_equal(CU._desc_bytes(e), CU._desc_bytes(t["e_desc"]))
    assert b["total"] == b["shift"] + len(t["wire"]) <= b["cap"]
    ok = CU.inreg_ok(t["desc"], K["inreg_max"])
    assert ok.all() == (c.style == "single_inreg")              # the frames behind the ballast; the ballast itself never is


def _relay(case):
    c, b = case, case.built()
    _crossing(c)
    st = b["status"][1:]
    assert (st == O.ERROR_INVALID_FRAME).any() and st[-1] == O.PARSE_MORE_DATA
    assert b["out_base"] == M - c.delta == b["out_h"] + b["b0"]
    assert O.header_size(b["b0"], bool(b["in_masked"])) == b["in_h"] and O.header_size(b["b0"], bool(b["out_mask"])) == b["out_h"]
    out, offs, desc, status = RU.expect_relay(b["wire"], b["wire_size"] - b["in_base"], b["index"][1:] - np.uint64(b["in_base"]),
                                              c.policy, b["out_mask"], b["keys"][1:])
    e = b["desc"][1:].copy()
    e["payload_off"] -= np.uint64(b["out_base"])
    e["wire_off"] -= np.uint64(b["in_base"])
    assert np.array_equal(CU._desc_bytes(e), CU._desc_bytes(desc)) and np.array_equal(status, st)
    assert np.array_equal(out, b["out"]) and b["total"] == b["out_base"] + len(out)
    assert (desc["mask"][status == O.PARSE_COMPLETE] != 0).all() == b["in_masked"]


def _fused(case):
    c, b = case, case.built()
    _crossing(c, inside=False)              # 4 KiB slots tile 2^32; payloads are at most 100 B
    if DEFAULT_KNOBS:
        assert c.route() == c.claim
    assert c.N == (1 << 20) + 4096 and b["wsize"] // c.N <= K["fused_avg_max"] and c.N > K["small_frames"]
    assert b["desc"]["payload_size"].max() <= 100 and (b["desc"]["payload_size"] == 0).any()
    st = b["status"]
    assert (st == O.ERROR_INVALID_FRAME).any() and (st == O.PARSE_MORE_DATA).any() and not (st == O.ERROR_OUT_OF_MEMORY).any()
    assert b["shift"] < M < b["total"] and b["shift"] % 4096 == 0
    t = b["tail_desc"]
    assert np.array_equal(t["payload_off"], b["desc"]["payload_off"][b["t0"]:])
    assert CU.blocks(c.N, K["fused_block"]) > 64                 # more than one round of the look-back


def _de_reloc(case):
    c, b = case, case.built()
    _crossing(c)
    if DEFAULT_KNOBS and not c.pe:
        assert c.route() == c.claim
    nb = CU.blocks(c.n, K["plan_block"])
    assert (nb > K["self_scan_blocks"]) == ("single" in c.name) and (c.n <= K["small_frames"]) == ("small" in c.name)
    st = b["status"]
    for code in (O.PARSE_COMPLETE, O.ERROR_INVALID_FRAME, O.PARSE_MORE_DATA, O.ERROR_DATA_TOO_BIG):
        assert (st == code).any(), code
    assert b["wire_size"] - 1 in b["index"] and not (st == O.ERROR_OUT_OF_MEMORY).any()
    out, d, s, tot = O.deserialize_batch(b["wire"][:b["wsize"]], b["index"] - np.uint64(b["base"]), align=c.align,
                                         max_payload=c.MAXP, capacity=b["cap"], flags=c.flags)
    e = b["desc"].copy()
    e["wire_off"] -= np.uint64(b["base"])
    assert np.array_equal(CU._desc_bytes(e), CU._desc_bytes(d)) and np.array_equal(s, st) and tot == b["total"]
    assert np.array_equal(out[:tot], b["out"])
    if c.flags:
        ctl = d["opcode"] >= 8
        assert ctl.any() and (~ctl).any()


def _ser_reloc(case):
    c, b = case, case.built()
    _crossing(c)
    nb = CU.blocks(c.n, K["plan_block"])
    assert (nb > K["self_scan_blocks"]) == ("single" in c.name)
    assert (c.n <= K["small_frames"] and b["cap"] <= K["small_bytes"]) == c.small
    assert CU.inreg_ok(b["desc"], K["inreg_max"]).all() == ("inreg" in c.name)
    wire, d = O.serialize_batch(CU.payload_np(), b["desc"].view(O.DESC_DTYPE))
    e = b["e_desc"].copy()
    e["payload_off"] -= np.uint64(b["base"])
    assert np.array_equal(CU._desc_bytes(e), CU._desc_bytes(d)) and np.array_equal(wire, b["wire"])
    assert np.array_equal(b["d_in"]["payload_off"] - np.uint64(b["base"]), b["desc"]["payload_off"])


def _relay_reloc(case):
    c, b = case, case.built()
    _crossing(c)
    assert (CU.blocks(c.n, K["plan_block"]) > K["self_scan_blocks"]) == ("big" in c.name)
    rel = b["index"] - np.uint64(b["base"])
    assert (np.diff(rel[:c.K].astype(np.int64)) < 0).all() and (c.n == c.K or np.array_equal(rel[:c.K], rel[c.K:2 * c.K]))
    out, offs, desc, status = RU.expect_relay(b["wire"], b["wsize"], rel, c.policy, c.out_mask, b["keys"])
    e = b["desc"].copy()
    e["wire_off"] -= np.uint64(b["base"])
    assert np.array_equal(CU._desc_bytes(e), CU._desc_bytes(desc)) and np.array_equal(status, b["status"])
    assert np.array_equal(out, b["out"]) and (status == O.ERROR_INVALID_FRAME).any() and (status == O.PARSE_MORE_DATA).any()


def _split_send(case):
    c, b = case, case.built()
    _crossing(c)
    assert U.crosses(b["pcross"]) and len(b["pcross"]["inside"]), c.msg("payload_off does not cross 2^32")
    exp = np.full(b["wlen"], U.SENT, np.uint8)
    e = O.encode_headers(b["desc"], exp, b["wlen"])
    O.mask_batch(b["payload"], e, exp, b["wlen"])
    assert np.array_equal(exp, b["exp"])
    u = b["e_desc"].copy()
    u["wire_off"] -= np.uint64(b["wbase"])
    u["payload_off"] -= np.uint64(b["pbase"])
    assert np.array_equal(CU._desc_bytes(u), CU._desc_bytes(e))
    if c.packed:
        import test_split_ops as S
        d = b["desc"]
        inrun = [g for g in range(len(d)) if S.packed_inrun(d, g, b["wlen"])]
        classes = {S.boundary_class(d, g) for g in inrun}
        assert {(hs, t) for hs, t, _ in classes} == {(hs, t) for hs in S.HEADER_CLASSES for t in range(16)}
        assert {(t, tph) for _, t, tph in classes} == {(t, tph) for t in range(16) for tph in range(16)}


def _split_recv(case):
    c, b = case, case.built()
    _crossing(c)
    assert U.crosses(b["pcross"]) and len(b["pcross"]["inside"]), c.msg("payload_off does not cross 2^32")
    pd, st = O.parse_headers(b["wire"], b["index"] - np.uint64(b["wbase"]), wire_size=b["wsize"])
    assert np.array_equal(st, b["status"])
    for code in (O.PARSE_COMPLETE, O.ERROR_INVALID_FRAME, O.PARSE_MORE_DATA):
        assert (st == code).any(), code
    u = b["desc"].copy()
    u["wire_off"] -= np.uint64(b["wbase"])
    u["payload_off"] -= np.uint64(b["obase"])
    for f in ("wire_off", "payload_size", "mask_key", "fin", "opcode", "mask", "header_size"):
        assert np.array_equal(u[f], pd[f]), f
    out = np.full(b["plen"], U.SENT, np.uint8)
    O.unmask_batch(b["wire"], u, st, out, b["plen"])
    assert np.array_equal(out, b["out"])


def _de_ballast(case):
    c, b = case, case.built()
    _crossing(c)
    if DEFAULT_KNOBS and not c.pe:
        assert c.route() == c.claim
    assert (CU.blocks(c.n, K["plan_block"]) > K["self_scan_blocks"]) == ("single" in c.name)
    assert b["b0"] == M - c.delta and b["b0"] % c.align == 0 and O.header_size(b["b0"], True) == 14
    st = b["status"][1:]
    for code in (O.PARSE_COMPLETE, O.ERROR_INVALID_FRAME, O.PARSE_MORE_DATA):
        assert (st == code).any(), code
    if c.flags:
        assert U.crosses(b["ctl_cross"]), c.msg("the control frames do not lie on both sides of 2^32")
    e = b["desc"][1:].copy()
    e["payload_off"] -= np.uint64(b["b0"])
    e["wire_off"] -= np.uint64(b["in_base"])
    assert np.array_equal(CU._desc_bytes(e), CU._desc_bytes(b["tail"]))
    out, d, s, tot = O.deserialize_batch(b["wire"][:b["wire_size"] - b["in_base"]], b["index"][1:] - np.uint64(b["in_base"]),
                                         align=c.align, capacity=b["cap"] - b["b0"], flags=c.flags)
    assert np.array_equal(CU._desc_bytes(d), CU._desc_bytes(b["tail"])) and np.array_equal(s, st)
    assert tot == b["total"] - b["b0"] and np.array_equal(out[:tot], b["out"])


def _uniform(case):
    c, b = case, case.built()
    _crossing(c)
    for k in ("pcross", "scross"):
        assert U.crosses(b[k]), c.msg(k)
    assert c.route() == c.claim
    assert M + (1 << 24) < b["total"] and c.n * c.fs > M and c.n * c.slot > M
    assert (c.n - 1) * c.Wf <= M + (1 << 24) or (c.n - 1) * c.fs <= M + (1 << 20)      # and no frame more than that takes
    s = set(b["samples"].tolist())
    for stride in (c.Wf, c.fs, c.slot):                       # every frame within 64 KiB of the mark
        assert set(range((M - 65536) // stride, (M + 65536) // stride + 1)) <= s
    assert set(range(8)) <= s and set(range(c.n - 8, c.n)) <= s and len(s) >= 256
    assert b["bad"] * c.Wf > M and b["bad"] * c.slot > M      # the frame the second run corrupts


def _h2de(case):
    c, b = case, case.built()
    _crossing(c)
    e = b["e"]
    oom = (e["h2_status"] == O.ERROR_OUT_OF_MEMORY).any()
    assert oom == (c.mode == "general") and (e["h2_status"] != 0).any() and 0 < e["n_msg"] <= b["n"]
    assert b["n"] > 1520                                        # some messages are two DATA frames long
    # nothing the call reports is an offset into the DATA arena: un-shifted, the index is the oracle's own
    assert np.array_equal(b["index"] - np.uint64(b["base"]), O.h2_index(b["h2"]))
    assert b["h2_size"] <= U.ARENA_BYTES and e["total"] <= b["cap"]


def _h2ser(case):
    c, b = case, case.built()
    _crossing(c)
    S = U.H2_S
    assert b["T"] == M - c.delta == b["w0"] + 9 * b["k"] and b["w0"] == 14 + b["b0"] and b["k"] > 260000
    assert c.n > K["small_frames"]
    h2, te = O.h2_serialize_batch(CU.payload_np(), b["desc"][1:].view(O.DESC_DTYPE), c.SID, S)
    assert np.array_equal(h2, b["h2"]) and b["total"] == b["T"] + len(h2) <= b["hcap"]
    e = b["e_desc"][1:].copy()
    e["wire_off"] -= np.uint64(b["w0"])
    te = te.copy()
    te["wire_off"] = W.wire_layout(b["desc"][1:])[0]
    assert np.array_equal(CU._desc_bytes(e), CU._desc_bytes(te))


def _handshake(case):
    import handshake_util as HU
    c, b = case, case.built()
    _crossing(c)
    assert np.array_equal(b["off"] - b["base"], b["rel"]) and b["rel"][-1] == len(b["raw"])
    assert b["base"] + len(b["raw"]) <= U.ARENA_BYTES
    want = b["ok"] if c.call == "check" else b["valid"]
    assert 0.2 * c.n < int(want.sum()) < 0.8 * c.n               # both verdicts well covered
    i = c.n // 2
    item = bytes(b["raw"][b["rel"][i]:b["rel"][i + 1]])
    if c.call == "check":
        assert bool(b["ok"][i]) == HU.check(b["accepts"][i].encode(), item)
    else:
        assert item == b["keys"][i] and b["accepts"][i] == O.ws_accept_key(item)


CHECKS = {U.SlotCase: _slots, U.IndexCase: _index, U.SerBallastCase: _ser, U.RelayBallastCase: _relay,
          U.FusedCase: _fused, U.DeRelocCase: _de_reloc, U.SerRelocCase: _ser_reloc, U.RelayRelocCase: _relay_reloc,
          U.SplitSendCase: _split_send, U.SplitRecvCase: _split_recv, U.DeBallastCase: _de_ballast,
          U.UniformCase: _uniform, U.H2DeRelocCase: _h2de, U.H2SerBallastCase: _h2ser, U.HandshakeCase: _handshake}


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_case_conditions(name):
    case = U.cases()[name]
    try:
        CHECKS[type(case)](case)
        assert case.device_bytes() <= U.BUDGET, case.device_bytes()
    finally:
        case.release()


def test_every_table_row_built_here_has_a_case():
    names = " ".join(U.CASE_NAMES)
    for part in ("slots_index_window", "slots_index_piece", "scatter_off_window", "scatter_off_piece", "slots_dest_2gib",
                 "slots_dest_1mib16_loop", "slots_dest_1mib16_straight", "slots_dest_window", "slots_dest_perframe",
                 "index_ws", "index_h2_info", "index_h2_noinfo", "ser_mixed2500", "ser_single_tiny", "ser_single_inreg",
                 "relay_unmask", "relay_mask", "relay_remask", "de_fused", "de_index_small", "de_index_plan3000",
                 "de_index_reasm3000", "de_index_single", "ser_off_small", "ser_off_mixed", "ser_off_single_tiny",
                 "ser_off_single_inreg", "relay_index_3000", "relay_index_big", "split_send_packed",
                 "split_send_scattered", "split_recv", "de_off_plan3000", "de_off_reasm8000", "de_off_single", "uniform_small", "uniform_general", "uniform_bytes",
                 "h2de_index_fast", "h2de_index_general", "h2ser_rows_S16384", "handshake_accept_key_off",
                 "handshake_upgrade_key_off", "handshake_check_resp_off", "slots_index_perframe2064"):
        assert part in names, part
    assert W.round16(U.MARK) == U.MARK
    assert cfws.INFO_DTYPE.itemsize == 8
