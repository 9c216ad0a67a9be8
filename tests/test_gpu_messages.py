"""Message and control tables of received frames on the GPU
(cfws_messages_batch, include/cfws.h) against the model of
tests/messages_util.py, which tests/test_messages_host.py pins to the
generator's own table and the host form to. Every call runs with the outputs
filled with a sentinel and the workspace with 0xAA."""
import numpy as np
import pytest

import messages_util as U
import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from coldforce_amd import workloads as W  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()


def G():
    return cfws.messages_group_frames()


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


class Call:
    """One cfws_messages_batch call's device buffers: sentinel-filled outputs
    with two rows behind each capacity, a 0xAA workspace."""

    def __init__(self, d, st, cf, mcap, ccap, ws_t=None):
        self.n, self.mcap, self.ccap = len(d), mcap, ccap
        self.conns = 0 if cf is None else len(cf)
        self.desc = cfws.desc_to_device(d) if len(d) else torch.zeros((1, 32), dtype=torch.uint8, device="cuda")[:0]
        self.status = None if st is None else torch.from_numpy(np.ascontiguousarray(st, np.int32)).cuda()
        self.cf = None if cf is None else (dev_i64(cf) if len(cf) else torch.zeros(1, dtype=torch.int64, device="cuda")[:0])
        self.msgs = torch.full((mcap + 2, 32), 0xEE, dtype=torch.uint8, device="cuda")
        self.control = torch.full((ccap + 2,), -1, dtype=torch.int32, device="cuda")
        self.cfm = torch.full((max(self.conns, 1) + 2,), -1, dtype=torch.int64, device="cuda")
        self.totals = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        size = cfws.lib().cfws_messages_workspace_size(self.n, self.conns)
        self.ws = ws_t if ws_t is not None else torch.empty(size, dtype=torch.uint8, device="cuda")
        assert self.ws.numel() >= size
        self.ws.fill_(0xAA)

    def launch(self):
        p = lambda t: None if t is None else t.data_ptr()
        return cfws.lib().cfws_messages_batch(
            p(self.desc), p(self.status), self.n, p(self.cf), self.conns, self.msgs.data_ptr(), self.mcap,
            self.cfm.data_ptr(), self.totals.data_ptr(), self.control.data_ptr(), self.ccap,
            self.totals.data_ptr() + 8, self.ws.data_ptr(), self.ws.numel(), None)

    def check(self, exp, what=""):
        em, ecfm, ec = exp
        torch.cuda.synchronize()
        assert self.totals.tolist() == [len(em), len(ec)], what
        wm, wc = min(self.mcap, len(em)), min(self.ccap, len(ec))
        msgs = self.msgs.cpu().numpy().reshape(-1)
        assert msgs[:wm * 32].tobytes() == em[:wm].tobytes(), what
        assert (msgs[wm * 32:] == 0xEE).all(), what
        control = self.control.cpu().numpy()
        assert np.array_equal(control[:wc].view(np.uint32), ec[:wc]) and (control[wc:] == -1).all(), what
        cfm = self.cfm.cpu().numpy()
        k = 1 if ecfm is None else len(ecfm)
        assert cfm[:k].tolist() == ([0] if ecfm is None else ecfm.tolist()), what
        assert (cfm[k:] == -1).all(), what


def run(d, st, cf, exp=None, mcap=None, ccap=None, what=""):
    exp = U.expect_messages(d, st, cf) if exp is None else exp
    c = Call(d, st, cf, len(exp[0]) if mcap is None else mcap, len(exp[2]) if ccap is None else ccap)
    assert c.launch() == 0, cfws.lib().cfws_last_error()
    c.check(exp, what)
    return exp


# ---- sizes and group boundaries ---------------------------------------------------

@pytest.mark.parametrize("which", ["1", "G-1", "G", "G+1", "3G+1"])
@pytest.mark.parametrize("conns", [None, 6])
def test_sizes_around_the_group(which, conns):
    n = {"1": 1, "G-1": G() - 1, "G": G(), "G+1": G() + 1, "3G+1": 3 * G() + 1}[which]
    rng = np.random.default_rng(n + (conns or 0))
    d, st, cf = U.random_table(rng, n, conns)
    run(d, st, cf)


def group_cases():
    g = G()
    one = U.message(1)
    cs = {}
    # fragments at frames G-2 .. G+1
    cs["message_straddles_a_group"] = (one * (g - 2) + U.message(4, U.BINARY) + one * 5, None)
    cs["message_spans_whole_groups"] = (one * 3 + U.message(2 * g + 3) + U.message(2, U.BINARY), None)
    cs["control_run_longer_than_a_group"] = ([(U.TEXT, 0)] + [(U.PING, 1)] * (g + 5) + [(U.CONT, 1)] + one, None)
    # one chain of unfinished CONTINUATIONs cut by connection boundaries at G-1, G and G+1
    cs["connection_boundaries_at_the_group"] = ([(U.CONT, 0)] * (2 * g), [0, g - 1, g, g + 1])
    cs["open_tail_in_a_groups_last_slot"] = (one * (g - 1) + [(U.TEXT, 0)], None)
    cs["open_tail_then_next_connection"] = (one * (g - 1) + [(U.TEXT, 0)] + [(U.CONT, 1)] + one * 2, [0, g])
    cs["group_of_only_ignored_frames"] = ([(U.TEXT, 0)] + [(U.TEXT, 1, 5, U.INVALID_FRAME)] * (2 * g + 7) +
                                          [(U.CONT, 1)], None)
    return cs


@pytest.mark.parametrize("name", ["message_straddles_a_group", "message_spans_whole_groups",
                                  "control_run_longer_than_a_group", "connection_boundaries_at_the_group",
                                  "open_tail_in_a_groups_last_slot", "open_tail_then_next_connection",
                                  "group_of_only_ignored_frames"])
def test_group_boundaries(name):
    rows, cf = group_cases()[name]
    d, st = U.table(rows)
    cf = None if cf is None else np.array(cf, np.uint64)
    exp = run(d, st, cf, what=name)
    flags = exp[0]["flags"].tolist()
    if name == "message_spans_whole_groups":
        assert exp[0]["n_fragments"].tolist() == [1, 1, 1, 2 * G() + 3, 2]
    if name == "control_run_longer_than_a_group":
        assert exp[0]["n_fragments"].tolist() == [2, 1] and len(exp[2]) == G() + 5
    if name == "connection_boundaries_at_the_group":
        assert flags == [U.HEADLESS | U.OPEN] * 4 and exp[0]["first_frame"].tolist() == [0, G() - 1, G(), G() + 1]
    if name == "open_tail_in_a_groups_last_slot":
        assert flags[-1] == U.OPEN and exp[0]["first_frame"][-1] == G() - 1
    if name == "open_tail_then_next_connection":
        assert flags[G() - 1:G() + 1] == [U.OPEN, U.HEADLESS | U.FINAL]
    if name == "group_of_only_ignored_frames":
        assert flags == [U.FINAL] and exp[0]["n_fragments"].tolist() == [2]


def test_status_null():
    rows, _ = group_cases()["control_run_longer_than_a_group"]
    d, _ = U.table(rows + U.message(3))
    run(d, None, None)
    run(d, None, np.array([0, 1, G() + 3], np.uint64))


def test_large_single_frame_messages_over_many_connections():
    """2^20 + 1 single-frame messages over 4,097 connections: the scan of the
    block sums beyond a handful of blocks, and d_conn_first_msg."""
    n, conns = (1 << 20) + 1, 4097
    rng = np.random.default_rng(4097)
    d = np.zeros(n, dtype=cfws.DESC_DTYPE)
    d["payload_size"] = rng.integers(0, 4000, n)
    d["payload_off"] = np.cumsum(d["payload_size"]) - d["payload_size"]
    d["fin"], d["opcode"], d["mask"] = 1, rng.integers(1, 3, n), 1
    cuts = np.sort(rng.integers(0, n + 1, conns - 1))
    cuts[100:103] = cuts[100]                                   # empty connections
    cf = np.concatenate([[0], np.sort(cuts)]).astype(np.uint64)
    exp = U.expect_messages(d, None, cf)
    assert len(exp[0]) == n and np.array_equal(exp[1], cf)
    run(d, None, cf, exp=exp)


# ---- host agreement -----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(U.fixed_cases()))
def test_device_equals_host_on_fixed_cases(name):
    """The fixed cases of the host test, device against host form byte for
    byte, at the capacities 0, total - 1 and total."""
    d, st, cf = U.fixed_cases()[name]
    hm, hcfm, hc, m, nc = cfws.messages_from_frames(d, st, cf)
    assert (len(hm), len(hc)) == (m, nc)
    for mcap in U.capacities(m):
        for ccap in U.capacities(nc):
            run(d, st, cf, exp=(hm, hcfm, hc), mcap=mcap, ccap=ccap, what=(name, mcap, ccap))


def test_control_outputs_may_be_null():
    d, st, cf = U.fixed_cases()["control_between_fragments"]
    exp = U.expect_messages(d, st, cf)
    c = Call(d, st, cf, len(exp[0]), 0)
    rc = cfws.lib().cfws_messages_batch(c.desc.data_ptr(), c.status.data_ptr(), c.n, None, 0, c.msgs.data_ptr(),
                                        c.mcap, None, c.totals.data_ptr(), None, 0, None, c.ws.data_ptr(),
                                        c.ws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert c.totals.tolist() == [len(exp[0]), -1]
    assert c.msgs.cpu().numpy().reshape(-1)[:32 * len(exp[0])].tobytes() == exp[0].tobytes()
    assert (c.control == -1).all() and (c.cfm == -1).all()


# ---- refusals ----------------------------------------------------------------------

def test_argument_errors_write_nothing():
    d, st, cf = U.fixed_cases()["empty_connections"]
    exp = U.expect_messages(d, st, cf)
    c = Call(d, st, cf, len(exp[0]), 4)
    L = cfws.lib()
    p = dict(desc=c.desc.data_ptr(), status=c.status.data_ptr(), cf=c.cf.data_ptr(), msgs=c.msgs.data_ptr(),
             cfm=c.cfm.data_ptr(), n_msg=c.totals.data_ptr(), control=c.control.data_ptr(),
             n_ctl=c.totals.data_ptr() + 8, ws=c.ws.data_ptr(), ws_size=c.ws.numel())

    def call(**over):
        a = dict(p, **over)
        return L.cfws_messages_batch(a["desc"], a["status"], c.n, a["cf"], c.conns, a["msgs"], c.mcap, a["cfm"],
                                     a["n_msg"], a["control"], c.ccap, a["n_ctl"], a["ws"], a["ws_size"], None)

    INVALID, WORKSPACE = -1, -2
    assert call(msgs=p["msgs"] + 8) == INVALID
    assert call(msgs=p["msgs"] + 1) == INVALID
    assert b"16-byte" in L.cfws_last_error()
    assert call(ws_size=p["ws_size"] - 1) == WORKSPACE
    assert call(ws_size=0) == WORKSPACE
    for name in ("desc", "msgs", "cfm", "n_msg", "control", "ws"):
        assert call(**{name: None}) == INVALID, name
    assert b"messages" in L.cfws_last_error()
    torch.cuda.synchronize()
    assert (c.msgs == 0xEE).all() and (c.control == -1).all() and (c.cfm == -1).all() and (c.totals == -1).all()
    assert (c.ws == 0xAA).all()
    assert call() == 0
    c.check(exp)


# ---- workspace reuse -----------------------------------------------------------------

def test_two_batches_through_one_workspace():
    rng = np.random.default_rng(2)
    a = U.random_table(rng, 2 * G() + 17, 9)
    b = U.random_table(rng, G() - 3, None)
    ws = torch.empty(cfws.lib().cfws_messages_workspace_size(len(a[0]), 9), dtype=torch.uint8, device="cuda")
    ea, eb = U.expect_messages(*a), U.expect_messages(*b)
    ca = Call(*a, len(ea[0]), len(ea[2]), ws_t=ws)
    cb = Call(*b, len(eb[0]), len(eb[2]), ws_t=ws)
    assert ca.launch() == 0 and cb.launch() == 0 and ca.launch() == 0       # back to back, same stream
    cb.check(eb, "second")
    ca.check(ea, "first, again after the second")


# ---- end to end --------------------------------------------------------------------

def test_end_to_end_one_connection():
    """Config 3's generator -> serialize -> reassembling receive -> messages,
    with no host copy between: the table equals the generator's and every
    message's arena bytes equal the original message."""
    desc, messages = W.zipf_batch(1 << 20, ping_every=3, max_messages=300)
    n_arena = messages["arena_bytes"]
    payload = torch.empty(W.round16(n_arena) + 16, dtype=torch.uint8, device="cuda")
    cfws.fill_splitmix(payload, 3)
    offs, total = W.wire_layout(desc)
    wire = torch.empty(W.round16(total), dtype=torch.uint8, device="cuda")
    cfws.serialize(payload, cfws.desc_to_device(desc), wire)
    out = torch.full((W.round16(n_arena) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    idx_t = torch.from_numpy(offs.astype(np.int64)).cuda()
    d2, st, ptot = cfws.deserialize(wire, total, idx_t, out, flags=cfws.DESERIALIZE_REASSEMBLE)
    msgs_t, _, control_t, m, nc = cfws.messages_batch(d2, st)
    assert (m, nc) == (len(messages["off"]), messages["pings"])
    got = cfws.messages_from_device(msgs_t[:m])
    assert np.array_equal(got["payload_off"], messages["off"])
    assert np.array_equal(got["payload_size"], messages["len"])
    assert np.array_equal(got["opcode"], messages["opcode"])
    assert np.array_equal(got["first_frame"], messages["first_frame"])
    assert (got["flags"] == U.FINAL).all() and not got["conn"].any() and not got["zero"].any()
    for i, (a, k) in enumerate(zip(messages["first_frame"], messages["n_frames"])):
        assert got["n_fragments"][i] == int((desc["opcode"][a:a + k] < 8).sum())
    assert np.array_equal(control_t[:nc].cpu().numpy(), np.flatnonzero(desc["opcode"] == 9))
    arena, orig = out.cpu().numpy(), payload.cpu().numpy()
    for r, off, ln in zip(got, messages["off"], messages["len"]):
        a, b = int(r["payload_off"]), int(r["payload_off"] + r["payload_size"])
        assert np.array_equal(arena[a:b], orig[int(off):int(off) + int(ln)])


def wire_of(frames):
    """Client-masked wire bytes of (opcode, fin, payload bytes) frames."""
    return b"".join(O.serialize_keyed(bool(fin), op, True, 0x9E3779B9 + 77 * i, data)
                    for i, (op, fin, data) in enumerate(frames))


def tick(buffers):
    """Index -> reassembling receive -> messages over the receive buffers of
    one tick, all on the device: (messages, conn_first_msg, control, arena)."""
    blob = b"".join(buffers)
    ends = np.cumsum([len(b) for b in buffers])
    begin_t = torch.from_numpy((ends - [len(b) for b in buffers]).astype(np.int64)).cuda()
    end_t = torch.from_numpy(ends.astype(np.int64)).cuda()
    buf_t = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    starts_t, first_t, consumed_t, stop_t, total = cfws.index_frames_batch(buf_t, begin_t, end_t)
    assert consumed_t.tolist() == ends.tolist()
    out = torch.full((len(blob) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d2, st, _ = cfws.deserialize(buf_t, len(blob), starts_t[:total], out, flags=cfws.DESERIALIZE_REASSEMBLE)
    msgs_t, cfm_t, control_t, m, nc = cfws.messages_batch(d2, st, conn_first_t=first_t)
    return cfws.messages_from_device(msgs_t[:m]), cfm_t.tolist(), control_t[:nc].tolist(), out.cpu().numpy()


def test_end_to_end_connections_over_two_ticks():
    """Three receive buffers (one empty, one ending inside a fragmented
    message, one whole) through the indexer, whose d_first is d_conn_first;
    then the tick that brings the rest: OPEN, then HEADLESS + FINAL, and the
    two byte ranges joined are the message."""
    rng = np.random.default_rng(11)
    by = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    hello, part = by(300), [by(5000), by(130), by(70000), by(9)]
    whole = [by(20), by(1000), by(7)]
    b1 = wire_of([(U.TEXT, 1, hello), (U.BINARY, 0, part[0]), (U.CONT, 0, part[1])])
    b2 = wire_of([(U.TEXT, 0, whole[0]), (U.PING, 1, b"12345678"), (U.CONT, 1, whole[1]), (U.BINARY, 1, whole[2])])
    msgs, cfm, control, arena = tick([b"", b1, b2])
    assert cfm == [0, 0, 2] and control == [4]
    assert msgs["conn"].tolist() == [1, 1, 2, 2] and msgs["first_frame"].tolist() == [0, 1, 3, 6]
    assert msgs["flags"].tolist() == [U.FINAL, U.OPEN, U.FINAL, U.FINAL]
    assert msgs["n_fragments"].tolist() == [1, 2, 2, 1] and msgs["opcode"].tolist() == [U.TEXT, U.BINARY, U.TEXT, U.BINARY]
    cut = lambda r, a: a[int(r["payload_off"]):int(r["payload_off"] + r["payload_size"])].tobytes()
    assert cut(msgs[0], arena) == hello and cut(msgs[2], arena) == whole[0] + whole[1]
    assert cut(msgs[3], arena) == whole[2]
    head = cut(msgs[1], arena)
    # the next tick: connection 1's buffer begins with the CONTINUATION frames
    b1 = wire_of([(U.CONT, 0, part[2]), (U.CONT, 1, part[3]), (U.TEXT, 1, hello)])
    msgs, cfm, control, arena = tick([b"", b1, b""])
    assert cfm == [0, 0, 2] and control == []
    assert msgs["flags"].tolist() == [U.HEADLESS | U.FINAL, U.FINAL] and msgs["conn"].tolist() == [1, 1]
    assert msgs["opcode"].tolist() == [U.CONT, U.TEXT] and msgs["n_fragments"].tolist() == [2, 1]
    assert head + cut(msgs[0], arena) == b"".join(part)
    assert cut(msgs[1], arena) == hello
