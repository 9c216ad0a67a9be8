"""HTTP/2 DATA frames of many streams, by message, on the GPU
(cfws_h2_streams_batch, include/cfws.h) against the model of
tests/h2_streams_util.py, which tests/test_h2_streams.py pins the host form
to. Every call runs with each output an allocation of exactly what the counts
say between two 64-byte guards, outputs and guards filled with a sentinel and
the workspace with 0xAA; every output is compared byte for byte up to its
count and the guards must keep the sentinel."""
import numpy as np
import pytest

import h2_streams_util as U
import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402

GUARD = 64
INVALID, WORKSPACE = -1, -2


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()


def G():
    return cfws.h2_streams_group_frames()


def dev_bytes(a):
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)
    return torch.from_numpy(b.copy()).cuda() if len(b) else torch.zeros(16, dtype=torch.uint8, device="cuda")


class Call:
    """One cfws_h2_streams_batch call's device buffers."""

    OUTPUTS = ("order", "order_frame", "msgs", "cfm", "stream_first", "counts")

    def __init__(self, starts, info, cf, exp, fill=0xEE, ws_t=None, ws_fill=0xAA):
        self.n, self.fill, self.exp = len(info), fill, exp
        self.conns = 0 if cf is None else len(cf)
        self.starts, self.info = dev_bytes(np.asarray(starts, np.uint64)), dev_bytes(info)
        self.cf = None if cf is None else dev_bytes(np.asarray(cf, np.uint64))
        c = exp[5]
        frames, rows = c[1] + c[3], c[0] + c[2]
        self.want = dict(order=exp[0].tobytes(), order_frame=exp[1].tobytes(), msgs=exp[2].tobytes(),
                         cfm=(np.zeros(1, np.uint64) if cf is None else exp[3]).tobytes(),
                         stream_first=exp[4].tobytes(), counts=np.array(c, np.uint64).tobytes())
        assert (len(self.want["order"]), len(self.want["msgs"])) == (8 * frames, 32 * rows)
        self.buf = {k: torch.full((2 * GUARD + len(self.want[k]),), fill, dtype=torch.uint8, device="cuda")
                    for k in self.OUTPUTS}
        size = cfws.lib().cfws_h2_streams_workspace_size(self.n, self.conns)
        self.ws = ws_t if ws_t is not None else torch.empty(size, dtype=torch.uint8, device="cuda")
        assert self.ws.numel() >= size
        self.ws.fill_(ws_fill)

    def ptr(self, k):
        return self.buf[k].data_ptr() + GUARD

    def args(self):
        return dict(starts=self.starts.data_ptr(), info=self.info.data_ptr(),
                    cf=None if self.cf is None else self.cf.data_ptr(), order=self.ptr("order"),
                    order_frame=self.ptr("order_frame"), msgs=self.ptr("msgs"), cfm=self.ptr("cfm"),
                    stream_first=self.ptr("stream_first"), counts=self.ptr("counts"), ws=self.ws.data_ptr(),
                    ws_size=self.ws.numel())

    def launch(self, **over):
        a = dict(self.args(), **over)
        return cfws.lib().cfws_h2_streams_batch(a["starts"], a["info"], self.n, a["cf"], self.conns, a["order"],
                                                a["order_frame"], a["msgs"], a["cfm"], a["stream_first"],
                                                a["counts"], a["ws"], a["ws_size"], None)

    def outputs(self):
        torch.cuda.synchronize()
        return {k: self.buf[k].cpu().numpy() for k in self.OUTPUTS}

    def check(self, what=""):
        for k, host in self.outputs().items():
            n = len(self.want[k])
            assert (host[:GUARD] == self.fill).all() and (host[GUARD + n:] == self.fill).all(), (what, k, "guard")
            if k == "counts":
                assert np.frombuffer(host[GUARD:GUARD + n].tobytes(), np.uint64).tolist() == self.exp[5], what
            assert host[GUARD:GUARD + n].tobytes() == self.want[k], (what, k)

    def untouched(self):
        return all((h == self.fill).all() for h in self.outputs().values())


def run(starts, info, cf, what="", **kw):
    exp = U.expect(starts, info, cf)
    c = Call(starts, info, cf, exp, **kw)
    assert c.launch() == 0, cfws.lib().cfws_last_error()
    c.check(what)
    return exp


# ---- the fixed cases ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(U.fixed_cases()))
def test_fixed_cases(name):
    """Every fixed case of the host test (64-bit starts at and above 2^32
    among them: d_order carries them whole)."""
    starts, info, cf = U.fixed_cases()[name]
    exp = run(starts, info, cf, what=name)
    host = cfws.h2_streams_from_frames(starts, info, cf)
    assert host[5] == exp[5] and host[2].tobytes() == exp[2].tobytes()


def test_optional_outputs_may_be_null():
    starts, info, cf = U.fixed_cases()["no_conn_first"]
    c = Call(starts, info, cf, U.expect(starts, info, cf))
    assert c.launch(order_frame=None, cfm=None, stream_first=None) == 0
    out = c.outputs()
    for k in ("order", "msgs", "counts"):
        assert out[k][GUARD:GUARD + len(c.want[k])].tobytes() == c.want[k], k
    for k in ("order_frame", "cfm", "stream_first"):
        assert (out[k] == c.fill).all(), k


# ---- sizes around the sort's tile ---------------------------------------------------

@pytest.mark.parametrize("between", [False, True])
@pytest.mark.parametrize("how", ["distinct", "one", "mixed"])
@pytest.mark.parametrize("which", ["1", "G-1", "G", "G+1", "2G+3"])
def test_connection_sizes_around_the_tile(which, how, between):
    """A connection of 1, G-1, G, G+1 and 2G+3 DATA records (G: the rows one
    workgroup sorts in LDS; a connection across a multiple of G goes through
    the merge passes), alone and between two small neighbours that move it
    off the tile grid."""
    n = {"1": 1, "G-1": G() - 1, "G": G(), "G+1": G() + 1, "2G+3": 2 * G() + 3}[which]
    rng = np.random.default_rng(n * 7 + len(how) + between)
    rows = U.connection(n, how, rng)
    cf = None
    if between:
        rows = [U.d(2, 5), U.d(1, 6, U.END), U.d(2, 7)] + rows + [U.d(1, 1, U.END), U.d(1, 2)]
        cf = np.array([0, 3, 3 + n], np.uint64)
    starts, info = U.table(rows)
    exp = run(starts, info, cf, what=(which, how, between))
    if how == "distinct" and not between:
        assert exp[1].tolist() == [k for k in range(n - 1, -1, -1) if k % 3] + [k for k in range(n - 1, -1, -1)
                                                                                if k % 3 == 0]


def test_connections_across_several_tiles():
    """Connections that take two, three and four merge passes next to ones
    that take none, ignored records between the DATA records."""
    rng = np.random.default_rng(5)
    g = G()
    sizes = [5, 9 * g + 5, 0, 17, 3 * g - 1, 2, g, 4 * g + 2, 40]
    rows, cf = [], []
    for k, n in enumerate(sizes):
        cf.append(len(rows))
        for r in U.connection(n, ["mixed", "distinct", "one"][k % 3], rng):
            rows.append(r)
            if rng.random() < 0.05:
                rows.append((U.PING, 0, 0, 8))
    starts, info = U.table(rows)
    run(starts, info, np.array(cf, np.uint64))


def test_5000_connections_of_0_to_9_records():
    rng = np.random.default_rng(5000)
    rows, cf = [], []
    for c in range(5000):
        cf.append(len(rows))
        k = int(rng.integers(0, 10))
        sids = rng.integers(0, 4, k)
        ends = rng.random(k) < 0.4
        rows += [(U.DATA if rng.random() < 0.9 else U.HEADERS, int(s), U.END if e else 0, 100) for s, e in
                 zip(sids, ends)]
    starts, info = U.table(rows)
    exp = run(starts, info, np.array(cf, np.uint64))
    assert exp[5][0] > 3000 and exp[5][2] > 3000


def test_random_tables():
    rng = np.random.default_rng(0x6833)
    for t in range(12):
        starts, info, cf = U.random_table(rng, int(rng.integers(1, 3000)), [None, 1, 7, 300][t % 4])
        run(starts, info, cf, what=t)


# ---- what the workspace and the outputs held ----------------------------------------

def test_prefill_does_not_change_the_result_and_two_batches_share_a_workspace():
    rng = np.random.default_rng(8)
    a = U.random_table(rng, 2 * G() + 77, 9)
    b = U.random_table(rng, G() - 5, None)
    ws = torch.empty(cfws.lib().cfws_h2_streams_workspace_size(len(a[1]), 9), dtype=torch.uint8, device="cuda")
    ea, eb = U.expect(*a), U.expect(*b)
    got = []
    for fill in (0xA5, 0x00):
        ca = Call(*a, ea, fill=fill, ws_t=ws, ws_fill=fill)
        assert ca.launch() == 0
        ca.check(("first", fill))
        cb = Call(*b, eb, fill=fill, ws_t=ws, ws_fill=fill)
        # back to back on one stream through one workspace: second, then the first again
        assert cb.launch() == 0 and ca.launch() == 0
        cb.check(("second", fill))
        ca.check(("first again", fill))
        out = ca.outputs()
        got.append({k: out[k][GUARD:GUARD + len(ca.want[k])].tobytes() for k in Call.OUTPUTS})
    assert got[0] == got[1]


# ---- refusals ----------------------------------------------------------------------

def test_argument_errors_write_nothing():
    starts, info, cf = U.fixed_cases()["empty_connections"]
    c = Call(starts, info, cf, U.expect(starts, info, cf))
    L = cfws.lib()
    a = c.args()
    assert c.launch(msgs=a["msgs"] + 8) == INVALID
    assert c.launch(msgs=a["msgs"] + 1) == INVALID
    assert b"16-byte" in L.cfws_last_error()
    assert c.launch(ws_size=a["ws_size"] - 1) == WORKSPACE
    assert c.launch(ws_size=0) == WORKSPACE
    for name in ("starts", "info", "order", "msgs", "cfm", "counts", "ws"):
        assert c.launch(**{name: None}) == INVALID, name
    assert b"h2 streams" in L.cfws_last_error()
    big = L.cfws_h2_streams_batch(a["starts"], a["info"], 1 << 32, a["cf"], c.conns, a["order"], a["order_frame"],
                                  a["msgs"], a["cfm"], a["stream_first"], a["counts"], a["ws"], 1 << 62, None)
    assert big == INVALID and b"2^32" in L.cfws_last_error()
    assert c.untouched() and (c.ws == 0xAA).all()
    assert c.launch() == 0
    c.check()


def test_no_frames_writes_zero_counts():
    for cf in (None, np.zeros(3, np.uint64)):
        starts, info = U.table([])
        c = Call(starts, info, cf, U.expect(starts, info, cf))
        assert c.launch() == 0
        c.check(cf)
        assert c.launch(starts=None, info=None, order=None, msgs=None) == 0
        c.check(cf)


# ---- end to end --------------------------------------------------------------------

# one stream's WS frames: (opcode, fin, payload bytes); three WS messages of 1, 3 and 1 fragments
WS_FRAMES = [(1, 1, 0), (2, 0, 7), (0, 0, 126), (0, 1, 1000), (1, 1, 40000)]
WS_FIELDS = ("payload_size", "mask_key", "fin", "opcode", "mask", "header_size")


def stream_bytes(rng, sid):
    """The DATA frames of one stream carrying WS_FRAMES, as a list of byte strings."""
    arena = rng.integers(0, 256, 42000, dtype=np.uint8)
    d = np.zeros(len(WS_FRAMES), dtype=O.DESC_DTYPE)
    for i, (op, fin, size) in enumerate(WS_FRAMES):
        d[i] = (int(rng.integers(0, 42000 - size)), 0, size, int(rng.integers(0, 1 << 32)), fin, op, 1, 0)
    h2, _ = O.h2_serialize_batch(arena, d, sid, 16384)
    at = [int(x) for x in O.h2_index(h2)] + [len(h2)]
    return [h2[a:b].tobytes() for a, b in zip(at[:-1], at[1:])]


def control_frame(rng):
    k = int(rng.integers(0, 3))
    if k == 0:
        return bytes([0, 0, 6, U.SETTINGS, 0, 0, 0, 0, 0]) + bytes([0, 4, 0, 1, 0, 0])
    if k == 1:
        return bytes([0, 0, 8, U.PING, 0, 0, 0, 0, 0]) + bytes(8)
    return bytes([0, 0, 4, U.WINDOW_UPDATE, 0, 0, 0, 0, 1]) + bytes([0, 0, 16, 0])


def build_connections(seed):
    """7 connections of 1 to 4 streams: per connection the byte strings of its
    frames in wire order, (stream id or None, bytes), the streams' DATA frames
    interleaved at random with SETTINGS, PING and WINDOW_UPDATE between."""
    rng = np.random.default_rng(seed)
    conns = []
    for c in range(7):
        sids = [1 + 2 * int(x) for x in rng.permutation(6)[:1 + c % 4]]
        left = {sid: stream_bytes(rng, sid) for sid in sids}
        frames = []
        while left:
            sid = int(rng.choice(sorted(left)))
            frames.append((sid, left[sid].pop(0)))
            if not left[sid]:
                del left[sid]
            if rng.random() < 0.3:
                frames.append((None, control_frame(rng)))
        conns.append(frames)
    return conns


def expected_messages(frames_by_conn):
    """(conn, stream) -> what oracle.h2_deserialize_batch delivers from that
    stream's own frames, up to its last END_STREAM: per message (descriptor
    fields, status, payload bytes)."""
    out = {}
    for c, frames in enumerate(frames_by_conn):
        for sid in sorted({s for s, _ in frames if s is not None}):
            own = [b for s, b in frames if s == sid]
            while own and not own[-1][4] & 1:
                own.pop()
            if not own:
                continue
            h2 = np.frombuffer(b"".join(own), np.uint8).copy()
            r = O.h2_deserialize_batch(h2, O.h2_index(h2), 16384)
            out[(c, sid)] = [(tuple(int(dd[f]) for f in WS_FIELDS), int(st),
                              r["payload"][int(dd["payload_off"]):int(dd["payload_off"] + dd["payload_size"])].tobytes())
                             for dd, st in zip(r["msg_desc"], r["msg_status"])]
    return out


def tick(buffers):
    """index (ALL) -> streams -> counts -> one receive over d_order[:F] ->
    message tables per stream, all on the device. Returns the delivered
    messages per (conn, stream) in table order, the WS message tables, each
    connection's consumed position and the bytes of its tails' frames."""
    blob = b"".join(buffers)
    ends = np.cumsum([len(b) for b in buffers])
    begins = ends - [len(b) for b in buffers]
    begin_t, end_t = torch.from_numpy(begins.astype(np.int64)).cuda(), torch.from_numpy(ends.astype(np.int64)).cuda()
    buf_t = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    starts_t, info_t, first_t, consumed_t, stop_t, total = cfws.h2_index_frames_batch(
        buf_t, begin_t, end_t, select=cfws.H2_INDEX_ALL)
    order_t, of_t, msgs_t, cfm_t, sf_t, counts = cfws.h2_streams_batch(starts_t, info_t, total, conn_first_t=first_t)
    M, F, T, TF, S = counts
    starts = starts_t[:total].cpu().numpy().view(np.uint64)
    info = cfws.h2_info_from_device(info_t[:total])
    exp = U.expect(starts, info, first_t.cpu().numpy().view(np.uint64))
    assert counts == exp[5]
    assert np.array_equal(order_t[:F + TF].cpu().numpy().view(np.uint64), exp[0])
    rec = cfws.h2_stream_msgs_from_device(msgs_t[:M + T])
    assert rec.tobytes() == exp[2].tobytes()
    pool = torch.empty(len(blob) + 16, dtype=torch.uint8, device="cuda")
    pay = torch.empty(len(blob) + 16 * F + 64, dtype=torch.uint8, device="cuda")
    st, md, ms, tot, m = cfws.h2_deserialize(buf_t, len(blob), order_t[:F], pool, pay)
    assert m == M
    assert (st == cfws.H2_PARSE_COMPLETE).all()
    desc, status, arena = cfws.desc_from_device(md), ms.cpu().numpy(), pay.cpu().numpy()
    got = {}
    for k in range(M):
        dd = desc[k]
        body = arena[int(dd["payload_off"]):int(dd["payload_off"] + dd["payload_size"])].tobytes()
        got.setdefault((int(rec[k]["conn"]), int(rec[k]["stream_id"])), []).append(
            (tuple(int(dd[f]) for f in WS_FIELDS), int(status[k]), body))
    ws_msgs_t, ws_first_t, _, n_ws, _ = cfws.messages_batch(md, ms, conn_first_t=sf_t[:S])
    ws_msgs = cfws.messages_from_device(ws_msgs_t[:n_ws])
    # the tails: whole DATA frames, headers included
    of = of_t[:F + TF].cpu().numpy().view(np.uint32)
    tails = {}
    for r in rec[M:]:
        fr = of[int(r["first"]):int(r["first"] + r["n_data"])]
        tails.setdefault(int(r["conn"]), []).extend(
            (int(f), blob[int(starts[f]):int(starts[f]) + 9 + int(info[f]["length"])]) for f in fr)
    return dict(got=got, rec=rec[:M], ws_msgs=ws_msgs, ws_first=ws_first_t.tolist(), S=S,
                consumed=(consumed_t.cpu().numpy() - begins).tolist(), tails=tails)


def test_end_to_end_many_streams():
    conns = build_connections(21)
    assert sorted({len({s for s, _ in fr if s is not None}) for fr in conns}) == [1, 2, 3, 4]
    t = tick([b"".join(b for _, b in fr) for fr in conns])
    exp = expected_messages(conns)
    assert t["got"] == exp and not t["tails"]
    assert t["consumed"] == [sum(len(b) for _, b in fr) for fr in conns]
    # per stream, the WS fragments joined: messages of 1, 3 and 1 fragments
    n_streams = sum(len({s for s, _ in fr if s is not None}) for fr in conns)
    assert t["S"] == n_streams and len(t["ws_msgs"]) == 3 * n_streams
    assert t["ws_msgs"]["n_fragments"].tolist() == [1, 3, 1] * n_streams
    assert (t["ws_msgs"]["flags"] == cfws.MESSAGE_FINAL).all()
    assert t["ws_first"] == list(range(0, 3 * n_streams, 3))
    assert t["ws_msgs"]["conn"].tolist() == [s for s in range(n_streams) for _ in range(3)]


def test_cut_buffers_and_a_second_tick_that_carries_the_tails():
    """Buffers cut inside a frame: the first tick delivers what END_STREAM
    closed and sets the rest aside as tails; the second tick's buffer is the
    tails' whole DATA frames in arrival order, then the bytes from where the
    walk stopped. Both ticks together deliver what one uncut tick does."""
    conns = build_connections(22)
    whole = [b"".join(b for _, b in fr) for fr in conns]
    rng = np.random.default_rng(3)
    cut_at = [len(w) if c % 3 == 2 else int(rng.integers(10, len(w))) for c, w in enumerate(whole)]
    first = tick([w[:k] for w, k in zip(whole, cut_at)])
    # what the first tick must deliver: the frames that are whole in the cut buffer
    seen = []
    for fr, k in zip(conns, cut_at):
        at, keep = 0, []
        for s, b in fr:
            if at + len(b) <= k:
                keep.append((s, b))
            at += len(b)
        seen.append(keep)
    assert first["consumed"] == [sum(len(b) for _, b in keep) for keep in seen]
    assert first["got"] == expected_messages(seen)
    assert first["tails"] and any(k < len(w) for w, k in zip(whole, cut_at))
    second = tick([b"".join(b for _, b in sorted(first["tails"].get(c, []))) + w[first["consumed"][c]:]
                   for c, w in enumerate(whole)])
    assert not second["tails"]
    both = {}
    for t in (first, second):
        for key, msgs in t["got"].items():
            both.setdefault(key, []).extend(msgs)
    assert both == expected_messages(conns)
