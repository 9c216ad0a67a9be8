"""HTTP/2 receive-buffer frame indexing on the GPU
(cfws_h2_index_frames_batch, include/cfws.h) and the host
receive built on the host walk (cfws_pipeline_h2_receive), each against the
model of tests/h2_index_util.py, which tests/test_h2_index.py pins to the
reference through tests/golden/h2_index_cases.json."""
import random

import numpy as np
import pytest

import h2_index_util as U
import oracle as O
from conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from test_gpu_guard import GuardBuf, _glib  # noqa: E402

FILTERS = [(U.ALL, 0), (U.DATA_ONLY, 0), (U.DATA_ONLY, 1)]


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()


def arena_of(conns, rng, lead=0):
    """Connections (bytes, begin inside the bytes) laid into one arena with
    junk between them: (arena bytes, begin[], end[])."""
    parts, begin, end, at = [bytes([0xEE]) * lead], [], [], lead
    for blob, b in conns:
        begin.append(at + b)
        end.append(at + len(blob))
        gap = bytes([0xEE]) * rng.randrange(0, 13)
        parts += [blob, gap]
        at += len(blob) + len(gap)
    return b"".join(parts), begin, end


def model_batch(arena, begin, end, mf, sel, sid):
    """The expected device outputs: (starts, info, first, consumed, stop)."""
    S, I, first, consumed, stop = [], [], [], [], []
    k = 0
    for b, e in zip(begin, end):
        s, i, c, st = U.expect_h2_index(arena, b, e, mf, sel, sid)
        first.append(k)
        k += len(s)
        S.append(s)
        I.append(i)
        consumed.append(c)
        stop.append(st)
    cat = (lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt))
    return cat(S, np.uint64), cat(I, U.INFO_DTYPE), first, consumed, stop


def check_batch(arena, begin, end, mf, sel, sid, cap=None, buf_t=None, with_info=True):
    """One launch against the model; positions at or past the capacity keep
    their sentinel, in starts and info alike."""
    es, ei, efirst, econs, estop = model_batch(arena, begin, end, mf, sel, sid)
    total = len(es)
    cap = max(total, 1) + 3 if cap is None else cap
    if buf_t is None:
        buf_t = torch.from_numpy(np.frombuffer(arena, np.uint8).copy()).cuda() if arena else \
            torch.zeros(1, dtype=torch.uint8, device="cuda")
    b_t = torch.tensor(begin, dtype=torch.int64, device="cuda")
    e_t = torch.tensor(end, dtype=torch.int64, device="cuda")
    starts_t = torch.full((max(cap, 1),), -1, dtype=torch.int64, device="cuda")[:cap]
    info_t = torch.full((max(cap, 1), 16), 0xEE, dtype=torch.uint8, device="cuda")[:cap] if with_info else None
    _, _, first, consumed, stop, got_total = cfws.h2_index_frames_batch(
        buf_t, b_t, e_t, mf, sel, sid, starts_t=starts_t, info_t=info_t, with_info=with_info)
    torch.cuda.synchronize()
    assert got_total == total
    assert first.cpu().tolist() == efirst
    assert consumed.cpu().tolist() == econs
    assert stop.cpu().tolist() == estop
    w = min(cap, total)
    gs = starts_t.cpu().numpy().view(np.uint64)
    assert np.array_equal(gs[:w], es[:w])
    assert (gs[w:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    if with_info:
        gi = info_t.cpu().numpy()
        assert gi[:w].tobytes() == ei[:w].tobytes()
        assert (gi[w:] == 0xEE).all()
    return total


def test_fixture_blobs_one_connection_each():
    """Every fixture blob as one connection of one arena: one launch per
    max_frame and filter, with d_info."""
    cases = [(c, U.decode_blob(c["blob"])) for c in golden("h2_index_cases.json")]
    rng = random.Random(1)
    for mf in sorted({c["max_frame"] for c, _ in cases}):
        arena, begin, end = arena_of([(b, c["begin"]) for c, b in cases if c["max_frame"] == mf], rng, lead=7)
        for sel, sid in FILTERS:
            check_batch(arena, begin, end, mf, sel, sid)
    # max_frame_size 0 is 16384
    arena, begin, end = arena_of([(b, c["begin"]) for c, b in cases if c["max_frame"] == 16384], rng)
    es = model_batch(arena, begin, end, 16384, U.ALL, 0)
    assert check_batch(arena, begin, end, 0, U.ALL, 0) == len(es[0])


def conn_with_selected(rng, n_selected, cut_tail):
    """A connection with exactly n_selected DATA frames of stream 1 and
    unselected frames (other streams' DATA, control frames) between them."""
    others = [lambda: U.frame(U.T_DATA, 0, 3, rng.randbytes(rng.randrange(0, 9))),
              lambda: U.frame(U.T_PING, 0, 0, rng.randbytes(8)),
              lambda: U.frame(U.T_WINUP, 0, 0, rng.randbytes(4)),
              lambda: U.frame(U.T_SETTINGS, 0, 0, rng.randbytes(6)),
              lambda: U.frame(U.T_HEADERS, 0x4, 1, rng.randbytes(5))]
    parts = []
    for _ in range(n_selected):
        parts += [rng.choice(others)() for _ in range(rng.randrange(0, 3))]
        parts.append(U.frame(U.T_DATA, rng.randrange(2), 1, rng.randbytes(rng.randrange(0, 12))))
    parts += [rng.choice(others)() for _ in range(rng.randrange(0, 3))]
    blob = b"".join(parts)
    if cut_tail:
        blob += U.frame(U.T_DATA, 0, 1, rng.randbytes(20))[:rng.choice([1, 8, 9, 15])]
    return blob


@pytest.fixture(scope="module")
def slot_line():
    rng = random.Random(64)
    counts = [0, 1, 63, 64, 65, 66, 129, 700, 64, 65, 2]
    conns = [(conn_with_selected(rng, k, i % 2 == 1), 0) for i, k in enumerate(counts)]
    return counts, arena_of(conns, rng, lead=3)


def test_slot_line_all_filters(slot_line):
    """Connections around the 64 kept starts, with unselected frames between
    the selected ones (the 65th selected frame is not the 65th frame)."""
    counts, (arena, begin, end) = slot_line
    es = model_batch(arena, begin, end, 16384, U.DATA_ONLY, 1)
    per = np.diff(es[2] + [len(es[0])]).tolist()
    assert per == counts
    all_frames = model_batch(arena, begin, end, 16384, U.ALL, 0)
    assert len(all_frames[0]) > len(es[0]) + 500
    for sel, sid in FILTERS:
        check_batch(arena, begin, end, 16384, sel, sid)
    check_batch(arena, begin, end, 16384, U.DATA_ONLY, 1, with_info=False)


@pytest.mark.parametrize("where", ["inside_first_64", "past_the_64th", "zero", "exact"])
def test_slot_line_capacity(slot_line, where):
    counts, (arena, begin, end) = slot_line
    first = np.concatenate([[0], np.cumsum(counts)])
    c700 = counts.index(700)
    cap = {"inside_first_64": int(first[c700]) + 20, "past_the_64th": int(first[c700]) + 64 + 111,
           "zero": 0, "exact": int(first[-1])}[where]
    check_batch(arena, begin, end, 16384, U.DATA_ONLY, 1, cap=cap)
    check_batch(arena, begin, end, 16384, U.ALL, 0, cap=cap)


@pytest.mark.parametrize("n", [257, 5000])
def test_scan_and_grid_edges(n):
    """257 connections (more than one workgroup) and 5,000 of 0-3 frames
    (more than one 2,048-entry scan block), with empty connections
    (begin == end) among them and the first connection inside the arena."""
    rng = np.random.default_rng(n)
    pr = random.Random(n)
    conns = []
    for c in range(n):
        blob = U.random_buffer(rng, int(rng.integers(0, 4)), quirk=.05, cut=c % 5 == 4, max_payload=12)
        conns.append((blob, len(blob) if c % 11 == 3 else 0))      # begin == end
    arena, begin, end = arena_of(conns, pr, lead=29)
    for sel, sid in FILTERS:
        check_batch(arena, begin, end, 16384, sel, sid)


def test_no_connections_writes_total_only():
    dev = "cuda"
    tot = torch.full((1,), 77, dtype=torch.int64, device=dev)
    first = torch.full((4,), -1, dtype=torch.int64, device=dev)
    starts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(cfws.lib().cfws_h2_index_workspace_size(0), dtype=torch.uint8, device=dev)
    rc = cfws.lib().cfws_h2_index_frames_batch(None, None, None, 0, 0, 0, 0, starts.data_ptr(), None, 4,
                                               first.data_ptr(), None, None, tot.data_ptr(), ws.data_ptr(),
                                               ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(tot.item()) == 0
    assert (first == -1).all() and (starts == -1).all()


def mux_connection(seed, s1_sizes, s3_sizes):
    """One connection's receive buffer with two WS-over-HTTP/2 streams
    (client-masked frames, DATA frames of at most 16,384 bytes) interleaved
    in order, and control frames between them."""
    rng = random.Random(seed)
    streams = []
    for sid, sizes in ((1, s1_sizes), (3, s3_sizes)):
        d = np.zeros(len(sizes), dtype=O.DESC_DTYPE)
        off = 0
        for i, sz in enumerate(sizes):
            d[i] = (off, 0, sz, rng.getrandbits(32), True, 2, True, 0)
            off += sz
        h2, _ = O.h2_serialize_batch(O.fill_splitmix(off + 16, seed + sid, 0), d, sid, 16384)
        idx = [int(x) for x in O.h2_index(h2)] + [len(h2)]
        streams.append([h2[a:b].tobytes() for a, b in zip(idx[:-1], idx[1:])])
    control = [lambda: U.frame(U.T_SETTINGS, 0, 0, rng.randbytes(12)), lambda: U.frame(U.T_SETTINGS, 1, 0),
               lambda: U.frame(U.T_WINUP, 0, rng.choice([0, 1, 3]), rng.randbytes(4)),
               lambda: U.frame(U.T_PING, rng.randrange(2), 0, rng.randbytes(8))]
    parts = [control[0](), U.frame(U.T_HEADERS, 0x4, 1, rng.randbytes(20)), U.frame(U.T_HEADERS, 0x4, 3, rng.randbytes(20))]
    a, b = streams
    while a or b:
        src = a if (a and (not b or rng.random() < .5)) else b
        parts.append(src.pop(0))
        if rng.random() < .5:
            parts.append(rng.choice(control)())
    return b"".join(parts)


# the sizes of h2_echo_digests.json's small case, a 40,000-byte frame that
# spans three DATA frames, and the small sizes a header form changes at
S1_SIZES = [16376, 5, 40000, 0, 16376, 126, 125]
S3_SIZES = [100, 16376, 0, 3000, 16377, 7]


def test_index_feeds_the_h2_receive():
    """DATA + stream id 1 over a multiplexed connection is the index
    cfws_h2_deserialize_batch takes: its result equals the oracle's on the
    same buffer with the model's index."""
    assert golden("h2_echo_digests.json")[0]["payload"] == S1_SIZES[0]
    blob = mux_connection(8441, S1_SIZES, S3_SIZES)
    buf = np.frombuffer(blob, np.uint8)
    es, ei, consumed, stop = U.expect_h2_index(blob, 0, len(blob), 16384, U.DATA_ONLY, 1)
    assert stop == U.COMPLETE and len(es) == 9                 # the 40,000-byte frame spans three
    h2_t = torch.from_numpy(buf.copy()).cuda()
    b_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    e_t = torch.full((1,), len(blob), dtype=torch.int64, device="cuda")
    starts_t, info_t, first, cons, st, total = cfws.h2_index_frames_batch(h2_t, b_t, e_t, 16384, U.DATA_ONLY, 1)
    assert total == len(es) and int(cons[0]) == consumed and int(st[0]) == stop
    assert np.array_equal(starts_t[:total].cpu().numpy().view(np.uint64), es)
    info = cfws.h2_info_from_device(info_t[:total])
    assert info.tobytes() == ei.tobytes() and info["flags"][-1] & U.F_END_STREAM
    e = O.h2_deserialize_batch(buf, es, 16384)
    pool = torch.empty(len(blob), dtype=torch.uint8, device="cuda")
    pay = torch.full((len(blob) + 16 * total + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    h2s, md, ms, tot, m = cfws.h2_deserialize(h2_t, len(blob), starts_t[:total], pool, pay)
    torch.cuda.synchronize()
    assert m == e["n_msg"] == len(S1_SIZES) and int(tot.item()) == e["total"]
    assert np.array_equal(h2s.cpu().numpy(), e["h2_status"]) and np.array_equal(ms.cpu().numpy(), e["msg_status"])
    gd = cfws.desc_from_device(md)
    for f in ("payload_off", "wire_off", "payload_size", "mask_key", "fin", "opcode", "mask", "header_size"):
        assert np.array_equal(gd[f], e["msg_desc"][f]), f
    assert gd["payload_size"].tolist() == S1_SIZES
    assert np.array_equal(pay[:e["total"]].cpu().numpy(), e["payload"][:e["total"]])


def test_guarded_arena_reads_only_the_connections():
    """An exact arena flush against an unmapped range, the last connection
    ending on the arena's last byte (and one flush against an unmapped range
    before its start): a read outside the arena faults."""
    torch.cuda.synchronize()
    if not _glib().guard_supported():
        pytest.skip("no HIP virtual memory management on this device")
    rng = random.Random(950)
    conns = [(conn_with_selected(rng, k, cut), 0) for k, cut in ((3, True), (70, False), (0, True), (66, True))]
    arena, begin, end = arena_of(conns, rng)
    arena = arena[:end[-1]]                                # ends with the last connection's last byte
    assert begin[0] == 0
    # guard before the start: the first connection begins on the arena's first byte
    g = GuardBuf(len(arena), False).upload(np.frombuffer(arena, np.uint8))
    try:
        for sel, sid in FILTERS:
            check_batch(arena, begin, end, 16384, sel, sid, buf_t=g)
    finally:
        torch.cuda.synchronize()
        g.free()
    # guard after the end: round16(n) == n, so the mapped end is the arena's end
    pad = -len(arena) % 16
    arena = bytes([0xEE]) * pad + arena
    begin, end = [b + pad for b in begin], [e + pad for e in end]
    assert end[-1] == len(arena) and len(arena) % 16 == 0
    g = GuardBuf(len(arena), True).upload(np.frombuffer(arena, np.uint8))
    try:
        for sel, sid in FILTERS:
            check_batch(arena, begin, end, 16384, sel, sid, buf_t=g)
    finally:
        torch.cuda.synchronize()
        g.free()


def test_argument_errors_write_nothing():
    blob = U.frame(U.T_DATA, 1, 1, b"abc") * 3
    buf = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    b_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    e_t = torch.full((1,), len(blob), dtype=torch.int64, device="cuda")
    L = cfws.lib()
    ws = torch.empty(L.cfws_h2_index_workspace_size(1), dtype=torch.uint8, device="cuda")
    outs = {k: torch.full((8,), -1, dtype=dt, device="cuda")
            for k, dt in (("starts", torch.int64), ("first", torch.int64), ("consumed", torch.int64),
                          ("stop", torch.int32), ("total", torch.int64))}
    info = torch.full((8 * 16 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert info.data_ptr() % 16 == 0

    def call(select=0, info_ptr=info.data_ptr(), ws_size=ws.numel(), **null):
        p = {k: (None if k in null else v.data_ptr()) for k, v in outs.items()}
        return L.cfws_h2_index_frames_batch(buf.data_ptr(), b_t.data_ptr(), e_t.data_ptr(), 1, 0, select, 0,
                                            p["starts"], info_ptr, 8, p["first"], p["consumed"], p["stop"],
                                            p["total"], None if "ws" in null else ws.data_ptr(), ws_size, None)

    INVALID, WORKSPACE = -1, -2
    assert call(info_ptr=info.data_ptr() + 8) == INVALID
    assert call(info_ptr=info.data_ptr() + 1) == INVALID
    assert call(ws_size=ws.numel() - 1) == WORKSPACE
    assert call(ws_size=0) == WORKSPACE
    assert call(select=2) == INVALID
    for name in ("starts", "first", "consumed", "stop", "total", "ws"):
        assert call(**{name: True}) == INVALID, name
    assert b"h2 index" in L.cfws_last_error()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert (v == -1).all(), k
    assert (info == 0xEE).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert int(outs["total"][0]) == 3 and outs["starts"][:3].tolist() == [0, 12, 24]


def _pinned(data: bytes):
    t = torch.zeros(max(len(data), 16), dtype=torch.uint8, pin_memory=True)
    t.numpy()[:len(data)] = np.frombuffer(data, np.uint8)
    return t


def _same_receive(got, e, n_frames):
    st, md, ms, consumed, stop, tot = got
    assert len(st) == n_frames and np.array_equal(st, e["h2_status"])
    assert len(md) == e["n_msg"] and tot == e["total"] and np.array_equal(ms, e["msg_status"])
    for f in ("payload_off", "wire_off", "payload_size", "mask_key", "fin", "opcode", "mask", "header_size"):
        assert np.array_equal(md[f], e["msg_desc"][f]), f


def test_pipeline_h2_receive_whole_and_resumed():
    """cfws_pipeline_h2_receive on one multiplexed host buffer that ends
    inside a frame: once whole, once with a capacity that gives
    CFWS_INDEX_FULL (at a message boundary) and a resume from *consumed."""
    blob = mux_connection(77, S1_SIZES, S3_SIZES) + U.frame(U.T_DATA, 0, 1, b"x" * 50)[:30]
    buf = np.frombuffer(blob, np.uint8)
    es, ei, consumed, stop = U.expect_h2_index(blob, 0, len(blob), 16384, U.DATA_ONLY, 1)
    assert stop == U.MORE_DATA and len(es) == 9
    h2_t = _pinned(blob)
    cap = len(blob) + 16 * len(es) + 64
    out_t = torch.zeros(cap, dtype=torch.uint8, pin_memory=True)
    pl = cfws.Pipeline(chunk_bytes=1 << 18, max_frames=4096, depth=2)
    try:
        got = pl.h2_receive(h2_t.data_ptr(), 0, len(blob), out_t.data_ptr(), cap, max_frames=100, sid=1)
        e = O.h2_deserialize_batch(buf[:consumed], es, 16384, O.DEFAULT_MAX_PAYLOAD, 16, None, cap)
        assert got[3:5] == (consumed, stop)
        _same_receive(got, e, len(es))
        assert got[1]["payload_size"].tolist() == S1_SIZES
        assert np.array_equal(out_t.numpy()[:e["total"]], e["payload"][:e["total"]])

        # the first 5 DATA frames end message 3 (16376 | 5 | 40000 over three)
        k = 5
        assert ei["flags"][k - 1] & U.F_END_STREAM
        p1 = U.expect_h2_index(blob, 0, len(blob), 16384, U.DATA_ONLY, 1, max_starts=k)
        assert p1[3] == U.INDEX_FULL and p1[2] == int(es[k])
        got1 = pl.h2_receive(h2_t.data_ptr(), 0, len(blob), out_t.data_ptr(), cap, max_frames=k, sid=1)
        e1 = O.h2_deserialize_batch(buf[:p1[2]], p1[0], 16384, O.DEFAULT_MAX_PAYLOAD, 16, None, cap)
        assert got1[3:5] == (p1[2], U.INDEX_FULL)
        _same_receive(got1, e1, k)
        assert np.array_equal(out_t.numpy()[:e1["total"]], e1["payload"][:e1["total"]])
        got2 = pl.h2_receive(h2_t.data_ptr(), got1[3], len(blob), out_t.data_ptr(), cap, max_frames=100, sid=1)
        e2 = O.h2_deserialize_batch(buf[:consumed], es[k:], 16384, O.DEFAULT_MAX_PAYLOAD, 16, None, cap)
        assert got2[3:5] == (consumed, stop)
        _same_receive(got2, e2, len(es) - k)
        assert np.array_equal(out_t.numpy()[:e2["total"]], e2["payload"][:e2["total"]])
        assert got1[1]["payload_size"].tolist() + got2[1]["payload_size"].tolist() == S1_SIZES
    finally:
        pl.close()
