"""UTF-8 check of received text messages on the GPU
(cfws_utf8_messages_batch, include/cfws.h) against the model
of tests/utf8_util.py (CPython's strict decoder), which
tests/test_utf8_host.py pins the host form to. Every call runs with the
outputs filled with a sentinel, two rows behind each capacity, and the
workspace with 0xAA."""
import numpy as np
import pytest

import oracle as O
import utf8_util as U

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from coldforce_amd import workloads as W  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()


def P():
    return cfws.lib().cfws_utf8_piece_bytes()


def up(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).cuda()


def arena_t(arena):
    """The arena's bytes on the device, readable to round16."""
    a = np.frombuffer(arena, np.uint8) if isinstance(arena, (bytes, bytearray)) else arena
    t = torch.zeros(W.round16(len(a)) + 16, dtype=torch.uint8, device="cuda")
    t[:len(a)] = up(a)
    return t


class Call:
    """One cfws_utf8_messages_batch call's device buffers: sentinel-filled
    outputs with two rows behind each capacity, a 0xAA workspace. payload: a
    device tensor (or anything with data_ptr())."""

    def __init__(self, payload, payload_bytes, rows, carry=None, cap=None, ws_t=None):
        self.payload, self.pb, self.n = payload, payload_bytes, len(rows)
        self.cap = self.n if cap is None else cap
        self.msgs = up(np.ascontiguousarray(rows, cfws.MESSAGE_DTYPE).view(np.uint8).reshape(-1, 32)) if self.n else \
            torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
        self.carry = None if carry is None else up(np.asarray(carry, np.uint32)[:max(self.n, 1)].view(np.int32), np.int32)
        self.result = torch.full((self.n + 2, 16), 0xEE, dtype=torch.uint8, device="cuda")
        self.bad = torch.full((self.cap + 2,), -1, dtype=torch.int32, device="cuda")
        self.counts = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        size = cfws.lib().cfws_utf8_workspace_size(self.n)
        self.ws = ws_t if ws_t is not None else torch.empty(size, dtype=torch.uint8, device="cuda")
        assert self.ws.numel() >= size
        self.ws.fill_(0xAA)

    def launch(self, **over):
        a = dict(payload=self.payload.data_ptr(), msgs=self.msgs.data_ptr(),
                 carry=None if self.carry is None else self.carry.data_ptr(), result=self.result.data_ptr(),
                 bad=self.bad.data_ptr(), counts=self.counts.data_ptr(), ws=self.ws.data_ptr(), ws_size=self.ws.numel(),
                 n=self.n)
        a.update(over)
        return cfws.lib().cfws_utf8_messages_batch(a["payload"], self.pb, a["msgs"], a["n"], a["carry"], a["result"],
                                                   a["bad"], self.cap, a["counts"], a["ws"], a["ws_size"], None)

    def rows(self):
        torch.cuda.synchronize()
        return cfws.utf8_results_from_device(self.result[:self.n])

    def check(self, exp, what=""):
        res, bad, checked, n_bad = exp
        got = self.rows()
        assert self.counts.tolist() == [checked, n_bad, -1, -1], what
        U.same_rows(got, res, what)
        assert (self.result[self.n:] == 0xEE).all(), what
        k = min(self.cap, n_bad)
        b = self.bad.cpu().numpy()
        assert np.array_equal(b[:k].view(np.uint32), bad[:k]) and (b[k:] == -1).all(), what
        return got

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.result == 0xEE).all() and (self.bad == -1).all() and (self.counts == -1).all() and
                    (self.ws == 0xAA).all())


def run(arena, rows, carry=None, exp=None, cap=None, what="", payload_bytes=None):
    pb = len(arena) if payload_bytes is None else payload_bytes
    exp = U.model(arena, rows, carry, payload_bytes=pb) if exp is None else exp
    c = Call(arena_t(arena), pb, rows, carry, cap)
    assert c.launch() == 0, cfws.lib().cfws_last_error()
    c.check(exp, what)
    return exp


# ---- 1: the exhaustive short strings ------------------------------------------------

def test_every_short_string_over_the_alphabet():
    arena, rows, exp = U.exhaustive()
    run(arena, rows, exp=exp, what="exhaustive")
    h = cfws.utf8_check_messages(arena, rows)
    U.same_rows(h[0], exp[0], "host")
    assert np.array_equal(h[1], exp[1]) and h[2:] == exp[2:]


# ---- 2: lanes, pieces, waves, workgroups -----------------------------------------------

def test_probes_across_every_boundary():
    """Each probe written over a valid text at every offset of [b - 4, b + 1]
    for b at a chunk, a piece, two pieces, a wave's and a workgroup's bytes
    from the message's first chunk, the message starting 0, 1 and 15 bytes
    into its chunk; all variants are messages of one call. A message takes 17
    pieces, so that the messages' first pieces fall on every phase of the
    wave and of the workgroup."""
    L = cfws.lib()
    p, w, b = P(), L.cfws_utf8_wave_bytes(), L.cfws_utf8_workgroup_bytes()
    assert (p, w, b) == (256, 1024, 4096)
    n = max(3 * p, b) + 40
    base = U.valid_text(np.random.default_rng(2), n, (2, 3, 4))
    slot = W.round16(n) + 32
    parts, offs = [], []
    for r in (0, 1, 15):
        for edge in (16, p, 2 * p, w, b):
            for d in range(-4, 2):
                for probe in U.PROBES:
                    at = edge + d - r                              # in the message; edge counts from its chunk
                    if at < 0:
                        continue
                    s = bytearray(base)
                    s[at:at + len(probe)] = probe
                    offs.append(len(parts) * slot + r)
                    parts.append(b"\0" * r + bytes(s[:n]) + b"\0" * (slot - n - r))
    arena = b"".join(parts)
    rows = U.rows_of(offs, np.full(len(offs), n))
    exp = run(arena, rows, what="boundaries")
    kinds = exp[0]["flags"]
    assert (kinds & U.VALID != 0).any() and (kinds & U.INVALID != 0).any()


# ---- 3: sizes ------------------------------------------------------------------------------

def forms_of(rng, n):
    """A size's forms: valid, bad only in its last byte, bad only in its
    first, all ASCII, all 4-byte characters."""
    if n == 0:
        return [b""]
    v = bytearray(U.valid_text(rng, n))
    last, first = bytearray(v), bytearray(v)
    last[-1], first[0] = 0xFF, 0x80
    if n > 1 and (first[1] & 0xC0) == 0x80:                         # the first character was longer: keep the rest valid
        first = bytearray(b"\x80" + U.valid_text(rng, n - 1))
    return [bytes(v), bytes(last), bytes(first), b"a" * n, U.valid_text(rng, n, (4,))]


def test_small_sizes():
    rng = np.random.default_rng(3)
    p = P()
    strings = [s for n in (0, 1, 15, 16, 17, p - 1, p, p + 1) for s in forms_of(rng, n)]
    for base in (0, 5, 15):
        arena, rows = U.pack(strings, base=base)
        run(arena, rows, what=f"sizes from {base}")


def test_eight_mib_messages():
    """8 MiB + 3 bytes in each form, and bad at two places a workgroup's
    stride apart and more: the smaller position wins."""
    rng = np.random.default_rng(4)
    n = (8 << 20) + 3
    strings = forms_of(rng, n)
    two = bytearray(strings[0])
    two[(5 << 20) + 7], two[(1 << 20) + 3] = 0xFF, 0xFF
    strings.append(bytes(two))
    arena, rows = U.pack(strings, base=3)
    exp = run(arena, rows, what="8 MiB")
    f, pre = exp[0]["flags"], exp[0]["prefix"]
    assert f[0] == U.CHECKED | U.VALID and pre[0] == n and pre[2] == 0 and f[3] == f[4] == f[0]
    assert f[1] & U.BAD and n - 4 <= pre[1] < n and f[5] & U.BAD and (1 << 20) <= pre[5] <= (1 << 20) + 3


# ---- 4: message counts around the table pass's group -----------------------------------------

@pytest.mark.parametrize("which", ["1", "G-1", "G", "G+1", "3G+1"])
def test_message_counts_around_the_group(which):
    g = cfws.messages_group_frames()
    n = {"1": 1, "G-1": g - 1, "G": g, "G+1": g + 1, "3G+1": 3 * g + 1}[which]
    tiny = [U.CHARS[1], b"ok", b"\xc3", U.CHARS[2] + b"!", b"", b"\xe2\x28\xa1"]        # every third one is bad
    arena, rows = U.pack([tiny[i % 6] for i in range(n)])
    exp = run(arena, rows, what=which)
    assert exp[1].tolist() == list(range(2, n, 3))
    for cap in (0, 1, exp[3] + 1):
        run(arena, rows, exp=exp, cap=cap, what=(which, cap))


# ---- 5, 7: selection, and arenas between unmapped ranges ---------------------------------------

@pytest.fixture
def guards():
    import test_gpu_guard as TG
    if not TG._glib().guard_supported():
        pytest.skip("no HIP virtual memory management on this device")
    bufs = []

    def make(data, flush_end):
        b = TG.GuardBuf(len(data), flush_end, 0xEE)
        b.upload(np.frombuffer(data, np.uint8))
        bufs.append(b)
        return b
    yield make
    torch.cuda.synchronize()
    for b in bufs:
        b.free()


def test_selection_over_a_guarded_arena(guards):
    """The rows of the host test's selection case; the unchecked ranges lie
    past the arena, which ends at an unmapped range."""
    arena, rows, carry = U.selection_case()
    for cin, pb in ((carry, len(arena)), (None, len(arena)), (carry, len(arena) - 1)):
        c = Call(guards(arena, True), pb, rows, cin)
        assert c.launch() == 0, cfws.lib().cfws_last_error()
        c.check(U.model(arena, rows, cin, payload_bytes=pb), f"selection {cin is None} {pb}")


@pytest.mark.parametrize("flush_end", [False, True])
def test_arena_flush_against_unmapped_ranges(guards, flush_end):
    """The first message starts at the arena's byte 0 with a continuation
    byte (no look-behind before the arena, which begins at an unmapped range);
    the last ends at the arena's final byte with a truncated lead (the arena
    is readable to round16 and not a byte further)."""
    rng = np.random.default_rng(7)
    p = P()
    strings = [b"\xac" + U.valid_text(rng, 3 * p + 5), U.valid_text(rng, 33), U.valid_text(rng, 4 * p - 1) + b"\xf0\x9f"]
    if flush_end:
        strings.append(U.valid_text(rng, 30 - sum(len(s) for s in strings) % 16) + b"\xe2\x82")
    arena, rows = U.pack(strings)
    assert not flush_end or len(arena) % 16 == 0
    c = Call(guards(arena, flush_end), len(arena), rows)
    assert c.launch() == 0, cfws.lib().cfws_last_error()
    got = c.check(U.model(arena, rows), f"flush_end {flush_end}")
    assert got["flags"][0] & U.INVALID and got["prefix"][0] == 0 and got["flags"][-1] == U.CHECKED | U.TRUNCATED | U.BAD


# ---- 6: refusals, workspace reuse ------------------------------------------------------------------

def test_argument_errors_write_nothing():
    arena, rows, carry = U.selection_case()
    c = Call(arena_t(arena), len(arena), rows, carry, cap=4)
    L = cfws.lib()
    INVALID, WORKSPACE = -1, -2
    assert c.launch(result=c.result.data_ptr() + 8) == INVALID
    assert b"16-byte" in L.cfws_last_error()
    assert c.launch(payload=c.payload.data_ptr() + 4) == INVALID
    assert c.launch(ws_size=c.ws.numel() - 1) == WORKSPACE
    assert c.launch(ws_size=0) == WORKSPACE
    for name in ("msgs", "result", "payload", "bad", "counts", "ws"):
        assert c.launch(**{name: None}) == INVALID, name
    assert b"utf8" in L.cfws_last_error()
    assert c.launch(n=1 << 32) == INVALID
    assert c.untouched()
    assert c.launch() == 0
    c.check(U.model(arena, rows, carry, bad_capacity=4))


def test_no_messages_writes_two_zero_counts():
    c = Call(arena_t(b"abc"), 3, U.rows_of([], []))
    assert c.launch(msgs=None, result=None, bad=None) == 0
    torch.cuda.synchronize()
    assert c.counts.tolist() == [0, 0, -1, -1] and (c.result == 0xEE).all() and (c.ws == 0xAA).all()


def test_two_batches_through_one_workspace():
    g = cfws.messages_group_frames()
    rng = np.random.default_rng(6)
    a = U.pack([U.valid_text(rng, int(k)) + (b"\xff" if k % 5 == 0 else b"") for k in rng.integers(0, 700, 2 * g + 17)])
    b = U.pack([p + U.valid_text(rng, 300) for p in U.PROBES], base=9)
    ws = torch.empty(cfws.lib().cfws_utf8_workspace_size(len(a[1])), dtype=torch.uint8, device="cuda")
    ea, eb = U.model(*a), U.model(*b)
    ca = Call(arena_t(a[0]), len(a[0]), a[1], ws_t=ws)
    cb = Call(arena_t(b[0]), len(b[0]), b[1], ws_t=ws)
    assert ca.launch() == 0 and cb.launch() == 0 and ca.launch() == 0       # back to back, same stream
    cb.check(eb, "second")
    ca.check(ea, "first, again after the second")


def test_rows_may_repeat_and_overlap():
    """Overlapping rows make more pieces than the arena has: the grid strides."""
    rng = np.random.default_rng(8)
    text = U.valid_text(rng, 70000) + b"\xe2\x82"
    offs = np.array([0, 0, 1, 100, 0, 69000] * 20, dtype=np.uint64)
    rows = U.rows_of(offs, len(text) - offs)
    run(text, rows, what="overlap")


# ---- 8: offsets across 2^32 --------------------------------------------------------------------------

def test_offsets_across_two_to_the_32():
    """One relocation case (tests/wide_util.py's constants): the small
    problem's window lies at [2^32 - delta, ...) of an arena of 2^32 + 4 MiB;
    messages wholly below the mark, wholly above, and one that contains byte
    2^32 with a probe on each side of the mark. The rows equal the small
    problem's."""
    import wide_util as WU
    rng = np.random.default_rng(32)
    delta = WU.DELTAS["odd16"] + 5
    sizes = [int(k) for k in rng.integers(0, 3000, 300)]
    strings = [U.valid_text(rng, k) + (U.PROBES[i % len(U.PROBES)] if i % 4 == 0 else b"") for i, k in enumerate(sizes)]
    arena, rows = U.pack(strings)
    m = int(np.nonzero(rows["payload_off"] + rows["payload_size"] > delta)[0][0])       # holds byte 2^32
    a, z = int(rows["payload_off"][m]), int(rows["payload_off"][m] + rows["payload_size"][m])
    assert a < delta - 8 and z > delta + 8
    base = WU.MARK - delta
    big = WU.sentinel_arena(WU.ARENA_BYTES)
    for probe_at in (delta + 2, delta - 5):
        s = bytearray(arena)
        s[a:z] = U.valid_text(rng, delta - 5 - a) + b"abcdefghij" + U.valid_text(rng, z - delta - 5)
        s[probe_at:probe_at + 2] = b"\xc0\x80"
        small = bytes(s)
        assert len(small) == len(arena)
        exp = U.model(small, rows)
        assert exp[0]["prefix"][m] == probe_at - a
        WU.put(big, base, np.frombuffer(small, np.uint8))
        moved = rows.copy()
        moved["payload_off"] += np.uint64(base)
        cross = WU.crossing(moved["payload_off"], moved["payload_size"])
        assert WU.crosses(cross) and m in cross["inside"]
        c = Call(big, base + len(small), moved)
        assert c.launch() == 0, cfws.lib().cfws_last_error()
        c.check(exp, f"wide, probe at 2^32 {probe_at - delta:+d}")
    del big, c
    torch.cuda.synchronize()


# ---- 9: end to end --------------------------------------------------------------------------------------

def wire_of(frames, seed):
    """Client-masked wire bytes of (opcode, fin, payload bytes) frames."""
    return b"".join(O.serialize_keyed(bool(fin), op, True, 0x9E3779B9 + 77 * (seed + i), data)
                    for i, (op, fin, data) in enumerate(frames))


def fragments(rng, op, data, k):
    """data as k frames, cut anywhere (inside characters too)."""
    cuts = sorted(int(c) for c in rng.integers(0, len(data) + 1, k - 1))
    parts = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    return [(op if i == 0 else U.CONT, 1 if i == k - 1 else 0, part) for i, part in enumerate(parts)]


def tick(buffers):
    """Index -> reassembling receive -> messages, on the device: (msgs_t, host
    rows, arena tensor, its bytes)."""
    blob = b"".join(buffers)
    ends = np.cumsum([len(b) for b in buffers])
    begin_t = torch.from_numpy((ends - [len(b) for b in buffers]).astype(np.int64)).cuda()
    end_t = torch.from_numpy(ends.astype(np.int64)).cuda()
    buf_t = arena_t(blob)
    starts_t, first_t, consumed_t, _, total = cfws.index_frames_batch(buf_t, begin_t, end_t)
    assert consumed_t.tolist() == ends.tolist()
    out = torch.full((W.round16(len(blob)) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d2, st, _ = cfws.deserialize(buf_t, len(blob), starts_t[:total], out, flags=cfws.DESERIALIZE_REASSEMBLE)
    msgs_t, _, _, m, _ = cfws.messages_batch(d2, st, conn_first_t=first_t)
    return msgs_t[:m], cfws.messages_from_device(msgs_t[:m]), out


def verdicts(msgs_t, out, carry=None):
    c = Call(out, out.numel(), np.zeros(msgs_t.shape[0], cfws.MESSAGE_DTYPE), carry)
    c.msgs = msgs_t.contiguous()
    assert c.launch() == 0, cfws.lib().cfws_last_error()
    got = c.rows()
    return got, c.bad.cpu().numpy()[:int(c.counts[1])].tolist(), c.counts.tolist()[:2]


def test_end_to_end_over_two_ticks():
    """About 200 text and binary messages of 1-4 fragments over three
    connections, a few with probes, masked -> indexed -> received with
    REASSEMBLE -> cfws_messages_batch -> this call; the expected verdicts are
    the decoder's on the joined payloads. Two connections end inside a
    character of an unfinished text message; the next tick brings the rest,
    checked with the first tick's carry."""
    rng = np.random.default_rng(9)
    bufs, want = [[], [], []], [[], [], []]
    for i in range(200):
        text = i % 3 != 2
        data = U.valid_text(rng, int(rng.integers(0, 900)), (1, 2, 3, 4)) if text else rng.bytes(int(rng.integers(0, 900)))
        if text and i % 10 == 0:
            at = int(rng.integers(0, len(data) + 1))
            data = data[:at] + U.PROBES[(i // 10) % len(U.PROBES)] + data[at:]
        c = i % 3 if i < 190 else 0
        bufs[c] += fragments(rng, U.TEXT if text else U.BINARY, data, int(rng.integers(1, 5)))
        want[c].append((text, data, U.FINAL))
    # connections 1 and 2 end with an unfinished text message cut inside a character
    tails = []
    for c, cut in ((1, 2), (2, 1)):
        data = U.valid_text(rng, 400, (3, 4)) + U.CHARS[2] + U.valid_text(rng, 300, (2, 3))
        bufs[c] += [(U.TEXT, 0, data[:150]), (U.CONT, 0, data[150:400 + cut])]
        want[c].append((True, data[:400 + cut], U.OPEN))
        tails.append(data[400 + cut:])
    msgs_t, rows, out = tick([wire_of(b, 1000 * c) for c, b in enumerate(bufs)])
    flat = [w for c in want for w in c]
    assert len(rows) == len(flat) and rows["flags"].tolist() == [w[2] for w in flat]
    got, bad, counts = verdicts(msgs_t, out)
    exp_bad = []
    for m, (text, data, end) in enumerate(flat):
        if not text:
            assert got[m].tobytes() == bytes(16), m
            continue
        start, kind = U.classify(data)
        is_bad = kind == U.INVALID or (kind == U.TRUNCATED and end != U.OPEN)
        assert got["flags"][m] == U.CHECKED | kind | (U.BAD if is_bad else 0) and got["prefix"][m] == start, m
        exp_bad += [m] if is_bad else []
    assert bad == exp_bad and len(exp_bad) > 5 and counts == [sum(w[0] for w in flat), len(exp_bad)]
    opens = [m for m, w in enumerate(flat) if w[2] == U.OPEN]
    assert [got["flags"][m] for m in opens] == [U.CHECKED | U.TRUNCATED] * 2
    assert [(int(got["carry"][m]) >> 24) for m in opens] == [2, 1]
    # the next tick: each connection's buffer begins with the CONTINUATION frames
    nxt = [[(U.BINARY, 1, b"\xff\xfe")], fragments(rng, U.CONT, tails[0], 2), fragments(rng, U.CONT, tails[1], 3)]
    nxt[1].append((U.TEXT, 1, U.CHARS[0]))
    msgs_t, rows, out = tick([wire_of(b, 5000 + c) for c, b in enumerate(nxt)])
    assert rows["flags"].tolist() == [U.FINAL, U.HEADLESS | U.FINAL, U.FINAL, U.HEADLESS | U.FINAL]
    carry = np.zeros(4, dtype=np.uint32)
    carry[1], carry[3] = (int(got["carry"][m]) | U.CARRY_TEXT for m in opens)
    got2, bad2, counts2 = verdicts(msgs_t, out, carry)
    assert bad2 == [] and counts2 == [3, 0] and got2["flags"].tolist() == [0] + [U.CHECKED | U.VALID] * 3
    assert got2["prefix"].tolist() == [0, len(tails[0]), 2, len(tails[1])]
    # without the carry the same tails begin inside a character
    got3, bad3, _ = verdicts(msgs_t, out, np.array([0, U.CARRY_TEXT, 0, U.CARRY_TEXT], dtype=np.uint32))
    assert bad3 == [1, 3] and got3["prefix"].tolist() == [0, 0, 2, 0]
