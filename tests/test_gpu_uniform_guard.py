"""cfws_serialize_uniform and cfws_deserialize_slots_uniform over guarded
arenas (tests/native/guardmem.cpp, as test_gpu_guard.py and
test_gpu_slots.py run every other batch entry point): each arena is exact
and flush against an unmapped range, after its round16(size) end or before
its start, so one byte read or written outside it faults at once. Every
case is also compared with the oracle, byte for byte.

Why the send stays inside (cfws_uniform.hip, read before these ran; the
contract is "an arena is readable to round16 of its size, the keys to 4 n
bytes"): every chunk the kernels work on starts below min(total, capacity)
or, in the small kernel, below total, so its frame f is below n.
  * Body blocks A and B (both kernels): A is the aligned block holding the
    chunk's first payload byte; B is loaded only when the chunk's own last
    payload byte lies in it (ph != 0, and for a tail chunk ph + (W - off) >
    16). A block that holds a byte of [0, n fs) ends at or before
    round16(n fs) and starts at or after 0.
  * The small kernel's loads go through a buffer resource of 0x7ffffff0
    bytes from frame F0's payload: the range checks nothing inside the arena,
    the offsets do -- (q fs + off - hs) & ~15 of a live chunk of frame F0 + q
    < n, + 16 under the rule above; unwanted loads get the offset
    0x7ffffff0, which is out of the resource's range and reads zeros without
    an access. hx is the first block of frame F0 + q (its header starts the
    span's last chunk) or of F0 + q + 1, which the kernel checks to be < n.
  * The key window is a resource of min(4 (n - F0), 512) bytes at keys + F0:
    lanes past it read zeros without an access; q + 1 <= 109 < 128.
  * header_prep (general kernel): block A holds s_lo, a payload byte of
    frame f, or of f + 1 when that is < n (`next`); B only when ph + npay >
    16, the block of the chunk's last payload byte. keys[f + 1] only under
    `next`. The header lanes' frame is hD / W with hD < min(total, cap).
  * The byte kernel re-reads keys[f] after ++f only while D + j < total, so
    the byte belongs to frame f < n.
Stores are whole chunks at D + 16 <= capacity, single bytes below the
capacity otherwise.

The receive computes its own starts (i * stride): a start at or past
wire_size loads nothing (`wo < wire_size && blk < wire_size`, the 16 header
bytes only at wl <= wire_size - 16), as with an index entry past the wire
in test_gpu_slots.py."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from coldforce_amd import workloads as W  # noqa: E402
from test_gpu_guard import GuardBuf, _glib, _seed21_batch  # noqa: E402
from test_gpu_slots import expect_slots  # noqa: E402
from test_gpu_uniform import _frames  # noqa: E402
import test_uniform_cover as cover  # noqa: E402

SENT = 0xEE


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()
    torch.cuda.synchronize()
    if not _glib().guard_supported():
        pytest.skip("no HIP virtual memory management on this device")
    return torch.device("cuda", 0)


@pytest.fixture
def guards():
    bufs = []

    def make(n, flush_end=True):
        b = GuardBuf(n, flush_end, SENT)
        bufs.append(b)
        return b
    yield make
    torch.cuda.synchronize()
    for b in bufs:
        b.free()


SEND = [(fs, 1) for fs in (5, 26, 32, 100, 112, 256, 1000, 1024, 4096, 65520, 65536)] + \
       [(fs, 0) for fs in (32, 256, 1000)]


@pytest.mark.parametrize("flush_end", [True, False], ids=["end", "start"])
@pytest.mark.parametrize("fs,mask", SEND)
def test_guard_uniform_send(guards, fs, mask, flush_end):
    """The three send kernels with the payload in exactly n fs bytes, the
    keys in exactly 4 n and the wire in exactly the capacity: the whole
    batch, and a cut inside it."""
    n = cover.frames_for(fs, mask)
    payload, keys, d = _frames(n, fs, mask, 1, 2, fs + mask)
    exp, _ = O.serialize_batch(payload, d)
    total = len(exp)
    pay = guards(n * fs, flush_end).upload(payload)
    keys_b = guards(4 * n, flush_end).upload(keys.view(np.uint8)) if mask else None
    for cap in (total, total // 2 + 3):
        wire = guards(cap, flush_end)
        tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        cfws.serialize_uniform(pay, keys_b, n, fs, wire, fin=True, opcode=2, mask=bool(mask), total_t=tot,
                               wire_capacity=cap)
        torch.cuda.synchronize()
        assert int(tot.item()) == total
        got = wire.download()
        bad = np.nonzero(got[:cap] != exp[:cap])[0]
        assert bad.size == 0, f"cap {cap}: {bad.size} wire bytes differ, first at {bad[:8]}"
        assert (got[cap:] == SENT).all(), "written past the wire capacity"


def _recv_guarded(guards, wire, wire_size, n, stride, slot, cap, flush_end):
    """cfws_deserialize_slots_uniform from a wire of exactly wire_size bytes
    into an arena of exactly cap and info of exactly 8 n, against the slot
    receive's expectation over the starts i * stride
    (test_gpu_uniform._recv's); returns the mismatch count."""
    w = guards(max(wire_size, 1), flush_end).upload(wire[:wire_size])
    out = guards(max(cap, 1), flush_end)
    info = guards(8 * n, flush_end)
    mm = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    _, tot = cfws.deserialize_slots_uniform(w, wire_size, n, stride, out, slot, info, mismatch_t=mm,
                                            payload_capacity=cap)
    torch.cuda.synchronize()
    starts = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    e_arena, e_d, e_st, e_tot = expect_slots(wire, wire_size, starts, slot, cap)
    assert int(tot.item()) == e_tot
    fi = info.download()[:8 * n].view(cfws.INFO_DTYPE)
    st = fi["status"].astype(np.int32)
    bad = np.nonzero(st != e_st)[0]
    assert bad.size == 0, f"{bad.size} statuses differ, first {[(int(i), int(st[i]), int(e_st[i])) for i in bad[:6]]}"
    assert np.array_equal(fi["payload_size"], np.minimum(e_d["payload_size"], np.uint64(0xFFFFFFFF)).astype(np.uint32))
    ok = e_st == O.PARSE_COMPLETE
    assert np.array_equal(fi["opcode"], e_d["opcode"]) and np.array_equal(fi["fin"][ok], e_d["fin"][ok])
    got = out.download()
    bad = np.nonzero(got != e_arena)[0]
    assert bad.size == 0, f"{bad.size} arena bytes differ, first at {bad[:8]} (cap {cap})"
    odd = ~ok | (e_d["header_size"].astype(np.uint64) + e_d["payload_size"] != np.uint64(stride))
    assert int(mm.item()) == int(odd.sum())
    return e_st, int(odd.sum())


@pytest.mark.parametrize("flush_end", [True, False], ids=["end", "start"])
@pytest.mark.parametrize("fs", [256, 1000, 4096])
def test_guard_uniform_receive(guards, fs, flush_end):
    """The wire of a uniform batch at its stride: window kernels with one,
    two and eight blocks per lane."""
    n = 700
    payload, keys, d = _frames(n, fs, 1, 1, 2, fs)
    wire, _ = O.serialize_batch(payload, d)
    slot = W.round16(fs)
    st, odd = _recv_guarded(guards, wire, len(wire), n, cfws.uniform_frame_bytes(fs, True), slot, n * slot, flush_end)
    assert (st == O.PARSE_COMPLETE).all() and odd == 0


@pytest.mark.parametrize("flush_end", [True, False], ids=["end", "start"])
def test_guard_uniform_receive_non_uniform_wire(guards, flush_end):
    """test_uniform_receive_non_uniform_wire at stride 262: starts anywhere in
    headers and payloads, the last ones past the wire's end."""
    payload, desc = _seed21_batch(27)
    wire, _ = O.serialize_batch(payload, desc.view(O.DESC_DTYPE))
    stride = 262
    n = min(len(desc), len(wire) // stride + 3)
    assert n * stride > len(wire)
    _, odd = _recv_guarded(guards, wire, len(wire), n, stride, 96, n * 96, flush_end)
    assert odd > 0


@pytest.mark.parametrize("flush_end", [True, False], ids=["end", "start"])
def test_guard_uniform_receive_truncated_and_cut(guards, flush_end):
    """test_uniform_receive_truncated_and_cut: the wire ends one byte into
    the tenth-last frame (the kernel's own starts of the last nine lie past
    wire_size) and the capacity ends five bytes into a slot."""
    n, fs = 3000, 256
    payload, keys, d = _frames(n, fs, 1, 1, 2, 9)
    wire, _ = O.serialize_batch(payload, d)
    stride = cfws.uniform_frame_bytes(fs, True)
    cut, cap = (n - 10) * stride + 1, n * 256 // 2 + 5
    assert n * stride > cut + 9 * stride and cap % 256
    st, odd = _recv_guarded(guards, wire, cut, n, stride, 256, cap, flush_end)
    assert st[-1] == O.PARSE_MORE_DATA and odd == n - cap // 256
