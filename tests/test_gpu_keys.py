"""cfws_draw_mask_keys_device against the host form
(cfws_draw_mask_keys_seeded_at, itself pinned in tests/test_keys_host.py),
bit for bit: sizes round every run boundary of the kernel, unaligned and far
positions, seeds, mask flags, continuation, guarded arenas, the send it
feeds, and the call path.

The kernel's runs, in frames (cfws_keys.hip): a lane draws r = 32 (one
128-byte line of keys), a wave w = 64 r = 2,048, a workgroup G = 4 w = 8,192
(cfws_draw_keys_group_frames). With flags a thread ranks 16 frames, a block
4,096, and above 2,048 such blocks the block sums are scanned by a launch of
their own instead of by every block.

Why every access stays inside its arena (read from cfws_keys.hip before the
guarded cases ran; the contract is d_keys = 4 n bytes, flags readable to
round16(n), the workspace cfws_draw_keys_workspace_size(n)):
  * draw_keys_kernel loads only its two compile-time tables: kLanePow at
    lane < 64 (64 entries), kWavePow at bit j of the wave index g, and
    g < 2^21 = the table's 21 entries because n < 2^32 is checked on the
    host. A wave whose first frame is at or past n returns before anything;
    a lane whose first frame k0 is at or past n returns before its stores.
    Chunk c of a lane covers keys [kf, kf + 4), kf = k0 + 4 c, a multiple of
    4: it is stored whole only when kf + 4 <= n, key by key below n
    otherwise, and not at all when kf >= n. The base pointer is 16-byte
    aligned (checked), so a whole chunk is one aligned 16-byte store.
    *next_draw is written by thread 0 of block 0 only when non-NULL.
  * With flags the same kernel writes the workspace's first 4 n bytes (its
    "keys", n the same) and the layout puts the total's slot at
    round16(4 n) and the block sums after it: nb = ceil(n / 4096) words, the
    grid of both flag kernels, each block writing or reading partials[its
    own index] (and all nb of them in the self-scan).
  * flag_bits loads 16 bytes at i0 = 16 t only when i0 < n, so the load ends
    at or before round16(n); bits of frames at or past n are cleared.
  * keys_select_kernel reads packed[rank] only for a set flag of a frame
    below n: rank < masked frames <= n. It stores 16 keys as four aligned
    chunks when i0 + 16 <= n, key by key below n otherwise."""
import numpy as np
import pytest

import keys_util as KU
import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from coldforce_amd import workloads as W  # noqa: E402
from test_gpu_guard import GuardBuf, _glib  # noqa: E402
from test_gpu_timing import _batch, _recorded  # noqa: E402

R_LANE, R_WAVE = 32, 2048
FLAG_BLOCK, SELF_SCAN_BLOCKS = 4096, 2048
SEED = 1234
SENT = -286331154                      # 0xEEEEEEEE as int32
FIRST = (0, 1, 2, 3, 1000003)
FAR = (2**32 + 1, 2**40 + 3, 2**62)


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()
    torch.cuda.synchronize()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def G():
    g = cfws.draw_keys_group_frames()
    assert g % R_WAVE == 0 and R_WAVE % R_LANE == 0 and g > R_WAVE
    return g


def _dirty_ws(n):
    return torch.randint(0, 256, (cfws.draw_keys_workspace_size(n),), dtype=torch.uint8, device="cuda")


def _flags_t(flags):
    """The flags in round16(n) readable bytes, the padding non-zero."""
    if flags is None:
        return None
    f = np.full(max(W.round16(len(flags)), 16), 0xEE, np.uint8)
    f[:len(flags)] = flags
    return torch.from_numpy(f).cuda()


def _draw(n, first, seed=SEED, flags=None, stream=None):
    """One device call into n + 64 words of sentinel; returns (buffer, next)."""
    buf = torch.full((n + 64,), SENT, dtype=torch.int32, device="cuda")
    nxt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    cfws.draw_mask_keys_device(n, _flags_t(flags), seed, first, buf, nxt,
                               None if flags is None else _dirty_ws(n), stream=stream)
    return buf, nxt


def _check(n, first, seed=SEED, flags=None, want=None, stream=None):
    buf, nxt = _draw(n, first, seed, flags, stream)
    if want is None:
        want, want_next = cfws.draw_mask_keys_at(n, flags, seed, first)
    else:
        want, want_next = want
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    bad = np.nonzero(got[:n].view(np.uint32) != want[:n])[0]
    assert bad.size == 0, f"n {n} first_draw {first} seed {seed}: {bad.size} keys differ, first at {bad[:6]}"
    assert (got[n:] == SENT).all(), f"n {n}: written past 4 n bytes"
    assert int(nxt.item()) == want_next, (n, first, int(nxt.item()), want_next)


def _sizes(G):
    edge = {k * s + d for s in (R_LANE, R_WAVE, G) for k in (1, 2, 3) for d in (-1, 0, 1)}
    return sorted(set(range(1, 68)) | edge | {3 * G + 5, 2**20 + 7})


@pytest.mark.parametrize("first", FIRST)
def test_sizes(G, first):
    sizes = _sizes(G)
    ref, _ = cfws.draw_mask_keys_at(sizes[-1], None, SEED, first)         # every n: a prefix
    for n in sizes:
        _check(n, first, want=(ref, first + 4 * n))


@pytest.mark.parametrize("first", FAR)
def test_far_positions(G, first):
    n = 2 * G + 5
    _check(n, first)
    buf, _ = _draw(64, first)                                             # and against the Python oracle
    want, _ = KU.keys_at(SEED, first, 64)
    assert np.array_equal(buf[:64].cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF])
def test_seeds(G, seed):
    for first in (0, 1000003):
        _check(2 * G + 5, first, seed=seed)
    if seed == 0:                                                         # glibc seeds 0 as 1
        assert torch.equal(_draw(100, 0, seed=0)[0], _draw(100, 0, seed=1)[0])


def _pattern(name, n, G):
    if name == "flip":                                                    # flips exactly at G - 1, G, G + 1
        f = np.ones(n, np.uint8)
        f[G - 1:G] = 0
        f[G + 1:G + 2] = 0
        return f
    if name == "random":
        return (np.random.default_rng(n).random(n) < .6).astype(np.uint8) * 7       # any non-zero byte is set
    return np.full(n, 1 if name == "ones" else 0, np.uint8)


@pytest.mark.parametrize("pattern", ["zeros", "random", "ones", "flip"])
def test_flags(G, pattern):
    for n in (1, 17, G + 1, 3 * G + 5):
        flags = _pattern(pattern, n, G)
        for first in (0, 3):
            _check(n, first, flags=flags)
        if pattern == "zeros":
            _, nxt = _draw(n, 77, flags=flags)
            assert int(nxt.item()) == 77


def test_flags_past_the_self_scan_limit():
    """More than 2,048 blocks of flags: the block sums take the scan launch."""
    n = SELF_SCAN_BLOCKS * FLAG_BLOCK + FLAG_BLOCK + 1
    flags = (np.random.default_rng(8).random(n) < .6).astype(np.uint8)
    _check(n, 5, flags=flags)


@pytest.mark.parametrize("with_flags", [False, True])
def test_continuation(G, with_flags):
    n1, n2 = G + 3, 2 * G - 1
    flags = _pattern("random", n1 + n2, G) if with_flags else None
    first = 2**40 + 3
    a, mid = _draw(n1, first, flags=None if flags is None else flags[:n1])
    b, end = _draw(n2, int(mid.item()), flags=None if flags is None else flags[n1:])
    whole, end1 = _draw(n1 + n2, first, flags=flags)
    assert torch.equal(torch.cat([a[:n1], b[:n2]]), whole[:n1 + n2])
    assert int(end.item()) == int(end1.item())
    want, want_next = cfws.draw_mask_keys_at(n1 + n2, flags, SEED, first)
    assert np.array_equal(whole[:n1 + n2].cpu().numpy().view(np.uint32), want) and int(end1.item()) == want_next


@pytest.fixture
def guards():
    if not _glib().guard_supported():
        pytest.skip("no HIP virtual memory management on this device")
    bufs = []

    def make(n, flush_end=True):
        b = GuardBuf(n, flush_end, 0xEE)
        bufs.append(b)
        return b
    yield make
    torch.cuda.synchronize()
    for b in bufs:
        b.free()


@pytest.mark.parametrize("flush_end", [True, False], ids=["end", "start"])
@pytest.mark.parametrize("with_flags", [False, True], ids=["all", "flags"])
def test_guarded_arenas(G, guards, with_flags, flush_end):
    """d_keys in exactly 4 n bytes, the flags in round16(n), the workspace in
    exactly its size, each flush against an unmapped range."""
    for n in (1, 5, G - 1, G + 1, 3 * G + 5):
        flags = _pattern("random", n, G) if with_flags else None
        keys = guards(4 * n, flush_end)
        nxt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        f_b = ws = None
        if with_flags:
            f_b = guards(W.round16(n), flush_end).upload(_flags_t(flags).cpu().numpy())
            ws = guards(cfws.draw_keys_workspace_size(n), flush_end)
        cfws.draw_mask_keys_device(n, f_b, SEED, 3, keys, nxt, ws)
        torch.cuda.synchronize()
        want, want_next = cfws.draw_mask_keys_at(n, flags, SEED, 3)
        got = keys.download()
        assert np.array_equal(got[:4 * n].view(np.uint32), want), n
        assert (got[4 * n:] == 0xEE).all(), n
        assert int(nxt.item()) == want_next


def test_end_to_end_uniform_send():
    """Keys drawn on the device feed cfws_serialize_uniform: the wire of the
    reference's serialize with the host's keys."""
    n, fs = 1000, 256
    keys_t, _ = cfws.draw_mask_keys_device(n, None, SEED, 0)
    payload = O.fill_splitmix(n * fs + 16, 0x5EED0077, 0)
    pay_t = torch.from_numpy(payload).cuda()
    Wf = cfws.uniform_frame_bytes(fs, True)
    wire = torch.zeros(n * Wf + 16, dtype=torch.uint8, device="cuda")
    cfws.serialize_uniform(pay_t, keys_t, n, fs, wire, opcode=cfws.OPCODE_BINARY, mask=True)
    torch.cuda.synchronize()
    host = cfws.draw_mask_keys(n, seed=SEED)
    want = b"".join(O.serialize_keyed(True, cfws.OPCODE_BINARY, True, int(host[i]),
                                      payload[i * fs:(i + 1) * fs].tobytes()) for i in range(n))
    assert wire[:n * Wf].cpu().numpy().tobytes() == want


def test_non_default_stream(G):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _check(G + 7, 2, stream=s)
        _check(G + 7, 2, flags=_pattern("random", G + 7, G), stream=s)


def test_empty_batch():
    for flags in (None, np.zeros(0, np.uint8)):
        buf, nxt = _draw(0, 12345, flags=flags)
        torch.cuda.synchronize()
        assert (buf == SENT).all() and int(nxt.item()) == 12345
    # no keys and no next position: nothing to do
    cfws.draw_mask_keys_device(0, None, SEED, 9, keys_t=torch.empty(0, dtype=torch.int32, device="cuda"))
    assert cfws.lib().cfws_draw_mask_keys_device(SEED, 9, 0, None, None, None, None, 0, None) == cfws.OK


def _rc(n, flags_t, keys_t, ws_t, first=0):
    return cfws.lib().cfws_draw_mask_keys_device(SEED, first, n, cfws._p(flags_t), cfws._p(keys_t), None,
                                                 cfws._p(ws_t), 0 if ws_t is None else ws_t.numel(),
                                                 cfws._stream(None))


def test_argument_errors():
    n = 100
    keys = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
    flags_t = _flags_t(np.ones(n, np.uint8))
    ws = _dirty_ws(n)
    assert _rc(n, flags_t, keys, ws[:ws.numel() - 1]) == cfws.ERROR_WORKSPACE
    assert _rc(n, flags_t, keys, None) == cfws.ERROR_WORKSPACE
    assert _rc(n, None, keys[1:], None) == cfws.ERROR_INVALID_ARGUMENT      # 4 bytes off a 16-byte boundary
    assert _rc(n, None, None, None) == cfws.ERROR_INVALID_ARGUMENT
    assert _rc(n, None, keys, None, first=2**62 + 1) == cfws.ERROR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (keys == SENT).all()                                             # a refused call writes nothing
    assert _rc(n, flags_t, keys, ws) == cfws.OK
    torch.cuda.synchronize()


def test_pending_timing_pair_is_dropped():
    payload, d, wire = _batch(4096, 4096)
    a, b = cfws.TimingEvent(), cfws.TimingEvent()
    cfws.time_next_pass(a, b)
    cfws.draw_mask_keys_device(5000, None, SEED, 0)
    cfws.serialize(payload, d, wire)                   # would record a carried-over pair
    torch.cuda.synchronize()
    assert not _recorded(a, b)
