"""cfws_ws_client_keys_batch against the reference's fixtures
(tests/golden/handshake_client_cases.json) and the Python restatement
(tests/handshake_util.py, itself pinned in tests/test_handshake_rules.py),
byte for byte: sizes round every run boundary of the kernel, unaligned and far
positions, continuation, the mask-key draw that follows, guarded arenas and
the call path.

The kernel's runs, in connections (cfws_handshake.hip, client_keys_kernel): a
lane produces r = 8 (its 128 draws: the run of the mask-key kernel, so both
use the same jump tables), a wave w = 64 r = 512, a workgroup G = 4 w = 2,048
(cfws_ws_client_keys_group_conns).

Why every access stays inside its arena (read from cfws_handshake.hip and
cfws_keydev.h before the guarded cases ran; the contract is 32 n bytes for
each output, 16-byte aligned):
  * The kernel loads only compile-time tables: kLanePow at lane < 64 (64
    entries), kWavePow at bit j of the wave index g, and g < 2^21 = the
    table's 21 entries because n < 2^30 connections (2^21 waves of 512) is
    checked on the host; kB64 at a 6-bit index (65 bytes). The nonce, the key
    and the hash live in registers.
  * A wave whose first connection is at or past n returns before anything; a
    lane whose first connection c0 is at or past n returns after the wave's
    shuffles and before its stores; inside a lane's run the loop returns at
    the first c >= n. So stores happen only for c < n.
  * Connection c stores its key slot at ws_keys + 32 c and, only when the
    pointer is non-NULL, its accept slot at expect + 32 c: each exactly two
    16-byte stores, [32 c, 32 c + 32), which lies inside [0, 32 n). The base
    pointers are 16-byte aligned (checked on the host), so store_slot takes
    its aligned form and both stores are aligned.
  * *next_draw is written by thread 0 of block 0 only when non-NULL."""
import numpy as np
import pytest

import handshake_util as HU
from conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from test_gpu_guard import GuardBuf, _glib  # noqa: E402
from test_gpu_timing import _batch, _recorded  # noqa: E402

R_LANE, R_WAVE = 8, 512
SEED = 1234
SENT = 0xEE
FIRST = (0, 1, 2, 3, 1000003)
FAR = (2**32 + 1, 2**40 + 3, 2**62)
CASES = golden("handshake_client_cases.json")


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()
    torch.cuda.synchronize()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def G():
    g = cfws.ws_client_keys_group_conns()
    assert g % R_WAVE == 0 and g > R_WAVE
    return g


def _want(seed, first, n):
    """(key slots, accept slots) of n connections as the call writes them."""
    keys, accepts, _ = HU.client_keys(seed, first, n)
    return HU.slots(keys), HU.slots(accepts)


def _call(n, first, seed=SEED, with_accepts=True, stream=None):
    """One call into 32 n + 64 bytes of sentinel each; returns (keys, accepts, next)."""
    kb = torch.full((32 * n + 64,), SENT, dtype=torch.uint8, device="cuda")
    ab = torch.full((32 * n + 64,), SENT, dtype=torch.uint8, device="cuda")
    nxt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    cfws.ws_client_keys_into(n, kb, ab if with_accepts else None, nxt, seed, first, stream=stream)
    return kb, ab, nxt


def _check(n, first, seed=SEED, want=None, with_accepts=True, stream=None):
    kb, ab, nxt = _call(n, first, seed, with_accepts, stream)
    wk, wa = _want(seed, first, n) if want is None else want
    torch.cuda.synchronize()
    gk, ga = kb.cpu().numpy(), ab.cpu().numpy()
    bad = np.nonzero((gk[:32 * n] != wk[:32 * n]).reshape(n, 32).any(axis=1))[0]
    assert bad.size == 0, f"n {n} first_draw {first} seed {seed}: {bad.size} keys differ, first at {bad[:6]}"
    assert (gk[32 * n:] == SENT).all(), f"n {n}: keys written past 32 n bytes"
    if with_accepts:
        bad = np.nonzero((ga[:32 * n] != wa[:32 * n]).reshape(n, 32).any(axis=1))[0]
        assert bad.size == 0, f"n {n} first_draw {first}: {bad.size} accepts differ, first at {bad[:6]}"
        assert (ga[32 * n:] == SENT).all(), f"n {n}: accepts written past 32 n bytes"
    else:
        assert (ga == SENT).all(), f"n {n}: the accepts' buffer was not passed, yet written"
    assert int(nxt.item()) == first + 16 * n, (n, first, int(nxt.item()))


def test_reference_fixtures():
    for c in CASES["client"]:
        n = len(c["keys"])
        keys, accepts, nxt = cfws.ws_client_keys(n, c["seed"], c["first_draw"])
        assert keys == c["keys"], (c["seed"], c["first_draw"])
        assert accepts[:len(c["accepts"])] == c["accepts"]
        assert nxt == c["first_draw"] + 16 * n


def test_reference_then_frames():
    """The upgrade keys, then the mask keys of the frames those connections
    send: *d_next_draw is the first_draw of cfws_draw_mask_keys_device."""
    t = CASES["then_frames"]
    keys, _, nxt = cfws.ws_client_keys(len(t["keys"]), t["seed"], 0)
    assert keys == t["keys"]
    mk, end = cfws.draw_mask_keys_device(len(t["mask_keys"]), None, t["seed"], nxt)
    torch.cuda.synchronize()
    assert ["%08x" % k for k in mk.cpu().numpy().view(np.uint32)] == t["mask_keys"]
    assert int(end.item()) == nxt + 4 * len(t["mask_keys"])


def _sizes(G):
    edge = {k * s + d for s in (R_LANE, R_WAVE, G) for k in (1, 2, 3) for d in (-1, 0, 1)}
    return sorted(set(range(1, 68)) | edge | {3 * G + 5})


@pytest.mark.parametrize("first", FIRST)
def test_sizes(G, first):
    sizes = _sizes(G)
    ref = _want(SEED, first, sizes[-1])                                   # every n: a prefix
    for n in sizes:
        _check(n, first, want=ref)


@pytest.mark.parametrize("first", FAR)
def test_far_positions(G, first):
    _check(2 * G + 5, first)


def test_without_expected_accepts(G):
    for n in (1, R_LANE + 1, G + 3):
        _check(n, 3, with_accepts=False)


def test_continuation(G):
    n1, n2 = G + 3, 2 * G - 1
    first = 2**40 + 3
    ka, aa, mid = _call(n1, first)
    kb, ab, end = _call(n2, int(mid.item()))
    kw, aw, end1 = _call(n1 + n2, first)
    assert torch.equal(torch.cat([ka[:32 * n1], kb[:32 * n2]]), kw[:32 * (n1 + n2)])
    assert torch.equal(torch.cat([aa[:32 * n1], ab[:32 * n2]]), aw[:32 * (n1 + n2)])
    assert int(end.item()) == int(end1.item()) == first + 16 * (n1 + n2)
    wk, wa = _want(SEED, first, n1 + n2)
    assert np.array_equal(kw[:32 * (n1 + n2)].cpu().numpy(), wk)
    assert np.array_equal(aw[:32 * (n1 + n2)].cpu().numpy(), wa)


def test_accepts_equal_the_accept_call(G):
    keys, accepts, _ = cfws.ws_client_keys(G + 9, SEED, 5)
    assert cfws.ws_accept_keys([k.encode() for k in keys]) == accepts


@pytest.fixture
def guards():
    if not _glib().guard_supported():
        pytest.skip("no HIP virtual memory management on this device")
    bufs = []

    def make(n, flush_end=True):
        b = GuardBuf(n, flush_end, SENT)
        bufs.append(b)
        return b
    yield make
    torch.cuda.synchronize()
    for b in bufs:
        b.free()


@pytest.mark.parametrize("flush_end", [True, False], ids=["end", "start"])
def test_guarded_arenas(G, guards, flush_end):
    """Both outputs in exactly 32 n bytes, each flush against an unmapped range."""
    for n in (1, 5, G - 1, G + 1, 3 * G + 5):
        kb, ab = guards(32 * n, flush_end), guards(32 * n, flush_end)
        nxt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        cfws.ws_client_keys_into(n, kb, ab, nxt, SEED, 3)
        torch.cuda.synchronize()
        wk, wa = _want(SEED, 3, n)
        assert np.array_equal(kb.download()[:32 * n], wk), n
        assert np.array_equal(ab.download()[:32 * n], wa), n
        assert int(nxt.item()) == 3 + 16 * n


def test_non_default_stream(G):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _check(G + 7, 2, stream=s)


def test_empty_batch():
    kb, ab, nxt = _call(0, 12345)
    torch.cuda.synchronize()
    assert (kb == SENT).all() and (ab == SENT).all() and int(nxt.item()) == 12345
    assert cfws.ws_client_keys(0, SEED, 9) == ([], [], 9)
    # no connections and no next position: nothing to do
    assert cfws.lib().cfws_ws_client_keys_batch(SEED, 9, 0, None, None, None, None) == cfws.OK


def _rc(n, keys_t, acc_t, first=0, nxt_t=None):
    return cfws.lib().cfws_ws_client_keys_batch(SEED, first, n, cfws._p(keys_t), cfws._p(acc_t), cfws._p(nxt_t),
                                                cfws._stream(None))


def test_argument_errors():
    n = 100
    kb = torch.full((32 * n + 64,), SENT, dtype=torch.uint8, device="cuda")
    ab = torch.full((32 * n + 64,), SENT, dtype=torch.uint8, device="cuda")
    nxt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    bad = cfws.ERROR_INVALID_ARGUMENT
    assert _rc(n, kb[4:], ab, nxt_t=nxt) == bad                             # off a 16-byte boundary
    assert _rc(n, kb, ab[8:], nxt_t=nxt) == bad
    assert _rc(n, None, ab, nxt_t=nxt) == bad
    assert _rc(n, kb, ab, first=2**62 + 1, nxt_t=nxt) == bad
    assert _rc(2**30, kb, ab, nxt_t=nxt) == bad
    torch.cuda.synchronize()
    assert (kb == SENT).all() and (ab == SENT).all() and int(nxt.item()) == -1   # a refused call writes nothing
    assert _rc(n, kb, ab, first=2**62, nxt_t=nxt) == cfws.OK
    torch.cuda.synchronize()
    assert int(nxt.item()) == 2**62 + 16 * n


def test_pending_timing_pair_is_dropped():
    payload, d, wire = _batch(4096, 4096)
    a, b = cfws.TimingEvent(), cfws.TimingEvent()
    cfws.time_next_pass(a, b)
    cfws.ws_client_keys(500, SEED, 0)
    cfws.serialize(payload, d, wire)                   # would record a carried-over pair
    torch.cuda.synchronize()
    assert not _recorded(a, b)
