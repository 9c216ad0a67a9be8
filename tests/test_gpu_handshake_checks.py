"""cfws_ws_upgrade_keys_batch and cfws_ws_check_accept_batch: the server's
decision on each Sec-WebSocket-Key (co_http_request_validate_ws_upgrade,
co_ws_http_extension.c:156-170, over co_base64_decode's own rules) and the
client's strcmp of each answer (:247), against the reference's fixtures
(tests/golden/handshake_client_cases.json) and the Python restatement
(tests/handshake_util.py, pinned in tests/test_handshake_rules.py).

Why the guarded accesses stay inside (read from cfws_handshake.hip): thread
c < n reads key_off[c] and key_off[c + 1] (n + 1 offsets) and, with L their
difference, key bytes [0, L) only: a 24-byte key as three 8-byte loads when
its address is 8-byte aligned, byte loads otherwise, and any other length
through accept_msg_byte, which reads key[i] for i < L alone. It writes
valid[c], one byte, and its accept slot only where d_accept is given. The
class table is indexed by a byte (256 entries). Threads at or past n read and
write nothing; they only take part in the wave's count."""
import random

import numpy as np
import pytest

import handshake_util as HU
from conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from test_gpu_guard import GuardBuf, _glib  # noqa: E402

CASES = golden("handshake_client_cases.json")
SENT = 0xEE
RFC_KEY = b"dGhlIHNhbXBsZSBub25jZQ=="
RFC_ACCEPT = b"s3pPLMBiTxaQ9kYGzzhZRbK+xOo="


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def storm():
    """20,000 edited keys and 2,000 arbitrary byte strings, with the device's
    verdicts and accepts: computed once, shared."""
    rng = random.Random(0x57A9)
    keys = HU.edited_keys(rng, 20000) + [rng.randbytes(rng.randrange(0, 260)) for _ in range(2000)]
    valid, accepts, invalid = cfws.ws_upgrade_keys(keys)
    return keys, valid, accepts, invalid


def _raw_call(raw, off, n, valid_t, accept_t, count_t):
    rc = cfws.lib().cfws_ws_upgrade_keys_batch(cfws._p(raw), cfws._p(off), n, cfws._p(valid_t), cfws._p(accept_t),
                                               cfws._p(count_t), cfws._stream(None))
    torch.cuda.synchronize()
    return rc


def test_upgrade_reference_fixtures_one_batch():
    keys = [bytes.fromhex(h) for h, _, _ in CASES["decode"]]
    want = np.array([bool(ok) and length == 16 for _, ok, length in CASES["decode"]], np.uint8)
    valid, accepts, invalid = cfws.ws_upgrade_keys(keys)
    bad = np.nonzero(valid != want)[0]
    assert bad.size == 0, [keys[i] for i in bad[:5]]
    assert invalid == int((want == 0).sum())
    assert accepts == [HU.accept_of(k) for k in keys]


def test_upgrade_reference_fixtures_one_key_per_call():
    for h, ok, length in CASES["decode"]:
        key = bytes.fromhex(h)
        valid, accepts, invalid = cfws.ws_upgrade_keys([key])
        want = bool(ok) and length == 16
        assert (int(valid[0]), invalid) == (int(want), int(not want)), key
        assert accepts == [HU.accept_of(key)]


def test_upgrade_verdicts_storm(storm):
    keys, valid, _, invalid = storm
    want = np.array([HU.key_valid(k) for k in keys], np.uint8)
    bad = np.nonzero(valid != want)[0]
    assert bad.size == 0, [keys[i] for i in bad[:5]]
    assert invalid == int((want == 0).sum())
    assert 5000 <= int(want.sum()) <= 15000                               # both verdicts well covered


def test_upgrade_accepts_equal_the_accept_call(storm):
    keys, _, accepts, _ = storm
    assert accepts == cfws.ws_accept_keys(keys)


def test_upgrade_count_buffer_with_garbage_on_entry():
    keys = [RFC_KEY, b"A" * 23, RFC_KEY[:22], b" " + RFC_KEY, b""] * 130   # 650 keys: three workgroups
    raw, off = cfws._packed(keys, "cuda")
    valid = torch.full((len(keys),), SENT, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), 0x7badbeef, dtype=torch.int32, device="cuda")
    for _ in range(2):                                                    # and again, over its own result
        assert _raw_call(raw, off, len(keys), valid, None, count) == cfws.OK
        assert int(count.item()) == 3 * 130
    assert valid.cpu().numpy().tolist() == [1, 0, 1, 0, 0] * 130


def test_upgrade_without_accepts_and_empty_batch():
    keys = [RFC_KEY, b"x"]
    raw, off = cfws._packed(keys, "cuda")
    valid = torch.full((2 + 16,), SENT, dtype=torch.uint8, device="cuda")
    assert _raw_call(raw, off, 2, valid, None, None) == cfws.OK
    assert valid.cpu().numpy().tolist() == [1, 0] + [SENT] * 16
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    assert _raw_call(None, None, 0, None, None, count) == cfws.OK         # n == 0: the counter only
    assert int(count.item()) == 0
    assert _raw_call(None, off, 2, valid, None, None) == cfws.ERROR_INVALID_ARGUMENT
    assert _raw_call(raw, off, 2, None, None, None) == cfws.ERROR_INVALID_ARGUMENT


@pytest.mark.parametrize("base", [0, 8, 1, 3], ids=lambda b: f"base{b}")
def test_upgrade_keys_packed_24_apart(base):
    """Both load forms of a 24-byte key: 8-byte aligned (three 8-byte loads)
    and not (byte loads)."""
    rng = random.Random(base)
    keys = [k for k in HU.edited_keys(rng, 1500) if len(k) == 24][:300]
    assert len(keys) == 300 and 30 <= sum(map(HU.key_valid, keys)) <= 270  # both verdicts
    buf = torch.zeros(base + 24 * len(keys) + 64, dtype=torch.uint8, device="cuda")
    buf[base:base + 24 * len(keys)] = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    off = torch.arange(0, 24 * (len(keys) + 1), 24, dtype=torch.int64, device="cuda")
    valid = torch.zeros(len(keys), dtype=torch.uint8, device="cuda")
    out = torch.zeros(32 * len(keys), dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert _raw_call(buf[base:], off, len(keys), valid, out, count) == cfws.OK
    want = [int(HU.key_valid(k)) for k in keys]
    assert valid.cpu().numpy().tolist() == want and int(count.item()) == want.count(0)
    assert cfws._slot_strings(out, len(keys)) == [HU.accept_of(k) for k in keys]


@pytest.mark.parametrize("slot_shift", [0, 1])
def test_upgrade_decreasing_offsets(slot_shift):
    """A key whose end offset lies below its start gets valid 0 and an
    all-zero slot; its neighbours are computed as usual. slot_shift 1: the
    output is not 16-byte aligned (the byte-store form)."""
    keys = [RFC_KEY, b"x" * 24, b"abc"]
    raw = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    off = torch.tensor([0, 24, 10, 51], dtype=torch.int64, device="cuda")  # key 1: [24, 10)
    buf = torch.full((3 * 32 + 16,), SENT, dtype=torch.uint8, device="cuda")
    out = buf[slot_shift:]
    valid = torch.full((3,), SENT, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert _raw_call(raw, off, 3, valid, out, count) == cfws.OK
    h = out[:96].cpu().numpy().reshape(3, 32)
    last = b"".join(keys)[10:51]
    assert bytes(h[0, :29]) == RFC_ACCEPT + b"\0" and not h[1].any()
    assert bytes(h[2, :29]) == HU.accept_of(last).encode() + b"\0"
    assert valid.cpu().numpy().tolist() == [1, 0, int(HU.key_valid(last))] and int(count.item()) == 2
    if slot_shift:                                                        # the slot's last 3 bytes left alone
        assert (h[0, 29:] == SENT).all() and (h[2, 29:] == SENT).all()
    else:
        assert not h[0, 28:].any() and not h[2, 28:].any()


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


def test_upgrade_guarded(guards):
    """The keys exactly their bytes long and flush at the end (their total a
    multiple of 16, so the arena ends with the last key), d_valid exactly n
    bytes (n a multiple of 16 likewise)."""
    rng = random.Random(5)
    keys = HU.edited_keys(rng, 319) + [b"A" * 266 + b"=" * 734]           # n = 320: a multiple of 16
    pad = -sum(map(len, keys)) % 16
    keys[0] = b"=" * pad + keys[0]                                        # total: a multiple of 16
    n, total = len(keys), sum(map(len, keys))
    assert n % 16 == 0 and total % 16 == 0 and n > 256
    raw_np = np.frombuffer(b"".join(keys), np.uint8)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)).cuda()
    raw = guards(total).upload(raw_np)
    valid = guards(n)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert _raw_call(raw, off, n, valid, None, count) == cfws.OK
    want = [int(HU.key_valid(k)) for k in keys]
    assert valid.download()[:n].tolist() == want and int(count.item()) == want.count(0)


# ---- the client's check of the answers ----------------------------------------

def _check_call(expect, answers):
    expect_t = torch.from_numpy(HU.slots(expect)).cuda()
    ok, failed = cfws.ws_check_accept(expect_t, answers)
    want = [int(HU.check(e, a)) for e, a in zip(expect, answers)]
    assert ok.tolist() == want, [(e, a) for e, a, o, w in zip(expect, answers, ok, want) if o != w][:5]
    assert failed == want.count(0)
    return want


def test_check_accept_cases():
    a = RFC_ACCEPT
    answers = [a, a[:-1], a + b"=", b"", a[:10] + b"\0" + a[11:], a + b"\0", a + b"\0junk", a[:27] + b"\0"]
    answers += [a[:i] + bytes([a[i] ^ 1]) + a[i + 1:] for i in range(28)]  # one byte changed at each position
    want = _check_call([a] * len(answers), answers)
    assert want == [1, 0, 0, 0, 0, 1, 1, 0] + [0] * 28
    # an empty expectation: only an empty answer (or one starting with NUL) matches
    assert _check_call([b"", b"", b""], [b"", b"\0x", b"x"]) == [1, 1, 0]


def test_check_accept_many_and_counts():
    rng = random.Random(3)
    keys, accepts, _ = HU.client_keys(7, 11, 1000)
    expect = [x.encode() for x in accepts]
    answers = []
    for e in expect:
        how = rng.randrange(4)
        answers.append(e if how < 2 else e[:-1] if how == 2 else e[:5] + b"#" + e[6:])
    want = _check_call(expect, answers)
    assert 300 < sum(want) < 700


def test_check_accept_decreasing_offsets_and_empty_batch():
    a = RFC_ACCEPT
    expect_t = torch.from_numpy(HU.slots([a, a, a])).cuda()
    resp = torch.from_numpy(np.frombuffer(a + a + a, np.uint8).copy()).cuda()
    off = torch.tensor([0, 28, 20, 48], dtype=torch.int64, device="cuda")  # answer 1: [28, 20); answer 2: a[20:] + a[:20]
    ok = torch.full((3 + 16,), SENT, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    L = cfws.lib()
    assert L.cfws_ws_check_accept_batch(cfws._p(expect_t), cfws._p(resp), cfws._p(off), 3, cfws._p(ok),
                                        cfws._p(count), cfws._stream(None)) == cfws.OK
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == [1, 0, 0] + [SENT] * 16 and int(count.item()) == 2
    assert L.cfws_ws_check_accept_batch(None, None, None, 0, None, cfws._p(count), cfws._stream(None)) == cfws.OK
    torch.cuda.synchronize()
    assert int(count.item()) == 0
    assert L.cfws_ws_check_accept_batch(cfws._p(expect_t), None, cfws._p(off), 3, cfws._p(ok), None,
                                        cfws._stream(None)) == cfws.ERROR_INVALID_ARGUMENT


def test_round_trip_client_server_client():
    """The client's keys, the server's decision and answers, the client's check."""
    n = cfws.ws_client_keys_group_conns() + 77
    keys_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    expect_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    cfws.ws_client_keys_into(n, keys_t, expect_t, None, seed=99, first_draw=6)
    keys = [k.encode() for k in cfws._slot_strings(keys_t, n)]
    valid, answers, invalid = cfws.ws_upgrade_keys(keys)                  # the server's side
    assert valid.all() and invalid == 0
    ok, failed = cfws.ws_check_accept(expect_t, [a.encode() for a in answers])
    assert ok.all() and failed == 0
    answers[5] = answers[6]
    ok, failed = cfws.ws_check_accept(expect_t, [a.encode() for a in answers])
    assert failed == 1 and not ok[5] and ok.sum() == n - 1
