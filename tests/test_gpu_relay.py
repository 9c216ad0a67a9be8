"""cfws_relay_batch on the GPU (include/cfws.h), bit-exact
against tests/relay_util.expect_relay (the oracle's deserialize + serialize).
Every arena is exact and flush against an unmapped range (GuardBuf,
tests/test_gpu_guard.py), filled with 0xEE: the out wire must match below
min(total, capacity) and keep the sentinel from there to round16(capacity);
d_desc, d_status and *d_out_total must match too. The shapes are the smallest
at which each part can go wrong (header classes, source-against-destination
phases, region classes, frames that emit nothing, capacity cuts, index forms,
the plan above its self-scan)."""
import re

import numpy as np
import pytest

import oracle as O
import relay_util as RU

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from coldforce_amd import workloads as W  # noqa: E402
from test_gpu_guard import GuardBuf, _seed21_batch, device, guards  # noqa: E402,F401

DESC_FIELDS = ("payload_off", "wire_off", "payload_size", "mask_key", "fin", "opcode", "mask", "header_size")


def _keys(n, seed=7):
    return (O.splitmix_words(seed, 0, n) >> np.uint64(9)).astype(np.uint32)


def _keys_t(keys):
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int32).copy()).cuda()


def _relay(guards, wire, wire_size, starts, policy, out_mask, keys, cap=None, flush_end=True,
           max_payload=O.DEFAULT_MAX_PAYLOAD, expect=None):
    """One cfws.relay call over exact guarded arenas, checked against the
    expectation; returns the expectation (out wire, offsets, desc, status)."""
    exp = expect or RU.expect_relay(wire, wire_size, starts, policy, out_mask, keys, max_payload)
    e_out, _, e_desc, e_st = exp
    total = len(e_out)
    cap = total if cap is None else cap
    n = len(starts)
    w = guards(max(wire_size, 1), flush_end).upload(wire[:wire_size])
    out = guards(max(cap, 1), flush_end)
    idx = torch.from_numpy(np.asarray(starts, dtype=np.uint64).astype(np.int64)).cuda()
    d_t, st_t, tot = cfws.relay(w, wire_size, idx, out, policy, out_mask, _keys_t(keys[:n]) if out_mask else None,
                                max_payload=max_payload, out_capacity=cap)
    torch.cuda.synchronize()
    assert int(tot.item()) == total
    assert np.array_equal(st_t.cpu().numpy(), e_st)
    d = cfws.desc_from_device(d_t)
    for f in DESC_FIELDS:
        assert np.array_equal(d[f], e_desc[f]), f
    got = out.download()
    c = min(total, cap)
    bad = np.nonzero(got[:c] != e_out[:c])[0]
    assert bad.size == 0, f"{bad.size} of {c} out bytes differ, first at {bad[:8]}"
    assert (got[c:] == 0xEE).all(), "written at or past min(total, capacity)"
    return exp


def _uniform(n, size, in_mask, seed, opcode=2):
    return RU.frames_wire([size] * n, [in_mask] * n, [1] * n, [opcode] * n, seed)


# 1. header classes: h_in, h_out in {2, 4, 6, 8, 10, 14}
HEADER_SIZES = [0, 1, 15, 16, 17, 125, 126, 127, 65535, 65536]


@pytest.mark.parametrize("out_mask", [0, 1])
@pytest.mark.parametrize("in_mask", [0, 1])
def test_header_classes(guards, in_mask, out_mask):
    for k, size in enumerate(HEADER_SIZES):                    # each alone: the frame at offset 0
        wire, starts = _uniform(1, size, in_mask, 40 + k, opcode=1)
        _relay(guards, wire, len(wire), starts, RU.VERBATIM, out_mask, _keys(1, size))
    n = len(HEADER_SIZES)                                      # and back to back
    wire, starts = RU.frames_wire(HEADER_SIZES, [in_mask] * n, [k & 1 for k in range(n)], [2] * n, 50)
    _relay(guards, wire, len(wire), starts, RU.VERBATIM, out_mask, _keys(n))


# 2. phase drift: consecutive sizes walk the source through every phase
# against the 16-aligned output chunks
@pytest.mark.parametrize("masks", [(1, 0), (0, 1), (1, 1)], ids=["unmask", "mask", "remask"])
@pytest.mark.parametrize("base", [200, 5000])
def test_phase_drift(guards, base, masks):
    n = 64
    wire, starts = RU.frames_wire([base + j for j in range(n)], [masks[0]] * n, [1] * n, [2] * n, base)
    _relay(guards, wire, len(wire), starts, RU.VERBATIM, masks[1], _keys(n, base))


# 3. region classes
def _seed21_wire(seed=21):
    payload, desc = _seed21_batch(seed)
    wire, d = O.serialize_batch(payload, desc.view(O.DESC_DTYPE))
    return wire, d["wire_off"].astype(np.uint64)


@pytest.fixture(scope="module")
def mixed():
    return _seed21_wire()


@pytest.mark.parametrize("shape", ["3x64k", "40x12000", "300tiny"])
@pytest.mark.parametrize("masks", [(1, 0), (1, 1)], ids=["unmask", "remask"])
def test_region_classes(guards, shape, masks):
    if shape == "3x64k":            # fast and two-frame regions; in -> out drifts by 4 per frame
        wire, starts = _uniform(3, 65536, masks[0], 31)
    elif shape == "40x12000":
        wire, starts = _uniform(40, 12000, masks[0], 32)
    else:                           # more than 64 frames in a region: the per-chunk search
        n = 300
        wire, starts = RU.frames_wire([j % 41 for j in range(n)], [masks[0]] * n, [1] * n, [1] * n, 33)
    _relay(guards, wire, len(wire), starts, RU.VERBATIM, masks[1], _keys(len(starts), 3))


@pytest.mark.parametrize("policy", [RU.VERBATIM, RU.ECHO_SERVER], ids=["verbatim", "echo"])
@pytest.mark.parametrize("out_mask", [0, 1])
def test_region_classes_mixed_batch(guards, mixed, policy, out_mask):
    wire, starts = mixed
    _relay(guards, wire, len(wire), starts, policy, out_mask, _keys(len(starts), 4))


# 4. frames that emit nothing
@pytest.mark.parametrize("out_mask", [0, 1])
def test_non_complete_frames_change_no_outgoing_byte(guards, out_mask):
    """Invalid byte 0 (-7001), over max_payload (-7005) and a truncated last
    frame (MORE_DATA) between COMPLETE ones: the out wire is that of the
    COMPLETE frames alone."""
    sizes = [300, 20, 5000, 100, 0, 700, 64, 4096, 9, 130, 2000, 50]
    n = len(sizes)
    wire, starts = RU.frames_wire(sizes, [j % 3 != 0 for j in range(n)], [1] * n, [2] * n, 61, bad_b0=(1, 6, 7))
    wire_size = len(wire) - 5                                  # the last frame loses 5 bytes
    keys = _keys(n, 61)
    _, _, _, st = _relay(guards, wire, wire_size, starts, RU.VERBATIM, out_mask, keys, max_payload=4500)
    assert list(st) == [0, -7001, -7005, 0, 0, 0, -7001, -7001, 0, 0, 0, 1]
    ok = st == 0
    out_all = RU.expect_relay(wire, wire_size, starts, RU.VERBATIM, out_mask, keys, 4500)[0]
    out_ok = RU.expect_relay(wire, wire_size, starts[ok], RU.VERBATIM, out_mask, keys[ok], 4500)[0]
    assert np.array_equal(out_all, out_ok)


@pytest.mark.parametrize("out_mask", [0, 1])
def test_echo_server_policy(guards, out_mask):
    """200 PONG / CLOSE frames between two data frames emit nothing; a PING
    (fin = 0, empty, 125 bytes) comes back as a final PONG."""
    sizes = [1000] + [(7 * j) % 126 for j in range(200)] + [3000, 33, 0, 125, 10]
    ops = [1] + [10 if j % 2 else 8 for j in range(200)] + [2, 9, 9, 9, 0]
    fins = [1] * 201 + [0, 0, 1, 1, 1]
    n = len(sizes)
    wire, starts = RU.frames_wire(sizes, [1] * n, fins, ops, 62)
    e_out, offs, _, _ = _relay(guards, wire, len(wire), starts, RU.ECHO_SERVER, out_mask, _keys(n, 62))
    assert (offs[1:202] == offs[1]).all() and offs[1] == 1000 + (8 if out_mask else 4)
    for i, size in ((202, 33), (203, 0), (204, 125)):          # the PONGs: fin = 1, opcode 0xA
        assert e_out[int(offs[i])] == 0x8A and e_out[int(offs[i]) + 1] & 0x7f == size
    _relay(guards, wire, len(wire), starts, RU.VERBATIM, out_mask, _keys(n, 62))   # PINGs as they came


# 5. capacity
@pytest.mark.parametrize("flush_end", [True, False], ids=["end", "start"])
def test_capacity_cuts(guards, flush_end):
    sizes = [5000, 70, 9000, 300]
    wire, starts = RU.frames_wire(sizes, [1] * 4, [1] * 4, [2] * 4, 63)
    keys = _keys(4, 63)
    exp = RU.expect_relay(wire, len(wire), starts, RU.VERBATIM, 1, keys)
    total = len(exp[0])
    off2 = int(exp[1][2])                                      # frame 2: 8-byte header, 9,000-byte body
    for cap in (0, off2 + 3, off2 + 8, off2 + 8 + 4097, total - 1, total, total + 16):
        _relay(guards, wire, len(wire), starts, RU.VERBATIM, 1, keys, cap=cap, flush_end=flush_end, expect=exp)


# 6. index forms
def test_reversed_index(guards, mixed):
    wire, starts = mixed
    rev = starts[::-1][:1500].copy()
    _relay(guards, wire, len(wire), rev, RU.ECHO_SERVER, 1, _keys(len(rev), 5))


def test_fan_out(guards):
    wire, starts = RU.frames_wire([10, 777, 10], [1, 1, 0], [1] * 3, [1] * 3, 64)
    _relay(guards, wire, len(wire), np.repeat(starts[1:2], 64), RU.VERBATIM, 1, _keys(64, 6))


@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single(guards, n):
    wire, starts = RU.frames_wire([100, 200], [1, 0], [1, 1], [2, 2], 65)
    _relay(guards, wire, len(wire), starts[:n], RU.VERBATIM, 1, _keys(2), cap=256 if n == 0 else None)


# 7. more plan blocks than the apply kernel sums itself: the scan launch
def test_plan_above_self_scan(guards):
    n = 524289 + 7
    sizes = (np.arange(n, dtype=np.uint64) * 7 // 3) % 4
    ops = np.where(np.arange(n) % 5 == 3, 9, 2)
    wire, starts = RU.frames_wire(sizes, np.arange(n) % 3 != 1, np.ones(n), ops, 66)
    _relay(guards, wire, len(wire), starts, RU.ECHO_SERVER, 1, _keys(n, 66))


# 8. the two-call path
def test_agrees_with_deserialize_then_serialize(guards, mixed):
    wire, starts = mixed
    n = len(starts)
    keys = _keys(n, 8)
    e_out = _relay(guards, wire, len(wire), starts, RU.VERBATIM, 1, keys)[0]
    w = guards(len(wire)).upload(wire)
    idx = torch.from_numpy(starts.astype(np.int64)).cuda()
    cap = int(O.deserialize_batch(wire, starts, align=16)[3])
    arena = guards(cap)
    d_t, st_t, _ = cfws.deserialize(w, len(wire), idx, arena, align=16)
    torch.cuda.synchronize()
    assert bool((st_t == 0).all())
    d = cfws.desc_from_device(d_t)
    d["mask"] = 1
    d["mask_key"] = keys
    out = guards(len(e_out))
    tot = cfws.serialize(arena, cfws.desc_to_device(d), out)
    torch.cuda.synchronize()
    assert int(tot.item()) == len(e_out)
    assert np.array_equal(out.download(len(e_out)), e_out)


# 9. arguments
class _View:
    """Bytes [off, off + n) of a GuardBuf, as the tensors cfws.py takes."""

    def __init__(self, buf, off, n):
        self.buf, self.off, self.n, self.device = buf, off, n, buf.device

    def data_ptr(self):
        return self.buf.data_ptr() + self.off

    def numel(self):
        return self.n


@pytest.mark.parametrize("what", ["overlap", "misaligned_out", "misaligned_in", "policy", "workspace", "no_keys"])
def test_argument_errors_write_nothing(guards, what):
    wire, starts = _uniform(8, 500, 1, 67)
    n, size = len(starts), len(wire)
    cap = size
    both = guards(W.round16(size) + cap + 32).upload(wire)
    w, out = _View(both, 0, size), _View(both, W.round16(size), cap)
    policy, keys = RU.VERBATIM, _keys_t(_keys(n))
    ws = cfws.relay_workspace(n, cap)
    rc = -1                                                    # CFWS_ERROR_INVALID_ARGUMENT
    if what == "overlap":
        out = _View(both, W.round16(size) - 16, cap)           # the input's last readable block
    elif what == "misaligned_out":
        out = _View(both, W.round16(size) + 8, cap)
    elif what == "misaligned_in":
        w = _View(both, 8, size - 8)
    elif what == "policy":
        policy = 2
    elif what == "workspace":
        ws, rc = ws[:cfws.lib().cfws_relay_workspace_size(n, cap) - 1], -2      # CFWS_ERROR_WORKSPACE
    else:
        keys = None
    before = both.download()
    d_t = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
    st_t = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tot = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    idx = torch.from_numpy(starts.astype(np.int64)).cuda()
    with pytest.raises(cfws.CodecError, match=re.escape(f"rc={rc}:")):
        cfws.relay(w, w.numel(), idx, out, policy, True, keys, desc_t=d_t, status_t=st_t, ws_t=ws, total_t=tot)
    torch.cuda.synchronize()
    assert np.array_equal(both.download(), before)
    assert bool((d_t == 0x5A).all()) and bool((st_t == 0x5A5A5A5A).all()) and int(tot.item()) == 77


# 10. the timing hook
def test_timing_pair_recorded_and_consumed(guards):
    wire, starts = _uniform(64, 4096, 1, 68)
    w = guards(len(wire)).upload(wire)
    out = guards(len(wire))
    idx = torch.from_numpy(starts.astype(np.int64)).cuda()
    a, b = cfws.TimingEvent(), cfws.TimingEvent()
    cfws.time_next_pass(a, b)
    cfws.relay(w, len(wire), idx, out)
    torch.cuda.synchronize()
    t1 = a.elapsed_time(b)
    assert t1 >= 0.0
    for _ in range(3):                                         # later calls leave the pair alone
        cfws.relay(w, len(wire), idx, out)
    torch.cuda.synchronize()
    assert a.elapsed_time(b) == t1
