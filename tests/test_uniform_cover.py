"""The shapes of the uniform-send GPU tests, and the check that they reach
every case of the kernels (cfws_uniform.hip). Host arithmetic only: no
library, no GPU.

The wire of a uniform batch is n frames of W = hs + fs bytes back to back,
written in aligned 16-byte chunks; each wave owns `span` bytes of it (4 KiB
in the small kernel for payloads under 1,024 bytes, 2 KiB from there and in
the general kernel). Chunk k is at D = 16 k, its frame is f = D // W and
off = D % W. A chunk is

  body  off >= hs and off + 16 <= W: payload bytes only;
  tail  off >= hs, off + 16 > W: the end of f's payload, then frame f + 1's
        header at chunk byte t = W - off (position t, 1..15);
  own   off < hs: the chunk starts `off` bytes into f's header (position
        -off).

A tail or own chunk also carries the head of the header's frame's payload
when the header ends before chunk byte 16, and it may be the last chunk of
its wave's span: there the head is a load of the lane's own, not the next
lane's block. What a kernel does with a chunk depends on (kind, position,
last-of-span with a head) alone, and that triple is periodic in D with
period lcm(W, span). So a batch of

  n = lcm(W, span) / W + 2

frames reaches every class any longer batch reaches; the test below
asserts it against a batch of twice that, class by class, for every case
the GPU tests import from here (tests/test_gpu_uniform.py,
tests/test_gpu_uniform_guard.py, tests/knob_parity.py). The frame that
ends the batch has no successor; its chunk is left out of the comparison
(the count tests cover it)."""
import math

import numpy as np
import pytest

SPAN_SMALL, SPAN_2K = 4096, 2048

# payload sizes of the small kernel's sweep (test_uniform_small_kernel_period),
# each masked and not: 7-bit lengths (hs 2 / 6) up to 112, 16-bit from 128
SMALL_PAYLOADS = (32, 48, 64, 80, 96, 112, 128, 240, 1008, 1024, 2000, 4096, 65520)
# general-kernel frames of 32..66 wire bytes (test_uniform_general_short_frames)
GENERAL_SHORT = [(fs, 1) for fs in (26, 27, 31, 33, 47, 57, 58, 59, 60)] + \
                [(fs, 0) for fs in (30, 31, 33, 61, 62, 63, 65)]
# the largest frames the bytes kernel takes (W = 31), next to the boundary
BYTES_NEIGHBOURS = [(25, 1), (29, 0)]
# the knob sweep (knob_parity.py uniform) on the small kernel, at either span
KNOB_PAYLOADS = (32, 112, 256, 1008, 1024, 4096, 65520)
# ... and on the general kernel, whose span no knob selects: one period of
# 100,000-byte frames is 1,026 of them (102 MB), and CFWS_UNIFORM_LDS changes
# how many workgroups are resident, not what a chunk holds, so 40 frames (each
# meets 49 spans at its own phase)
KNOB_GENERAL = (100_000, 40)


def header_size(fs, mask):
    """co_ws_frame.c:34-91: 2 bytes, 2 or 8 of extended length, 4 of key."""
    return 2 + (8 if fs > 65535 else 2 if fs > 125 else 0) + (4 if mask else 0)


def frame_bytes(fs, mask):
    return header_size(fs, mask) + fs


def route(fs, mask):
    """uniform_route restated."""
    if 32 <= fs <= 65535 and fs % 16 == 0:
        return "small"
    return "general" if frame_bytes(fs, mask) >= 32 else "bytes"


def default_span(fs, mask, span2_min=1024):
    """The wire bytes a wave owns (small_span with CFWS_UNIFORM_SPAN2_MIN;
    kGenSpan; the bytes kernel has no waves' spans: one chunk per thread)."""
    if route(fs, mask) == "small":
        return SPAN_2K if fs >= span2_min else SPAN_SMALL
    return SPAN_2K


def period_frames(fs, mask, span=None):
    """The rule: the frames of one period of (frame, span) phase, and two."""
    W = frame_bytes(fs, mask)
    span = default_span(fs, mask) if span is None else span
    return math.lcm(W, span) // W + 2


def chunk_classes(fs, mask, n, span):
    """{(kind, header position, last of its span with a body head)} over the
    header chunks of n frames, and ("body", ph, False) for body chunks (ph:
    the source phase of the chunk's first byte)."""
    hs = header_size(fs, mask)
    W = hs + fs
    total = n * W
    D = np.arange(0, total, 16, dtype=np.int64)
    f, off = D // W, D % W
    body = (off >= hs) & (off + 16 <= W)
    own = off < hs
    tail = ~body & ~own
    has_next = f + 1 < n
    pos = np.where(own, -off, W - off)
    head = np.where(own, hs - off < 16, has_next & (W - off + hs < 16))
    last = (D // 16) % (span // 16) == span // 16 - 1
    out = set()
    ph = (f * fs + off - hs) % 16
    out |= {("body", int(p), False) for p in np.unique(ph[body])}
    for kind, sel in (("own", own), ("tail", tail & has_next)):
        code = np.unique((pos[sel] + 16) * 2 + (last[sel] & head[sel]))
        out |= {(kind, int(c) // 2 - 16, bool(c & 1)) for c in code}
    return out


def header_chunks_per_span(fs, mask, n):
    """The largest n_hdr of serialize_uniform_kernel over the batch's waves,
    with the kernel's own fa / fb: over 64, its header pass takes a second
    round."""
    hs = header_size(fs, mask)
    W = hs + fs
    D0 = np.arange(0, n * W, SPAN_2K, dtype=np.int64)
    F0 = D0 // W
    base = F0 * W
    rel0 = D0 - base
    fa = np.where(base + hs > D0, F0, F0 + 1)
    fb = np.minimum(F0 + (rel0 + SPAN_2K - 1) // W, n)
    return int(np.where(fa <= fb, 2 * (fb - fa + 1), 0).max())


SMALL_CASES = [(fs, mask) for fs in SMALL_PAYLOADS for mask in (1, 0)]
# every (fs, mask, span) a GPU test takes its n from: the default spans, and
# for the knob sweep both spans (CFWS_UNIFORM_SPAN2_MIN=0 / 2^30)
COVERED = sorted(
    {(fs, m, default_span(fs, m)) for fs, m in SMALL_CASES + GENERAL_SHORT + BYTES_NEIGHBOURS} |
    {(256, m, SPAN_SMALL) for m in (1, 0)} |
    {(fs, m, s)
     for fs in KNOB_PAYLOADS for m in (1, 0) for s in (SPAN_SMALL, SPAN_2K)})


def frames_for(fs, mask, otherwise=700):
    """n by the rule where the table above has the case on its default span."""
    return period_frames(fs, mask) if (fs, mask, default_span(fs, mask)) in COVERED else otherwise


@pytest.mark.parametrize("fs,mask,span", COVERED)
def test_one_period_reaches_every_class(fs, mask, span):
    n = period_frames(fs, mask, span)
    assert n <= 2050
    # 33.7 MB of wire at the most on the default spans; the knob sweep's
    # 65,520-byte unmasked frames on 4 KiB spans twice that
    assert n * frame_bytes(fs, mask) <= (34 << 20) * (1 if span == default_span(fs, mask) else 2)
    one = chunk_classes(fs, mask, n, span)
    two = chunk_classes(fs, mask, 2 * n, span)
    assert one == two, sorted(two - one)


def test_small_cases_take_the_small_kernel_and_their_classes():
    """7-bit-length headers (hs 2 / 6) put a header at 8 positions of a
    chunk, 16-bit ones (hs 4 / 8) at 4 or 2; each case meets a header at the
    start of a chunk, one that ends its chunk with no head after it, a head
    at the last chunk of a span and, with 6-byte headers, a header that its
    chunk cuts (an own chunk at a negative position)."""
    for fs, mask in SMALL_CASES:
        assert route(fs, mask) == "small"
        hs = header_size(fs, mask)
        span = default_span(fs, mask)
        c = chunk_classes(fs, mask, period_frames(fs, mask), span)
        hdr = {x for x in c if x[0] != "body"}
        positions = {p % 16 for _, p, _ in hdr if p >= 0}
        assert len(positions) == 16 // math.gcd(hs, 16), (fs, mask, sorted(positions))
        assert any(last for _, _, last in hdr), (fs, mask)
        assert ("own", 0, False) in hdr
        # headers start at multiples of gcd(hs, 16): only a 6-byte one is cut
        assert any(k == "own" and p < 0 for k, p, _ in hdr) == (hs == 6), (fs, mask)
        assert any(k == "tail" and p + hs >= 16 for k, p, _ in hdr), (fs, mask)
        # W and hs are even, so a header ends at an even chunk byte: the
        # shortest head is 2 bytes (hs 2 / 6; 4 bytes at hs 4, 8 at hs 8)
        assert all((p + hs) % 2 == 0 for _, p, _ in hdr), (fs, mask)
        assert any(p + hs == 14 for _, p, _ in hdr) == (hs in (2, 6)), (fs, mask)
        # the header chunks and the body chunk
        if fs <= 125:
            assert 16 <= len(hdr) + 1 <= 18, (fs, mask, len(hdr))
        else:
            assert 4 <= len(hdr) + 1 <= 8, (fs, mask, len(hdr))


def test_general_short_frames_take_a_second_header_round():
    """serialize_uniform_kernel hands out 64 header chunks a round, two per
    frame whose header meets the 2 KiB span: frames of up to 63 wire bytes
    put 33 or more headers into some span (a second round); 64..66 bytes
    exactly 32, a full first round, and 67 one short of it."""
    for fs, mask in GENERAL_SHORT:
        assert route(fs, mask) == "general"
        W = frame_bytes(fs, mask)
        assert 32 <= W <= 67
        n_hdr = header_chunks_per_span(fs, mask, period_frames(fs, mask))
        if W <= 63:
            assert n_hdr > 64, (fs, mask, n_hdr)
        else:
            assert n_hdr == (64 if W <= 66 else 62), (fs, mask, n_hdr)
    assert sum(frame_bytes(fs, m) <= 63 for fs, m in GENERAL_SHORT) == 10   # of the 16
    for fs, mask in BYTES_NEIGHBOURS:
        assert route(fs, mask) == "bytes" and frame_bytes(fs, mask) == 31
    # the frames tested before this table: never a second round
    for fs in (100, 125, 126, 127, 250, 257, 300, 1000, 1023):
        assert header_chunks_per_span(fs, 1, 5000) <= 64
