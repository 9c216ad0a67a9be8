"""HTTP/2 receive-buffer frame indexing on the host (cfws_h2_index_frames,
include/cfws.h): the walk of co_http2_client.c:462-541.

* the model (tests/h2_index_util.py) equals every case of
  tests/golden/h2_index_cases.json, which the reference's own
  co_http2_frame_deserialize produced: the pin to the reference;
* cfws_h2_index_frames equals the fixture, then the model on seeded random
  buffers (all types, quirk frames, cuts, the three filter forms), on resumed
  walks and on the frames the reference leaves undefined;
* the walk, built with -fsanitize=address,undefined into a stand-alone
  program, over exact-size heap buffers.

The device form: tests/test_gpu_h2_index.py.
"""
import os
import struct
import subprocess

import numpy as np

import h2_index_util as U
from conftest import ROOT, golden

from coldforce_amd import cfws

FILTERS = [(U.ALL, 0), (U.DATA_ONLY, 0), (U.DATA_ONLY, 1)]


def fixture_cases():
    return [(c, U.decode_blob(c["blob"])) for c in golden("h2_index_cases.json")]


def rows(starts, info):
    return [[int(s), int(r["type"]), int(r["flags"]), int(r["stream_id"]), int(r["length"]), int(r["advance"])]
            for s, r in zip(starts, info)]


def same(got, exp, what=""):
    assert np.array_equal(got[0], exp[0]), what
    assert got[1].tobytes() == exp[1].tobytes(), what
    assert tuple(got[2:]) == tuple(exp[2:]), what


def test_fixture_covers_what_it_must():
    cs = {c["name"]: c for c, _ in fixture_cases()}
    assert len(cs) >= 60
    assert sum("reference" in c for c in cs.values()) >= 8
    # the 16-bit SETTINGS count, as the reference itself decided it
    assert cs["settings_length_393216_u16_count"]["frames"] == [[0, 4, 0, 0, 393216, 9]]
    assert cs["ping_longer"]["frames"] == [[0, 6, 0, 0, 10, 17]] and cs["ping_longer"]["stop"] == U.ERROR
    assert cs["data_padded_reserved_bit_sid"]["frames"][0][3] == 0x80000005
    assert cs["length_over_max_incomplete"]["stop"] == U.ERROR


def test_model_equals_reference_fixture():
    for c, blob in fixture_cases():
        s, i, consumed, stop = U.expect_h2_index(blob, c["begin"], len(blob), c["max_frame"], U.ALL, 0)
        assert rows(s, i) == c["frames"], c["name"]
        assert (consumed, stop) == (c["consumed"], c["stop"]), c["name"]
        if "reference" in c:        # the undefined frame: this library's ERROR, at that frame
            assert stop == U.ERROR and U.hop(blob, consumed, len(blob), c["max_frame"])[6], c["name"]


def test_host_walk_equals_fixture():
    for c, blob in fixture_cases():
        buf = np.frombuffer(blob, np.uint8)
        s, i, consumed, stop = cfws.h2_index_frames(buf, c["begin"], len(blob), c["max_frame"])
        assert rows(s, i) == c["frames"], c["name"]
        assert (consumed, stop) == (c["consumed"], c["stop"]), c["name"]
        assert not i["zero"].any()
        for sel, sid in FILTERS:
            same(cfws.h2_index_frames(buf, c["begin"], len(blob), c["max_frame"], sel, sid),
                 U.expect_h2_index(blob, c["begin"], len(blob), c["max_frame"], sel, sid), c["name"])


def test_host_walk_equals_model_on_random_buffers():
    rng = np.random.default_rng(0x4832)
    stops = set()
    for t in range(200):
        blob = U.random_buffer(rng, int(rng.integers(1, 40)), quirk=[0, .03, .15][t % 3], cut=t % 2 == 1)
        buf = np.frombuffer(blob, np.uint8)
        begin = int(rng.integers(0, len(blob) + 1)) if t % 7 == 6 else 0
        mf = [16384, 0, 30, (1 << 24) - 1][t % 4]
        for sel, sid in FILTERS + [(U.ALL, 3), (U.DATA_ONLY, 0x80000005)]:
            exp = U.expect_h2_index(blob, begin, len(blob), mf, sel, sid)
            same(cfws.h2_index_frames(buf, begin, len(blob), mf, sel, sid), exp, t)
            stops.add(exp[3])
    assert stops == {U.COMPLETE, U.MORE_DATA, U.ERROR}


def test_host_walk_full_and_resume():
    """A full `starts` stops at the next SELECTED frame (unselected frames
    before it are consumed); resuming from *consumed continues the walk."""
    rng = np.random.default_rng(77)
    blob = U.random_buffer(rng, 300, sids=(1, 3))[:-5]          # ends inside its last frame
    buf = np.frombuffer(blob, np.uint8)
    for sel, sid in FILTERS:
        whole = U.expect_h2_index(blob, 0, len(blob), 16384, sel, sid)
        assert len(whole[0]) > 40
        for step in (0, 1, 7):
            same(cfws.h2_index_frames(buf, 0, len(blob), 16384, sel, sid, max_starts=step),
                 U.expect_h2_index(blob, 0, len(blob), 16384, sel, sid, max_starts=step))
        got_s, got_i, pos = [], [], 0
        while True:
            s, i, pos2, stop = cfws.h2_index_frames(buf, pos, len(blob), 16384, sel, sid, max_starts=7)
            got_s.append(s)
            got_i.append(i)
            if stop != U.INDEX_FULL:
                pos = pos2
                break
            assert len(s) == 7 and pos2 == whole[0][7 * len(got_s)]      # the next selected frame's start
            pos = pos2
        same((np.concatenate(got_s), np.concatenate(got_i), pos, stop), whole)


def test_undefined_frames_are_errors_at_that_frame():
    seen = 0
    for c, blob in fixture_cases():
        if "reference" not in c:
            continue
        seen += 1
        # the buffer ends with the undefined frame's own last byte
        p = c["consumed"]
        length = int.from_bytes(blob[p:p + 3], "big")
        cut = blob[:p + 9 + length]
        buf = np.frombuffer(cut, np.uint8)
        s, i, consumed, stop = cfws.h2_index_frames(buf, c["begin"], len(cut), c["max_frame"])
        assert (consumed, stop) == (p, U.ERROR) and rows(s, i) == c["frames"], c["name"]
    assert seen >= 8


def test_bad_select_and_empty_ranges():
    buf = np.frombuffer(U.frame(U.T_DATA, 0, 1, b"abc"), np.uint8)
    s, i, consumed, stop = cfws.h2_index_frames(buf, 0, buf.size, select=2)
    assert (len(s), consumed, stop) == (0, 0, U.ERROR)
    s, i, consumed, stop = cfws.h2_index_frames(buf, 5, buf.size, select=7)
    assert (len(s), consumed, stop) == (0, 5, U.ERROR)
    for begin, end in ((4, 4), (9, 3), (12, 12)):
        s, i, consumed, stop = cfws.h2_index_frames(buf, begin, end)
        assert (len(s), consumed, stop) == (0, begin, U.COMPLETE)


def fnv1a(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_sanitized_walk_over_exact_size_heap_buffers(tmp_path):
    """The host walk built with AddressSanitizer + UBSan into a stand-alone
    program (make build/h2_index_asan), over every fixture blob cut at each
    length 0..24 and whole, each cut in a heap allocation of exactly its
    size: no report, and every walk equals the model."""
    cases = fixture_cases()
    path = tmp_path / "blobs.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c, blob in cases:
            f.write(struct.pack("<IIQ", c["max_frame"], c["begin"], len(blob)) + blob)
    mk = subprocess.run(["make", "-s", "-C", ROOT, "build/h2_index_asan"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    r = subprocess.run([os.path.join(ROOT, "build", "h2_index_asan"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) > 3000
    for b, cut, sel, sid, k, consumed, stop, h in lines:
        c, blob = cases[int(b)]
        cut = int(cut)
        s, i, e_consumed, e_stop = U.expect_h2_index(blob[:cut], min(c["begin"], cut), cut, c["max_frame"],
                                                     int(sel), int(sid))
        assert (int(k), int(consumed), int(stop)) == (len(s), e_consumed, e_stop), (c["name"], cut, sel, sid)
        assert int(h, 16) == fnv1a(s.tobytes() + i.tobytes()), (c["name"], cut, sel, sid)
