"""HTTP/2 DATA frames of many streams, by message, on the host
(cfws_h2_streams_from_frames, include/cfws.h).

* cfws_h2_streams_from_frames equals the model (tests/h2_streams_util.py: a
  dict of pools per connection, fed in arrival order) on the fixed cases, with
  a sentinel behind every count, and on 200 seeded random tables;
* the fixed cases cover what they must;
* the record is 32 bytes and the symbols are exported;
* the host form, built with -fsanitize=address,undefined into a stand-alone
  program, over exact-size heap arrays.

The device form: tests/test_gpu_h2_streams.py.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import h2_streams_util as U
from conftest import ROOT

from coldforce_amd import cfws


def same(got, exp, what=""):
    """(order, order_frame, msgs, conn_first_msg, stream_first, counts) against the model's, whole."""
    assert got[5] == exp[5], what
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), what
    assert got[2].tobytes() == exp[2].tobytes(), what
    assert np.array_equal(got[3], exp[3]), what
    assert np.array_equal(got[4], exp[4]), what


@pytest.mark.parametrize("name", sorted(U.fixed_cases()))
def test_host_form_fixed_cases(name):
    starts, info, cf = U.fixed_cases()[name]
    exp = U.expect(starts, info, cf)
    same(cfws.h2_streams_from_frames(starts, info, cf), exp, name)
    # nothing past the counts is written: a sentinel behind each
    frames, rows = exp[5][1] + exp[5][3], exp[5][0] + exp[5][2]
    n_cfm = 1 if cf is None else len(cf)
    order = np.full(frames + 2, 0xEEEEEEEEEEEEEEEE, np.uint64)
    order_frame = np.full(frames + 2, 0xEEEEEEEE, np.uint32)
    msgs = np.full((rows + 2) * 32, 0xEE, np.uint8)
    cfm = np.full(n_cfm + 2, 0xEEEEEEEEEEEEEEEE, np.uint64)
    sf = np.full(exp[5][4] + 2, 0xEEEEEEEEEEEEEEEE, np.uint64)
    counts = np.full(7, 0xEEEEEEEEEEEEEEEE, np.uint64)
    st, inf = np.ascontiguousarray(starts, np.uint64), np.ascontiguousarray(info)
    cfa = None if cf is None else np.ascontiguousarray(cf, np.uint64)
    m = cfws.lib().cfws_h2_streams_from_frames(st.ctypes.data, inf.ctypes.data, len(inf),
                                               None if cf is None else cfa.ctypes.data, 0 if cf is None else len(cf),
                                               order.ctypes.data, order_frame.ctypes.data, msgs.ctypes.data,
                                               cfm.ctypes.data, sf.ctypes.data, counts.ctypes.data)
    assert m == exp[5][0] and counts[:5].tolist() == exp[5], name
    assert np.array_equal(order[:frames], exp[0]) and (order[frames:] == 0xEEEEEEEEEEEEEEEE).all(), name
    assert np.array_equal(order_frame[:frames], exp[1]) and (order_frame[frames:] == 0xEEEEEEEE).all(), name
    assert msgs[:rows * 32].tobytes() == exp[2].tobytes() and (msgs[rows * 32:] == 0xEE).all(), name
    assert np.array_equal(cfm[:n_cfm], exp[3] if cf is not None else [0]), name
    assert (cfm[n_cfm:] == 0xEEEEEEEEEEEEEEEE).all(), name
    assert np.array_equal(sf[:exp[5][4]], exp[4]) and (sf[exp[5][4]:] == 0xEEEEEEEEEEEEEEEE).all(), name
    assert (counts[5:] == 0xEEEEEEEEEEEEEEEE).all(), name


def test_fixed_cases_cover_what_they_must():
    cs = {k: U.expect(*v) for k, v in U.fixed_cases().items()}
    C, T, F, P = U.CLOSED, U.TAIL, U.FIRST, U.PADDED
    two = cs["interleaved_two_streams"]
    assert two[1].tolist() == [1, 3, 0, 2] and two[2]["stream_id"].tolist() == [3, 5]
    assert two[2]["length_sum"].tolist() == [7, 101] and two[2]["end_frame"].tolist() == [3, 2]
    assert two[5] == [2, 4, 0, 0, 2] and two[4].tolist() == [0, 1]
    cct = cs["close_close_tail"]
    assert cct[2]["flags"].tolist() == [C | F, C, T] and cct[2]["n_data"].tolist() == [1, 2, 2]
    assert cct[2]["first"].tolist() == [0, 1, 3] and cct[5] == [2, 3, 1, 2, 1]
    assert cs["end_stream_only"][2]["n_data"].tolist() == [1] and cs["end_stream_only"][2]["length_sum"].tolist() == [0]
    assert cs["end_stream_only_after_close"][2]["n_data"].tolist() == [1, 1, 1]
    assert cs["data_on_stream_0"][1].tolist() == [1, 3] and cs["data_on_stream_0"][5] == [1, 2, 0, 0, 1]
    assert cs["only_stream_0"][5] == [0] * 5 and cs["only_stream_0"][3].tolist() == [0, 0]
    assert cs["reserved_bit_kept"][2]["stream_id"].tolist() == [1, 0x80000001]
    assert cs["reserved_bit_kept"][1].tolist() == [1, 3, 0, 2]
    assert cs["non_data_between"][1].tolist() == [4, 1, 6]
    assert cs["padded"][2]["flags"].tolist() == [C | F | P, C, C | F | P, T | P]
    assert cs["empty_connections"][3].tolist() == [0, 0, 0, 1, 1, 2, 2, 2]
    assert cs["empty_connections"][2]["conn"].tolist() == [2, 4, 4, 5]
    assert cs["empty_connections"][2]["flags"].tolist() == [C | F, C | F, T, T]
    adj = cs["same_id_adjacent_connections"]
    assert adj[2]["conn"].tolist() == [0, 1, 2] and adj[2]["n_data"].tolist() == [2, 1, 2]
    assert adj[2]["flags"].tolist() == [C | F] * 3 and adj[4].tolist() == [0, 1, 2]
    tn = cs["tail_then_same_id_closes_next_connection"]
    assert tn[2]["flags"].tolist() == [C | F, C | F, T, T] and tn[2]["n_data"].tolist() == [1, 1, 1, 1]
    assert tn[2]["conn"].tolist() == [0, 1, 0, 1] and tn[1].tolist() == [0, 2, 1, 3]
    assert cs["conn_first_above_n"][3].tolist() == [0, 1, 2, 2, 2] and cs["conn_first_above_n"][5] == [2, 2, 1, 1, 2]
    assert cs["no_conn_first"][2]["stream_id"].tolist() == [2, 4, 2] and not cs["no_conn_first"][2]["conn"].any()
    assert cs["empty_with_connections"][3].tolist() == [0, 0, 0] and cs["empty"][5] == [0] * 5
    big = cs["starts_at_and_above_2_32"]
    assert (big[0] >= (1 << 32) - 16009).all() and (big[0] >= 1 << 32).sum() == 3


def test_host_form_equals_model_on_random_tables():
    rng = np.random.default_rng(0x6832)
    seen = 0
    for t in range(200):
        conns = [None, 1, 7, 40][t % 4]
        n = int(rng.integers(0, 300))
        starts, info, cf = U.random_table(rng, n, conns, max_streams=int(rng.integers(1, 8)))
        exp = U.expect(starts, info, cf)
        same(cfws.h2_streams_from_frames(starts, info, cf), exp, t)
        seen |= int(np.bitwise_or.reduce(exp[2]["flags"])) if len(exp[2]) else 0
    assert seen == U.CLOSED | U.TAIL | U.FIRST | U.PADDED


def test_record_size_and_exports():
    assert cfws.H2_STREAM_MSG_DTYPE.itemsize == 32
    src = open(os.path.join(ROOT, "include", "cfws.h")).read()
    assert "typedef struct cfws_h2_stream_msg {   /* 32 bytes, two 16-byte stores */" in src
    names = {"cfws_h2_streams_from_frames", "cfws_h2_streams_workspace_size", "cfws_h2_streams_group_frames",
             "cfws_h2_streams_batch"}
    assert names <= set(cfws.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cfws.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert names <= exported
    G = cfws.h2_streams_group_frames()
    assert G >= 64 and G & (G - 1) == 0
    size = cfws.lib().cfws_h2_streams_workspace_size
    assert size(0, 0) > 0
    # 76 bytes per record and 4 per connection, plus the block sums
    assert 76 << 20 <= size(1 << 20, 0) < 77 << 20
    assert 4 << 20 <= size(0, 1 << 20) < (4 << 20) + 4096


def fnv1a(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_sanitized_host_form_over_exact_size_heap_arrays(tmp_path):
    """The host form built with AddressSanitizer + UBSan into a stand-alone
    program (make build/h2_streams_asan, which also asserts the record's 32
    bytes), over the fixed cases and 20 random tables with every array a heap
    allocation of exactly its size: no report, and every run equals the
    model."""
    rng = np.random.default_rng(77)
    cases = sorted(U.fixed_cases().items())
    cases += [("random%d" % t, U.random_table(rng, int(rng.integers(0, 200)), [None, 1, 9][t % 3])) for t in range(20)]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, (starts, info, cf) in cases:
            f.write(struct.pack("<II", len(info), 0xFFFFFFFF if cf is None else len(cf)))
            f.write(np.ascontiguousarray(starts, np.uint64).tobytes())
            f.write(np.ascontiguousarray(info).tobytes())
            if cf is not None:
                f.write(np.ascontiguousarray(cf, np.uint64).tobytes())
    mk = subprocess.run(["make", "-s", "-C", ROOT, "build/h2_streams_asan"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    r = subprocess.run([os.path.join(ROOT, "build", "h2_streams_asan"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [int(ln[0]) for ln in lines] == list(range(len(cases)))
    for ln in lines:
        name, (starts, info, cf) = cases[int(ln[0])]
        exp = U.expect(starts, info, cf)
        assert [int(x) for x in ln[1:6]] == exp[5], name
        cfm = np.zeros(1, np.uint64) if cf is None else exp[3]
        want = exp[0].tobytes() + exp[1].tobytes() + exp[2].tobytes() + cfm.tobytes() + exp[4].tobytes()
        assert int(ln[6], 16) == fnv1a(want), name
