"""UTF-8 check of received text messages on the host
(cfws_utf8_check_messages, include/cfws.h) against the model
of tests/utf8_util.py, whose oracle is CPython's strict decoder.

* every string of length 1-4 over the alphabet, 346,200 messages in one call;
* which messages are checked, and how FINAL / CUT / OPEN count a truncated end;
* carried bytes across two calls, at every cut of a 64-byte window, with and
  without a probe; carry values the library never emits;
* the BAD list against its capacity;
* the walk, built with -fsanitize=address,undefined into a stand-alone
  program, over exact-size heap arrays.

The device form: tests/test_gpu_utf8.py.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import utf8_util as U
from conftest import ROOT

from coldforce_amd import cfws


def host(arena, rows, carry_in=None, payload_bytes=None, bad_capacity=None):
    return cfws.utf8_check_messages(arena, rows, carry_in, bad_capacity, payload_bytes)


def same(got, exp, what=""):
    U.same_rows(got[0], exp[0], what)
    assert np.array_equal(got[1], exp[1]), what
    assert got[2:] == exp[2:], what


def test_result_row_and_exports():
    assert cfws.UTF8_RESULT_DTYPE.itemsize == 16
    names = {"cfws_utf8_check_messages", "cfws_utf8_workspace_size", "cfws_utf8_piece_bytes",
             "cfws_utf8_messages_batch"}
    assert names <= set(cfws.BATCH_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", cfws.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert names <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_the_decoder_sees_all_three_classes():
    """What the issue counted of the length-4 strings: the oracle itself."""
    arena, rows, (res, bad, checked, n_bad) = U.exhaustive()
    four = res["flags"][rows["payload_size"] == 4]
    assert [int((four & k != 0).sum()) for k in (U.VALID, U.TRUNCATED, U.INVALID)] == [1672, 3816, 326288]
    assert checked == len(rows) and n_bad == len(bad) == int((res["flags"] & U.BAD != 0).sum())


def test_every_short_string_over_the_alphabet():
    arena, rows, exp = U.exhaustive()
    same(host(arena, rows), exp, "exhaustive")


def test_probes_alone_and_inside_text():
    rng = np.random.default_rng(1)
    strings = list(U.PROBES) + [U.valid_text(rng, 37) + p + U.valid_text(rng, 21) for p in U.PROBES]
    strings += [p + b"tail" for p in U.PROBES] + [U.valid_text(rng, 64) + p for p in U.PROBES]
    arena, rows = U.pack(strings)
    rows["flags"][::3] = U.OPEN
    same(host(arena, rows), U.model(arena, rows), "probes")


def test_selection_and_end_flags():
    arena, rows, carry = U.selection_case()
    exp = U.model(arena, rows, carry)
    same(host(arena, rows, carry), exp, "with carry_in")
    f = exp[0]["flags"].tolist()
    ok, cut = U.CHECKED | U.VALID, U.CHECKED | U.TRUNCATED
    assert f == [ok, cut | U.BAD, cut, cut | U.BAD, U.CHECKED | U.INVALID | U.BAD, ok, 0, ok, ok, 0, 0, 0, 0, 0]
    assert exp[0]["prefix"][4] == 2 and exp[0]["carry"][2] == U.carry_word(U.CHARS[1][:2], text=False)
    assert exp[2:] == (8, 3) and exp[1].tolist() == [1, 3, 4]
    # without carry_in no CONTINUATION is text, and the HEADLESS rows' bytes stand alone
    none = U.model(arena, rows, None)
    same(host(arena, rows, None), none, "without carry_in")
    assert none[0]["flags"][5] == 0 and none[2:] == (7, 3)
    # the arena's last row ends at payload_bytes: one byte less and it is not checked
    short = U.model(arena, rows, carry, payload_bytes=len(arena) - 1)
    same(host(arena, rows, carry, payload_bytes=len(arena) - 1), short, "payload_bytes - 1")
    assert short[0]["flags"][8] == 0 and short[2] == 7


@pytest.mark.parametrize("probe", [None] + list(range(len(U.PROBES))))
def test_carry_across_two_calls(probe):
    whole = U.cut_text(None if probe is None else U.PROBES[probe])
    heads, tails = U.cut_rows(whole)
    r1 = host(whole, heads)
    same(r1, U.model(whole, heads), "heads")
    carry = r1[0]["carry"] | np.uint32(U.CARRY_TEXT)
    r2 = host(whole, tails, carry)
    same(r2, U.model(whole, tails, carry), "tails")
    U.check_cut(whole, r1[0], r2[0], f"probe {probe}")
    if probe is None or probe < len(U.CHARS):
        assert r1[3] == 0 and r2[3] == 0 and (r2[0]["flags"] == U.CHECKED | U.VALID).all()
        assert (r1[0]["carry"] != 0).any() and (r1[0]["carry"] == 0).any()


def test_carry_values_the_library_never_emits():
    """S = carry ++ bytes, whatever the carry holds."""
    bodies = [b"\xa9ok", b"\x82\xac", b"", b"\x80", b"abc", b"\x9f\x98\x80"]
    words = [U.carry_word(b"\x41\xc2"), U.carry_word(b"\x80\x80\x80"), U.carry_word(b"\xc3"), U.carry_word(b"\xf0\x9f\x98"),
             U.carry_word(b"\xe2\x82\xac"), 0x03FFFFFF | U.CARRY_TEXT]
    strings = [b for b in bodies for _ in words]
    carry = np.array(words * len(bodies), dtype=np.uint32)
    arena, rows = U.pack(strings, U.CONT, U.HEADLESS | U.FINAL)
    exp = U.model(arena, rows, carry)
    same(host(arena, rows, carry), exp, "odd carries")
    assert exp[0]["flags"][0] == U.CHECKED | U.VALID and exp[0]["prefix"][0] == 3          # 41 C2 A9 6F 6B
    assert exp[0]["flags"][1] & U.INVALID and exp[0]["prefix"][1] == 0                     # 80 80 80 ...
    assert exp[0]["flags"][2 * len(words) + 2] == U.CHECKED | U.TRUNCATED | U.BAD          # C3 alone, FINAL


def test_bad_list_against_its_capacity():
    arena, rows, exp = U.exhaustive()
    arena, rows = arena[:24 + 2 * 576], rows[:24 + 576]
    exp = U.model(arena, rows)
    total = exp[3]
    assert total > 3
    for cap in (0, 1, total, total + 1):
        result = np.zeros(len(rows), dtype=cfws.UTF8_RESULT_DTYPE)
        bad = np.full(cap + 2, 0xEEEEEEEE, dtype=np.uint32)
        counts = np.zeros(2, dtype=np.uint64)
        nb = cfws.lib().cfws_utf8_check_messages(arena, len(arena), rows.ctypes.data, len(rows), None,
                                                 result.ctypes.data, bad.ctypes.data if cap else None, cap,
                                                 counts.ctypes.data)
        assert nb == total and counts.tolist() == [exp[2], total], cap
        k = min(cap, total)
        assert np.array_equal(bad[:k], exp[1][:k]) and (bad[k:] == 0xEEEEEEEE).all(), cap
        U.same_rows(result, exp[0], f"capacity {cap}")


def test_sanitized_walk_over_exact_size_heap_arrays(tmp_path):
    """The host walk built with AddressSanitizer + UBSan into a stand-alone
    program (make build/utf8_asan), over the exhaustive call, the selection
    rows and the carry cases, the payload a heap allocation of exactly its
    size: no report, and every run equals the model."""
    cases = []
    arena, rows, exp = U.exhaustive()
    cases.append((arena, len(arena), rows, None, exp))
    arena, rows, carry = U.selection_case()
    for cin, pb in ((carry, len(arena)), (None, len(arena)), (carry, len(arena) - 1)):
        cases.append((arena, pb, rows, cin, U.model(arena, rows, cin, payload_bytes=pb)))
    for probe in [None] + U.PROBES:
        whole = U.cut_text(probe)
        heads, tails = U.cut_rows(whole)
        e1 = U.model(whole, heads)
        carry = e1[0]["carry"] | np.uint32(U.CARRY_TEXT)
        cases += [(whole, len(whole), heads, None, e1), (whole, len(whole), tails, carry, U.model(whole, tails, carry))]
    path, out = tmp_path / "cases.bin", tmp_path / "out.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for arena, pb, rows, cin, _ in cases:
            f.write(struct.pack("<QQII", len(arena), pb, len(rows), 0 if cin is None else 1))
            f.write(arena)
            f.write(np.ascontiguousarray(rows, cfws.MESSAGE_DTYPE).tobytes())
            if cin is not None:
                f.write(np.ascontiguousarray(cin[:len(rows)], np.uint32).tobytes())
    mk = subprocess.run(["make", "-s", "-C", ROOT, "build/utf8_asan"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    r = subprocess.run([os.path.join(ROOT, "build", "utf8_asan"), str(path), str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    blob, at = out.read_bytes(), 0
    for i, (_, _, rows, _, exp) in enumerate(cases):
        checked, n_bad = struct.unpack_from("<QQ", blob, at)
        at += 16
        assert (checked, n_bad) == exp[2:], i
        got = np.frombuffer(blob, cfws.UTF8_RESULT_DTYPE, len(rows), at)
        at += 16 * len(rows)
        U.same_rows(got, exp[0], f"case {i}")
        assert np.array_equal(np.frombuffer(blob, np.uint32, n_bad, at), exp[1]), i
        at += 4 * n_bad
    assert at == len(blob)
