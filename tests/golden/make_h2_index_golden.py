"""Writes tests/golden/h2_index_cases.json from the reference itself.

Run after `make ref` (needs oracle/_ref/libcfws_ref.so, the reference codec
compiled in place):

    python tests/golden/make_h2_index_golden.py

Every case is one receive buffer. The generator loops the reference's own
co_http2_frame_deserialize over it through oracle.ref_h2_recv exactly as the
receive loop does (co_http2_client.c:462-541): parse at the receive index,
stop on a result other than COMPLETE, else go on from the index the parse
left. It records, per case,

    {name, blob, begin, max_frame,
     frames: [[start, type, flags, sid, length, advance], ...],   COMPLETE frames only
     consumed, stop}

The reference's behaviour is undefined for a frame whose fixed fields take
more payload bytes than its length (need > length: it underflows an unsigned
length or reads past the frame). The generator consults the model
(tests/h2_index_util.py) before each reference call and never hands the
reference such a frame: the case then carries "reference": "undefined", its
frames before that one come from the reference, and stop = ERROR at that
frame is the library's own rule. Blobs are lists of hex strings and
[byte, count] runs (h2_index_util.decode_blob).
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O  # noqa: E402
import h2_index_util as U  # noqa: E402
from h2_index_util import frame  # noqa: E402

OUT = os.path.join(HERE, "h2_index_cases.json")


def pay(n: int, first: int = 0xA1) -> bytes:
    """n payload bytes, all >= 0xA1: a parse that lands inside them reads a
    length far above any max_frame used here."""
    return bytes(0xA1 + (first - 0xA1 + i) % 0x5E for i in range(n))


DATA3 = frame(U.T_DATA, U.F_END_STREAM, 1, b"xyz")          # the probe's follower frame


def cases():
    c = []

    def add(name, blob, begin=0, max_frame=16384):
        c.append((name, bytes(blob), begin, max_frame))

    T = U
    well = [
        frame(T.T_DATA, 0, 1, pay(11)),
        frame(T.T_HEADERS, 0x4, 1, pay(7)),
        frame(T.T_PRIORITY, 0, 3, pay(5)),
        frame(T.T_RST, 0, 3, pay(4)),
        frame(T.T_SETTINGS, 0, 0, pay(6)),
        frame(T.T_PUSH, 0x4, 1, pay(4 + 6)),
        frame(T.T_PING, 0, 0, pay(8)),
        frame(T.T_GOAWAY, 0, 0, pay(8 + 5)),
        frame(T.T_WINUP, 0, 1, pay(4)),
        frame(T.T_CONT, 0x4, 1, pay(9)),
    ]
    add("all_types_well_formed", b"".join(well))
    for i, w in enumerate(well):
        add(f"type_{i}_well_formed", w + DATA3)

    # every row of the advance table with a length that differs from its fixed
    # size: longer (defined: the next parse lands inside the frame) and
    # shorter (need > length: undefined in the reference)
    for name, typ, fixed in (("priority", T.T_PRIORITY, 5), ("rst_stream", T.T_RST, 4),
                             ("ping", T.T_PING, 8), ("window_update", T.T_WINUP, 4),
                             ("goaway", T.T_GOAWAY, 8)):
        add(f"{name}_exact", frame(typ, 0, 0, pay(fixed)) + DATA3)
        add(f"{name}_longer", frame(typ, 0, 0, pay(fixed + 2)) + DATA3)
        add(f"{name}_shorter", frame(typ, 0, 0, pay(fixed - 1)) + DATA3)
    add("ping_length_10_zero_tail", frame(T.T_PING, 0, 0, pay(8) + b"\0\0") + DATA3)
    for n in (0, 6, 7, 12):
        add(f"settings_length_{n}", frame(T.T_SETTINGS, 0, 0, pay(n)) + DATA3)
    # the parameter count is a uint16_t: 393216 / 6 = 65536 -> 0 parameters,
    # advance 9; the next parse reads ff ff ff = 2^24 - 1, not above max_frame
    add("settings_length_393216_u16_count", frame(T.T_SETTINGS, 0, 0, b"\xff" * 393216),
        max_frame=(1 << 24) - 1)
    add("settings_length_393222_u16_count", frame(T.T_SETTINGS, 0, 0, b"\xff" * 393222),
        max_frame=(1 << 24) - 1)

    # padding and priority
    add("data_padded", frame(T.T_DATA, T.F_PADDED, 1, b"\x03" + pay(5) + b"\0\0\0") + DATA3)
    add("data_padded_all_padding", frame(T.T_DATA, T.F_PADDED, 1, b"\x04" + b"\0" * 4) + DATA3)
    add("data_padded_reserved_bit_sid", frame(T.T_DATA, T.F_PADDED | T.F_END_STREAM, 0x80000005,
                                              b"\x02" + pay(6) + b"\0\0") + DATA3)
    add("headers_priority", frame(T.T_HEADERS, T.F_PRIORITY | 0x4, 1, pay(5 + 4)) + DATA3)
    add("headers_padded_priority", frame(T.T_HEADERS, T.F_PADDED | T.F_PRIORITY | 0x4, 1,
                                         b"\x02" + pay(5 + 4) + b"\0\0") + DATA3)
    add("headers_padded", frame(T.T_HEADERS, T.F_PADDED, 1, b"\x01" + pay(3) + b"\0") + DATA3)
    add("headers_padded_priority_exact", frame(T.T_HEADERS, T.F_PADDED | T.F_PRIORITY, 1,
                                               b"\x00" + pay(5)) + DATA3)
    add("push_promise_padded", frame(T.T_PUSH, T.F_PADDED | 0x4, 1, b"\x02" + pay(4 + 3) + b"\0\0") + DATA3)
    add("push_promise_length_9", frame(T.T_PUSH, 0x4, 1, pay(9)) + DATA3)
    add("goaway_length_10", frame(T.T_GOAWAY, 0, 0, pay(10)) + DATA3)
    # need > length: undefined in the reference
    add("data_padded_length_0", DATA3 + frame(T.T_DATA, T.F_PADDED, 1) + DATA3)
    add("data_padded_pad_too_long", DATA3 + frame(T.T_DATA, T.F_PADDED, 1, b"\x05" + pay(4)) + DATA3)
    add("headers_priority_length_3", frame(T.T_HEADERS, T.F_PRIORITY, 1, pay(3)) + DATA3)
    add("headers_padded_priority_short", frame(T.T_HEADERS, T.F_PADDED | T.F_PRIORITY, 1,
                                               b"\x01" + pay(5)) + DATA3)
    add("push_promise_length_2", frame(T.T_PUSH, 0, 1, pay(2)) + DATA3)
    add("push_promise_padded_short", frame(T.T_PUSH, T.F_PADDED, 1, b"\x00" + pay(3)) + DATA3)

    # errors
    add("type_10", DATA3 + frame(10, 0, 1, pay(4)) + DATA3)
    add("type_255_first", frame(255, 0, 0, b""))
    add("length_over_max_incomplete", DATA3 + frame(T.T_DATA, 0, 1, pay(3), length=16385))
    add("length_over_small_max_incomplete", frame(T.T_DATA, 0, 1, pay(3), length=101), max_frame=100)
    add("length_equals_small_max", frame(T.T_DATA, 0, 1, pay(100)) + DATA3, max_frame=100)
    add("settings_over_small_max", frame(T.T_SETTINGS, 0, 0, pay(12)) + DATA3, max_frame=11)

    # cuts: at 0, 1, 8, 9 bytes of a frame and inside its payload
    two = frame(T.T_SETTINGS, 0, 0, pay(6)) + frame(T.T_DATA, 0, 1, pay(20))
    for cut in (0, 1, 8, 9):
        add(f"cut_first_at_{cut}", two[:cut])
    for cut in (0, 1, 8, 9, 15, 28):
        add(f"cut_second_at_{cut}", two[:15 + cut])
    add("cut_inside_ping", DATA3 + frame(T.T_PING, 0, 0, pay(8))[:16])

    # begin inside the buffer
    add("begin_inside", b"\xee" * 5 + two + DATA3, begin=5)
    add("begin_at_second_frame", two + DATA3, begin=15)
    add("begin_equals_end", two, begin=len(two))

    # a multiplexed connection: two streams' DATA frames between control frames
    mux = [
        frame(T.T_SETTINGS, 0, 0, pay(12)),
        frame(T.T_SETTINGS, 0x1, 0),
        frame(T.T_WINUP, 0, 0, pay(4)),
        frame(T.T_HEADERS, 0x4, 1, pay(10)),
        frame(T.T_HEADERS, 0x4, 3, pay(10)),
        frame(T.T_DATA, 0, 1, pay(30)),
        frame(T.T_DATA, 0, 3, pay(17)),
        frame(T.T_PING, 0, 0, pay(8)),
        frame(T.T_DATA, T.F_END_STREAM, 1, pay(5)),
        frame(T.T_WINUP, 0, 3, pay(4)),
        frame(T.T_DATA, T.F_END_STREAM, 3, pay(60)),
        frame(T.T_PING, 0x1, 0, pay(8)),
        frame(T.T_DATA, T.F_END_STREAM, 1, pay(0)),
        frame(T.T_DATA, 0, 3, pay(33)),
        frame(T.T_WINUP, 0, 0, pay(4)),
        frame(T.T_DATA, T.F_END_STREAM, 1, pay(41)),
    ]
    add("multiplexed", b"".join(mux))
    add("multiplexed_cut_tail", b"".join(mux)[:-7])
    return c


def walk_reference(R, blob: bytes, begin: int, max_frame: int):
    frames, p, stop, undefined = [], begin, U.COMPLETE, False
    while len(blob) > p:
        st, *_rest, undef = U.hop(blob, p, len(blob), max_frame)
        if undef:
            assert st == U.ERROR
            stop, undefined = U.ERROR, True
            break
        r = O.ref_h2_recv(R, blob, p, max_frame)
        if r["rc"] != 0:
            stop = r["rc"]
            assert r["index"] == p                      # a failed parse leaves the index
            break
        frames.append([p, r["type"], r["flags"], r["sid"], r["length"], r["index"] - p])
        p = r["index"]
    return frames, p, stop, undefined


def main():
    R = O.ref_lib()
    if R is None:
        sys.exit("oracle/_ref/libcfws_ref.so not built: run `make ref` first")
    out = []
    for name, blob, begin, max_frame in cases():
        frames, consumed, stop, undefined = walk_reference(R, blob, begin, max_frame)
        rec = dict(name=name, blob=U.encode_blob(blob), begin=begin, max_frame=max_frame, frames=frames,
                   consumed=consumed, stop=stop)
        if undefined:
            rec["reference"] = "undefined"
        assert U.decode_blob(rec["blob"]) == blob
        out.append(rec)
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in out) + "\n]\n")
    print(f"{len(out)} cases ({sum('reference' in r for r in out)} with an undefined last frame) -> {OUT}: "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
