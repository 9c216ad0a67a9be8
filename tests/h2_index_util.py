"""What cfws_h2_index_frames / cfws_h2_index_frames_batch (include/cfws.h)
must produce, written once in plain Python and independently of the library:
the walk of the reference's HTTP/2 receive loop (co_http2_client.c:462-541)
around co_http2_frame_deserialize (co_http2_frame.c:211-533), plus the frame
builders and the fixture's blob coding the index tests share.

tests/golden/h2_index_cases.json pins this model to the reference itself."""
from __future__ import annotations

import numpy as np

COMPLETE, MORE_DATA, ERROR, INDEX_FULL = 0, 1, -1, 2
ALL, DATA_ONLY = 0, 1
T_DATA, T_HEADERS, T_PRIORITY, T_RST, T_SETTINGS, T_PUSH, T_PING, T_GOAWAY, T_WINUP, T_CONT = range(10)
F_END_STREAM, F_PADDED, F_PRIORITY = 0x1, 0x8, 0x20

INFO_DTYPE = np.dtype([("stream_id", "<u4"), ("length", "<u4"), ("advance", "<u4"),
                       ("type", "u1"), ("flags", "u1"), ("zero", "<u2")])
assert INFO_DTYPE.itemsize == 16


def hop(buf, p: int, e: int, max_frame: int):
    """One step at p of a buffer ending at e (e > p):
    (status, type, flags, sid, length, advance, undefined). `undefined` marks
    the frames the reference has no defined behaviour for (need > length):
    ERROR there is the library's own rule."""
    if e - p < 9:
        return MORE_DATA, 0, 0, 0, 0, 0, False
    length = int(buf[p]) << 16 | int(buf[p + 1]) << 8 | int(buf[p + 2])
    if length > max_frame:
        return ERROR, 0, 0, 0, 0, 0, False
    if e - p - 9 < length:
        return MORE_DATA, 0, 0, 0, 0, 0, False
    typ, flags = int(buf[p + 3]), int(buf[p + 4])
    if typ > 9:
        return ERROR, 0, 0, 0, 0, 0, False
    padded = 0
    if typ in (T_DATA, T_HEADERS, T_PUSH) and flags & F_PADDED:
        if length < 1:
            return ERROR, 0, 0, 0, 0, 0, True
        padded = 1 + int(buf[p + 9])
    need = {T_DATA: padded,
            T_HEADERS: padded + (5 if flags & F_PRIORITY else 0),
            T_PRIORITY: 5, T_RST: 4, T_SETTINGS: 0, T_PUSH: padded + 4,
            T_PING: 8, T_GOAWAY: 8, T_WINUP: 4, T_CONT: 0}[typ]
    if need > length:
        return ERROR, 0, 0, 0, 0, 0, True
    advance = {T_PRIORITY: 14, T_RST: 13, T_WINUP: 13, T_PING: 17,
               T_SETTINGS: 9 + 6 * ((length // 6) % 65536)}.get(typ, 9 + length)
    sid = int(buf[p + 5]) << 24 | int(buf[p + 6]) << 16 | int(buf[p + 7]) << 8 | int(buf[p + 8])
    return COMPLETE, typ, flags, sid, length, advance, False


def expect_h2_index(buf, begin: int, end: int, max_frame: int, select: int, stream_id: int,
                    max_starts: int | None = None):
    """(starts u64[k], info INFO_DTYPE[k], consumed, stop) of the walk over
    buf[begin, end). max_frame 0 = 16384; max_starts None = no limit."""
    max_frame = max_frame or 16384
    starts, info = [], []
    p, stop = begin, COMPLETE
    if select > 1:
        return np.zeros(0, np.uint64), np.zeros(0, INFO_DTYPE), begin, ERROR
    while end > p:
        stop, typ, flags, sid, length, advance, _ = hop(buf, p, end, max_frame)
        if stop != COMPLETE:
            break
        if (select == ALL or typ == 0) and (stream_id == 0 or sid == stream_id):
            if max_starts is not None and len(starts) == max_starts:
                stop = INDEX_FULL
                break
            starts.append(p)
            info.append((sid, length, advance, typ, flags, 0))
        p += advance
    return (np.array(starts, dtype=np.uint64), np.array(info, dtype=INFO_DTYPE).reshape(-1),
            p, stop)


def frame(typ: int, flags: int, sid: int, payload: bytes = b"", length: int | None = None) -> bytes:
    """An HTTP/2 frame: 9-byte header + payload. `length` overrides the
    header's length field (for frames that lie about it)."""
    n = len(payload) if length is None else length
    return bytes([n >> 16 & 0xff, n >> 8 & 0xff, n & 0xff, typ & 0xff, flags & 0xff]) + \
        (sid & 0xffffffff).to_bytes(4, "big") + payload


def random_frame(rng, sids=(1, 3, 0x80000005), quirk: float = 0.0, data: float = 0.5,
                 max_payload: int = 40) -> bytes:
    """One random frame of any type; with probability `quirk` one the walk
    treats specially: a fixed-size control frame with another length, bad
    padding, a type above 9, or a length above 16384."""
    sid = int(rng.choice(sids))
    if rng.random() < quirk:
        q = int(rng.integers(6))
        if q == 0:      # fixed-size type with a longer or shorter length
            typ, fixed = [(T_PRIORITY, 5), (T_RST, 4), (T_PING, 8), (T_WINUP, 4), (T_GOAWAY, 8)][int(rng.integers(5))]
            return frame(typ, 0, sid, rng.bytes(max(fixed + int(rng.integers(-2, 4)), 0)))
        if q == 1:      # SETTINGS of any length
            return frame(T_SETTINGS, 0, 0, rng.bytes(int(rng.integers(0, 20))))
        if q == 2:      # padded with a pad length that may not fit
            typ = [T_DATA, T_HEADERS, T_PUSH][int(rng.integers(3))]
            n = int(rng.integers(0, 8))
            body = (bytes([int(rng.integers(0, 10))]) + rng.bytes(n)) if n else b""
            return frame(typ, F_PADDED | (F_PRIORITY if rng.random() < .3 else 0), sid, body)
        if q == 3:
            return frame(int(rng.integers(10, 256)), 0, sid, rng.bytes(3))
        if q == 4:
            return frame(T_DATA, 0, sid, rng.bytes(4), length=16385 + int(rng.integers(100)))
        return frame(T_HEADERS, F_PRIORITY, sid, rng.bytes(int(rng.integers(0, 8))))
    if rng.random() < data:
        n = int(rng.integers(0, max_payload + 1))
        if rng.random() < .15:
            pad = int(rng.integers(0, 4))
            return frame(T_DATA, F_PADDED | (F_END_STREAM if rng.random() < .3 else 0), sid,
                         bytes([pad]) + rng.bytes(n) + b"\0" * pad)
        return frame(T_DATA, F_END_STREAM if rng.random() < .3 else 0, sid, rng.bytes(n))
    typ = int(rng.integers(1, 10))
    if typ == T_HEADERS:
        pri = rng.random() < .4
        return frame(typ, 0x4 | (F_PRIORITY if pri else 0), sid, rng.bytes((5 if pri else 0) + int(rng.integers(12))))
    if typ == T_PUSH:
        return frame(typ, 0x4, sid, rng.bytes(4 + int(rng.integers(12))))
    if typ == T_SETTINGS:
        return frame(typ, 0, 0, rng.bytes(6 * int(rng.integers(0, 4))))
    if typ == T_GOAWAY:
        return frame(typ, 0, 0, rng.bytes(8 + int(rng.integers(6))))
    if typ == T_CONT:
        return frame(typ, 0x4, sid, rng.bytes(int(rng.integers(12))))
    return frame(typ, 0, sid, rng.bytes({T_PRIORITY: 5, T_RST: 4, T_PING: 8, T_WINUP: 4}[typ]))


def random_buffer(rng, n_frames: int, quirk: float = 0.0, cut: bool = False, **kw) -> bytes:
    b = b"".join(random_frame(rng, quirk=quirk, **kw) for _ in range(n_frames))
    if cut and b:
        b = b[:int(rng.integers(0, len(b) + 1))]
    return b


# ---- fixture blob coding: a list of hex strings and [byte, count] runs --------

def encode_blob(b: bytes, min_run: int = 48) -> list:
    out, lit, i, n = [], bytearray(), 0, len(b)
    while i < n:
        j = i
        while j < n and b[j] == b[i]:
            j += 1
        if j - i >= min_run:
            if lit:
                out.append(bytes(lit).hex())
                lit = bytearray()
            out.append([b[i], j - i])
        else:
            lit += b[i:j]
        i = j
    if lit:
        out.append(bytes(lit).hex())
    return out


def decode_blob(parts: list) -> bytes:
    return b"".join(bytes.fromhex(x) if isinstance(x, str) else bytes([x[0]]) * x[1] for x in parts)
