"""TEST INFRASTRUCTURE ONLY -- the model and the inputs of the UTF-8 check's
tests (tests/test_utf8_host.py, tests/test_gpu_utf8.py; include/cfws.h,
"UTF-8 check of received text messages").

The oracle is CPython's strict decoder, bytes.decode('utf-8'): on failure
start = e.start, and the string is TRUNCATED exactly when e.reason is
'unexpected end of data', else INVALID. (Not the incremental decoder with
final=False: it waits on ED A0 / ED BF at the end of input instead of
rejecting them.) model() is a whole call: selection, carry, BAD, the BAD list
and the counts.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from coldforce_amd import cfws

TEXT, BINARY, CONT = 1, 2, 0
FINAL, CUT, OPEN, HEADLESS, LOST_BYTES = 1, 2, 4, 8, 16
CHECKED, VALID, TRUNCATED, INVALID, BAD = 1, 2, 4, 8, 16
CARRY_TEXT = 0x80000000

ALPHABET = bytes.fromhex("007F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")
assert len(ALPHABET) == 24

CHARS = [bytes.fromhex(h) for h in ("C3A9", "E282AC", "F09F9880")]         # a valid 2-, 3- and 4-byte character
PROBES = CHARS + [c[:k] for c in CHARS for k in range(1, len(c))] + [bytes.fromhex(h) for h in (
    "E08080", "EDA080", "F08F8080", "F4908080", "C080", "F5808080", "80", "C241", "E28241", "F0908041")]


def classify(s: bytes):
    """(start, kind) of the string: kind is VALID, TRUNCATED or INVALID."""
    try:
        s.decode("utf-8")
        return len(s), VALID
    except UnicodeDecodeError as e:
        return e.start, TRUNCATED if e.reason == "unexpected end of data" else INVALID


def carry_word(tail: bytes, text: bool = True) -> int:
    """The carry_in word of the bytes `tail` (at most 3)."""
    assert len(tail) <= 3
    return int.from_bytes(tail, "little") | len(tail) << 24 | (CARRY_TEXT if text else 0)


def carry_bytes(word: int) -> bytes:
    return int(word & 0xFFFFFF).to_bytes(3, "little")[:(word >> 24) & 3]


def model(payload, msgs, carry_in=None, payload_bytes=None, bad_capacity=None):
    """(result rows, bad list, checked, n_bad) of one call, by the header's rule."""
    arena = bytes(payload) if isinstance(payload, (bytes, bytearray)) else np.asarray(payload, np.uint8).tobytes()
    pb = len(arena) if payload_bytes is None else payload_bytes
    res = np.zeros(len(msgs), dtype=cfws.UTF8_RESULT_DTYPE)
    bad, checked = [], 0
    offs, sizes = msgs["payload_off"].tolist(), msgs["payload_size"].tolist()
    ops, fls = msgs["opcode"].tolist(), msgs["flags"].tolist()
    cins = [0] * len(msgs) if carry_in is None else np.asarray(carry_in, np.uint32).tolist()
    for m in range(len(msgs)):
        off, size, op, fl, cin = offs[m], sizes[m], ops[m], fls[m], cins[m]
        text = op == TEXT or (op == CONT and fl & HEADLESS and carry_in is not None and cin & CARRY_TEXT)
        if not text or fl & LOST_BYTES or off + size >= 1 << 64 or off + size > pb:
            continue
        head = carry_bytes(cin) if fl & HEADLESS else b""
        s = head + arena[off:off + size]
        start, kind = classify(s)
        flags = CHECKED | kind
        if kind == INVALID or (kind == TRUNCATED and not fl & OPEN):
            flags |= BAD
            bad.append(m)
        carry = carry_word(s[start:], text=False) if kind == TRUNCATED else 0
        res[m] = (max(start, len(head)) - len(head), carry, flags, 0, 0)
        checked += 1
    cap = len(bad) if bad_capacity is None else bad_capacity
    return res, np.array(bad[:cap], dtype=np.uint32), checked, len(bad)


def rows_of(offs, sizes, opcode=TEXT, flags=FINAL):
    """Message rows over the given ranges (one fragment each, connection 0)."""
    n = len(offs)
    r = np.zeros(n, dtype=cfws.MESSAGE_DTYPE)
    r["payload_off"], r["payload_size"] = offs, sizes
    r["first_frame"], r["n_fragments"] = np.arange(n), 1
    r["opcode"], r["flags"] = opcode, flags
    return r


def pack(strings, opcode=TEXT, flags=FINAL, base=0):
    """The strings back to back from `base` on: (arena bytes, rows)."""
    sizes = np.array([len(s) for s in strings], dtype=np.uint64)
    offs = base + np.cumsum(sizes) - sizes
    return b"\0" * base + b"".join(strings), rows_of(offs, sizes, opcode, flags)


@functools.lru_cache(maxsize=None)
def exhaustive():
    """Every string of length 1-4 over the alphabet as 346,200 text messages
    back to back: (arena bytes, rows, model). Built once per process."""
    parts, sizes = [], []
    a = np.frombuffer(ALPHABET, np.uint8)
    for ln in range(1, 5):
        grid = np.array(list(itertools.product(range(24), repeat=ln)), dtype=np.int64)
        parts.append(a[grid].reshape(-1))
        sizes.append(np.full(len(grid), ln, dtype=np.uint64))
    arena = np.concatenate(parts).tobytes()
    sizes = np.concatenate(sizes)
    assert len(sizes) == 346_200
    rows = rows_of(np.cumsum(sizes) - sizes, sizes)
    return arena, rows, model(arena, rows)


def valid_text(rng, nbytes: int, kinds=(1, 2, 3, 4)) -> bytes:
    """Exactly nbytes of well-formed UTF-8 that mixes characters of the given
    encoded lengths (the tail is filled with ASCII); long texts repeat a
    block of 64 KiB."""
    if nbytes > 1 << 18:
        return valid_text(rng, 1 << 16, kinds) * (nbytes >> 16) + valid_text(rng, nbytes & 0xFFFF, kinds)
    n = nbytes // min(kinds) + 1
    kind = rng.choice(kinds, n)
    lo = np.array([0, 0x20, 0x80, 0x800, 0x10000])[kind]
    hi = np.array([0, 0x7F, 0x800, 0x10000, 0x110000])[kind]
    cp = (lo + (rng.random(n) * (hi - lo)).astype(np.int64)).astype(np.int64)
    cp[(cp >= 0xD800) & (cp < 0xE000)] -= 0x800                      # no surrogates
    ends = np.cumsum(kind)
    k = int(np.searchsorted(ends, nbytes, side="right"))
    s = cp[:k].astype("<u4").tobytes().decode("utf-32-le").encode("utf-8")
    assert len(s) == (int(ends[k - 1]) if k else 0) <= nbytes
    return s + b"a" * (nbytes - len(s))


def same_rows(got, exp, what=""):
    """Result rows against the expected ones, whole; the first difference named."""
    g, e = np.asarray(got), np.asarray(exp)
    assert len(g) == len(e), what
    if g.tobytes() != e.tobytes():
        i = int(np.nonzero(g.view(np.uint8).reshape(len(g), 16) != e.view(np.uint8).reshape(len(e), 16))[0][0])
        raise AssertionError(f"{what}: row {i}: got {g[i]}, expected {e[i]}")


WINDOW = (70, 134)        # the 64 cuts of the carry cases
PROBE_AT = 100


def cut_text(probe: bytes | None = None) -> bytes:
    """A valid text of 200 bytes and more with a character boundary at
    PROBE_AT, where `probe` is inserted."""
    rng = np.random.default_rng(64)
    return valid_text(rng, PROBE_AT, (2, 3, 4)) + (probe or b"") + valid_text(rng, 100, (2, 3, 4))


def cut_rows(whole: bytes):
    """`whole` cut at every byte of WINDOW: the rows of the heads (TEXT, OPEN)
    and of the tails (CONTINUATION, HEADLESS | FINAL), over one arena."""
    cuts = np.arange(*WINDOW, dtype=np.uint64)
    return (rows_of(np.zeros(len(cuts), np.uint64), cuts, TEXT, OPEN),
            rows_of(cuts, len(whole) - cuts, CONT, HEADLESS | FINAL))


def check_cut(whole: bytes, r1, r2, what=""):
    """The rows of the heads and of the tails (given the heads' carry) against
    the decoder on the whole. A BAD head closes the connection. Otherwise the
    tail is BAD exactly when the whole is not valid, and the bytes before the
    whole's `start` are the head's prefix, the carried bytes when the tail
    completed their character, and the tail's prefix."""
    start, kind = classify(whole)
    for c, a, b in zip(range(*WINDOW), r1, r2):
        w = f"{what} cut {c}"
        h_start, h_kind = classify(whole[:c])
        assert a["flags"] & CHECKED and b["flags"] & CHECKED, w
        if h_kind == INVALID:
            assert a["flags"] & BAD and a["prefix"] == h_start == start, w
            continue
        assert not a["flags"] & BAD, w
        k = (int(a["carry"]) >> 24) & 3
        assert bool(b["flags"] & BAD) == (kind != VALID), w
        completed = k if (b["flags"] & VALID or b["prefix"] > 0) else 0
        assert int(a["prefix"]) + completed + int(b["prefix"]) == start, w


def selection_case():
    """Rows that exercise which messages are checked and how their end
    counts: (arena bytes, rows, carry_in). The ranges of the messages that
    are not checked lie outside the arena, so that a read of them shows under
    a sanitizer or against a guard range."""
    euro = CHARS[1]
    strings = [valid_text(np.random.default_rng(5), 40), euro[:2], euro[:2], euro[:2], b"ab\xc0\x80", euro[1:] + b"z",
               euro[1:] + b"z", b"", euro + b"!"]
    arena, rows = pack(strings)
    n = len(arena)
    rows["flags"][1:5] = [FINAL, OPEN, CUT, OPEN]                    # a truncated end: BAD, fine, BAD; invalid: BAD
    rows["opcode"][5:7], rows["flags"][5:7] = CONT, HEADLESS | FINAL  # with and without the text bit
    carry = np.zeros(len(rows) + 5, dtype=np.uint32)
    carry[5], carry[6] = carry_word(euro[:1]), carry_word(euro[:1], text=False)
    carry[0] = carry_word(b"\xe2\x82")                               # not HEADLESS: no carried bytes
    # BINARY, LOST_BYTES, a range ending past payload_bytes, one wrapping 2^64
    out = rows_of(np.array([n + 4096, n + 8192, n - 4, (1 << 64) - 8, n + 4096], dtype=np.uint64),
                  [64, 64, 5, 16, 64], TEXT, FINAL)
    out["opcode"][0] = BINARY
    out["flags"][1] |= LOST_BYTES
    out["opcode"][4], out["flags"][4] = CONT, FINAL                  # CONTINUATION, not HEADLESS, with the text bit
    carry[len(rows) + 4] = carry_word(b"", text=True)
    return arena, np.concatenate([rows, out]), carry
