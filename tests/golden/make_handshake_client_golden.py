#!/usr/bin/env python3
"""Generate tests/golden/handshake_client_cases.json from the REFERENCE itself
(oracle/_ref/libcfws_ref.so, after `make ref`): its own co_random,
co_base64_encode, co_base64_decode and co_ws_frame_serialize, called in place.

  client       per seed and first_draw: srandom(seed), first_draw draws
               discarded, then the keys of 40 consecutive
               co_http_request_create_ws_upgrade key draws
               (co_ws_http_extension.c:280-290: co_random of 16 bytes,
               co_base64_encode with padding) and the accept value of the
               first 4 (co_sha1 + co_base64_encode, :26-57);
  then_frames  srandom(1234), 37 key draws, then 50 masked
               co_ws_frame_serialize calls: the mask keys read back from the
               frames (the key stream goes on where the upgrade keys left it);
  decode       co_base64_decode's return value and *dest_length
               (co_base64.c:94-167) for hand-picked keys and for 2,000 keys
               with 0-3 random edits (tests/handshake_util.edited_keys).

Usage: python tests/golden/make_handshake_client_golden.py"""
import base64
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O  # noqa: E402
import handshake_util as HU  # noqa: E402

SEEDS = (1, 1234, 0xFFFFFFFF)
FIRST = (0, 1, 2, 3, 1000003)
CLIENT_KEYS, CLIENT_ACCEPTS = 40, 4
THEN_SEED, THEN_KEYS, THEN_FRAMES = 1234, 37, 50
EDITED, EDIT_SEED = 2000, 0x4B455953

RFC_KEY = b"dGhlIHNhbXBsZSBub25jZQ=="


def picked_keys():
    d22 = RFC_KEY[:22]
    return [
        RFC_KEY, d22, d22 + b"=",                                   # padded, unpadded, one '='
        b"A" * 21, b"A" * 22, b"A" * 23,                            # 15, 16, 17
        b"!-:_" * 5 + b"!-==", b"!-:_" * 6,
        RFC_KEY[:10] + b"\r\n" + RFC_KEY[10:], d22 + b"\r\n", b"\r\n" + RFC_KEY,
        b"=", b"", b"=" * 24 + b"A" * 8,
        b"\x80" * 22, b"\xff" * 22 + b"==", d22[:21] + b"\x80==", b"\x80", b"\x7f" * 22,
        RFC_KEY[:5] + b" " + RFC_KEY[5:], RFC_KEY[:5] + b"*" + RFC_KEY[6:], b"@" + d22, d22 + b"\0", b"\0" * 22,
        b"[" * 22, b"`" * 22, b"{" * 22,
        b"A" * 266 + b"=" * 734,                                    # 1,000 bytes: 750 - 734 = 16
        b"=" * 734 + b"A" * 266, b"A" * 1000,
    ]


def client_cases(R):
    out = []
    for seed in SEEDS:
        for first in FIRST:
            O.srandom(R, seed)
            HU.ref_random(R, first)                                 # first_draw calls of random() discarded
            keys = [HU.ref_client_key(R) for _ in range(CLIENT_KEYS)]
            out.append({"seed": seed, "first_draw": first, "keys": [k.decode() for k in keys],
                        "accepts": [O.ref_ws_accept_key(R, k) for k in keys[:CLIENT_ACCEPTS]]})
    return out


def then_frames(R):
    O.srandom(R, THEN_SEED)
    keys = [HU.ref_client_key(R).decode() for _ in range(THEN_KEYS)]
    mask_keys = []
    for i in range(THEN_FRAMES):
        f = O.ref_serialize(R, True, 2, True, bytes([i]) * (i % 7))
        mask_keys.append("%08x" % int.from_bytes(f[2:6], "little"))
    return {"seed": THEN_SEED, "keys": keys, "mask_keys": mask_keys}


def decode_cases(R):
    keys = picked_keys() + HU.edited_keys(random.Random(EDIT_SEED), EDITED)
    out = []
    for k in keys:
        ok, length = HU.ref_decode(R, k)
        out.append([k.hex(), int(ok), length])                      # key, return value, nonce_length
    gen = out[len(picked_keys()):]
    valid = sum(1 for _, ok, length in gen if ok and length == HU.NONCE)
    assert 4 * valid >= len(gen) and 4 * (len(gen) - valid) >= len(gen), (valid, len(gen))
    print(f"decode: {valid} of {len(gen)} generated keys valid")
    return out


def main():
    R = O.ref_lib("O2")
    if R is None:
        sys.exit("oracle/_ref not built: run `make ref`")
    assert HU.ref_encode(R, base64.b64decode(RFC_KEY)) == RFC_KEY
    cases = {"client": client_cases(R), "then_frames": then_frames(R), "decode": decode_cases(R)}
    with open(os.path.join(HERE, "handshake_client_cases.json"), "w") as f:
        json.dump(cases, f, separators=(",", ":"))
        f.write("\n")
    print("wrote handshake_client_cases.json")


if __name__ == "__main__":
    main()
