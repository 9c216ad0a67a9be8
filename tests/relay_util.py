"""What cfws_relay_batch (include/cfws.h) must produce, written once and from
the oracle only: the oracle's packed deserialize, a send descriptor per
emitted frame, the oracle's serialize. Also the seeded input wires that the
golden cases (tests/golden/relay_cases.json) and the GPU tests share."""
import random

import numpy as np

import oracle as O

VERBATIM, ECHO_SERVER = 0, 1


def decision(policy, status, fin, opcode):
    """(emit, fin', opcode') of one parsed frame (include/cfws.h, relay)."""
    if status != O.PARSE_COMPLETE:
        return False, fin, opcode
    if policy == VERBATIM or opcode <= 2:
        return True, fin, opcode
    if opcode == 9:
        return True, 1, 0xA
    return False, fin, opcode


def expect_relay(wire, wire_size, starts, policy, out_mask, out_keys, max_payload=O.DEFAULT_MAX_PAYLOAD):
    """Returns (out wire, per-frame out offsets, desc, status): desc / status
    as the parse writes them, desc.payload_off = the frame's out offset."""
    wire = np.ascontiguousarray(wire[:wire_size], dtype=np.uint8)
    starts = np.ascontiguousarray(starts, dtype=np.uint64)
    n = len(starts)
    pd, ps = O.parse_headers(wire, starts, max_payload)
    room = int(pd["payload_size"][ps == 0].sum()) + 16
    arena, desc, status, _ = O.deserialize_batch(wire, starts, align=1, max_payload=max_payload, capacity=room)
    assert np.array_equal(status, ps)
    # decision(), for every frame at once
    op = desc["opcode"]
    emit = (status == O.PARSE_COMPLETE) & ((policy == VERBATIM) | (op <= 2) | (op == 9))
    pong = (policy == ECHO_SERVER) & (op == 9)
    send = np.zeros(n, dtype=O.DESC_DTYPE)
    send["payload_off"] = desc["payload_off"]
    send["payload_size"] = desc["payload_size"]
    send["mask_key"] = np.asarray(out_keys, dtype=np.uint32)[:n] if out_mask else 0
    send["fin"] = np.where(pong, 1, desc["fin"])
    send["opcode"] = np.where(pong, 0xA, op)
    send["mask"] = 1 if out_mask else 0
    out, sent = O.serialize_batch(arena, send[emit])
    nbytes = np.zeros(n, dtype=np.uint64)
    nbytes[emit] = sent["payload_size"] + sent["header_size"].astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.uint64) if n else nbytes
    assert np.array_equal(offs[emit], sent["wire_off"]) and int(nbytes.sum()) == len(out)
    desc = desc.copy()
    desc["payload_off"] = offs
    return out, offs, desc, status


def frames_wire(sizes, in_masks, fins, opcodes, seed, bad_b0=()):
    """An input wire: frame i of sizes[i] payload bytes (splitmix payloads,
    keys from `seed`), serialized by the oracle; frames listed in bad_b0 get
    a reserved bit set in byte 0 (opcode bits > 0x0f: INVALID_FRAME).
    Returns (wire, starts)."""
    n = len(sizes)
    sizes = np.asarray(sizes, dtype=np.uint64)
    payload = O.fill_splitmix(max(int(sizes.sum()), 16), seed, 0)
    d = np.zeros(n, dtype=O.DESC_DTYPE)
    d["payload_off"] = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64) if n else sizes
    d["payload_size"] = sizes
    d["mask_key"] = (O.splitmix_words(seed ^ 0x6B6579, 0, n) >> np.uint64(13)).astype(np.uint32)
    d["fin"] = np.asarray(fins, dtype=np.uint8)
    d["opcode"] = np.asarray(opcodes, dtype=np.uint8)
    d["mask"] = np.asarray(in_masks, dtype=np.uint8)
    wire, d = O.serialize_batch(payload, d)
    wire = wire.copy()
    for i in bad_b0:
        wire[int(d["wire_off"][i])] |= 0x40
    return wire, d["wire_off"].astype(np.uint64)


GOLDEN_SIZES = [0, 1, 15, 16, 17, 125, 126, 127, 200, 1000, 5000, 65535, 65536]
GOLDEN_MAX_PAYLOAD = 65535          # the 65,536-byte frames are DATA_TOO_BIG


def golden_input(seed, n, cut):
    """The golden cases' input, from its seed: n frames of boundary sizes,
    mixed masks, fins and opcodes (data, CLOSE, PING, PONG), about one in nine
    with an invalid byte 0, the wire cut `cut` bytes before its end (the last
    frame MORE_DATA). Returns (wire, wire_size, starts, max_payload)."""
    rng = random.Random(seed)
    sizes, masks, fins, ops = [], [], [], []
    for _ in range(n):
        op = rng.choice([0, 1, 2, 8, 9, 10])
        sizes.append(rng.choice(GOLDEN_SIZES[:8]) if op >= 8 else rng.choice(GOLDEN_SIZES))
        masks.append(rng.random() < .6)
        fins.append(rng.random() < .7)
        ops.append(op)
    bad = [i for i in range(n) if rng.random() < 1 / 9]
    wire, starts = frames_wire(sizes, masks, fins, ops, seed, bad)
    return wire, len(wire) - cut, starts, GOLDEN_MAX_PAYLOAD
