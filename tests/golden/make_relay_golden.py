#!/usr/bin/env python3
"""Generate tests/golden/relay_cases.json from the REFERENCE codec itself
(oracle/_ref/libcfws_ref.so, after `make ref`).

Per case the input wire comes from a seed (tests/relay_util.golden_input).
For every policy and out_mask the reference's own co_ws_frame_deserialize
runs at each frame start (behind the callers' 2-byte precheck,
co_ws_client.c:202-206), and after srandom(seed) its co_ws_frame_serialize
frames each emitted payload again: the echo server's path
(examples/ws_server/main.c:54-71, co_ws_client.c:428-460, :563-600). Stored:
the statuses, the keys the reference drew (read back from its frames), the
out wire's size and SHA-256, and the first short frames as literals.

Usage: python tests/golden/make_relay_golden.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O  # noqa: E402
import relay_util as RU  # noqa: E402

CASES = [  # (seed, frames, bytes cut off the wire's end)
    (101, 24, 0), (102, 40, 1), (103, 40, 3), (104, 64, 0), (105, 12, 7), (106, 1, 0), (107, 0, 0),
]
LITERAL_MAX = 40
LITERALS = 4


def relay_by_reference(R, wire, wire_size, starts, max_payload, policy, out_mask, seed):
    data = wire[:wire_size].tobytes()
    O.srandom(R, seed)
    status, keys, frames = [], [], []
    for s in (int(x) for x in starts):
        if s > wire_size or wire_size - s < 2:                  # the callers' precheck
            status.append(O.PARSE_MORE_DATA)
            keys.append(0)
            continue
        r = O.ref_deserialize(R, data, s, max_payload)
        status.append(r["rc"])
        emit, fin, op = RU.decision(policy, r["rc"], int(r["fin"]), r["opcode"])
        if not emit:
            keys.append(0)
            continue
        payload = r["payload"][:r["payload_size"]] if r["payload"] else b""
        f = O.ref_serialize(R, bool(fin), op, bool(out_mask), payload)
        hs = O.header_size(len(payload), bool(out_mask))
        keys.append(int.from_bytes(f[hs - 4:hs], "little") if out_mask else 0)
        frames.append(f)
    return status, keys, frames


def main():
    R = O.ref_lib("O2")
    if R is None:
        sys.exit("oracle/_ref not built: run `make ref`")
    cases = []
    for seed, n, cut in CASES:
        wire, wire_size, starts, max_payload = RU.golden_input(seed, n, cut)
        runs = []
        for policy in (RU.VERBATIM, RU.ECHO_SERVER):
            for out_mask in (0, 1):
                status, keys, frames = relay_by_reference(R, wire, wire_size, starts, max_payload, policy,
                                                          out_mask, seed)
                out = b"".join(frames)
                runs.append({"policy": policy, "out_mask": out_mask, "status": status,
                             "out_keys": ["%08x" % k for k in keys], "out_total": len(out),
                             "out_frames": len(frames), "sha256": hashlib.sha256(out).hexdigest(),
                             "first_frames": [f.hex() for f in frames if len(f) <= LITERAL_MAX][:LITERALS]})
        cases.append({"seed": seed, "n": n, "cut": cut, "wire_sha256": hashlib.sha256(wire.tobytes()).hexdigest(),
                      "runs": runs})
    with open(os.path.join(HERE, "relay_cases.json"), "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")
    print("wrote relay_cases.json")


if __name__ == "__main__":
    main()
