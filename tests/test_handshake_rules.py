"""CPU checks of the upgrade's key handling (cfws_ws_client_keys_batch,
cfws_ws_upgrade_keys_batch, cfws_ws_check_accept_batch; include/cfws.h): the
restatement the GPU tests compare with (tests/handshake_util.py) reproduces
what the reference's own co_random, co_base64_encode, co_base64_decode and
co_ws_frame_serialize produced (tests/golden/handshake_client_cases.json) and,
where oracle/_ref is built, the reference itself on fresh keys; and the
host-only parts of the ABI: declarations, exports, the no-device return."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import handshake_util as HU
import oracle as O
from conftest import ROOT, golden, gpu_present

from coldforce_amd import cfws

LIB = os.path.join(ROOT, "coldforce_amd", "libcfws.so")
CASES = golden("handshake_client_cases.json")
NEW = ("cfws_ws_client_keys_batch", "cfws_ws_client_keys_group_conns", "cfws_ws_upgrade_keys_batch",
       "cfws_ws_check_accept_batch")


@pytest.mark.parametrize("case", CASES["client"], ids=[f"seed{c['seed']}-at{c['first_draw']}" for c in CASES["client"]])
def test_client_keys_reproduce_the_reference(case):
    n = len(case["keys"])
    keys, accepts, nxt = HU.client_keys(case["seed"], case["first_draw"], n)
    assert [k.decode() for k in keys] == case["keys"]
    assert accepts[:len(case["accepts"])] == case["accepts"]
    assert nxt == case["first_draw"] + 16 * n
    assert all(len(k) == 24 and k.endswith(b"==") for k in keys)


def test_client_fixture_covers_every_seed_and_position():
    assert {(c["seed"], c["first_draw"]) for c in CASES["client"]} == \
        {(s, f) for s in (1, 1234, 0xFFFFFFFF) for f in (0, 1, 2, 3, 1000003)}
    assert all(len(c["keys"]) == 40 and len(c["accepts"]) == 4 for c in CASES["client"])


def test_mask_keys_go_on_where_the_upgrade_keys_stop():
    t = CASES["then_frames"]
    keys, _, nxt = HU.client_keys(t["seed"], 0, len(t["keys"]))
    assert [k.decode() for k in keys] == t["keys"] and nxt == 16 * 37
    mask_keys, end = cfws.draw_mask_keys_at(len(t["mask_keys"]), None, t["seed"], nxt)
    assert ["%08x" % k for k in mask_keys] == t["mask_keys"] and len(mask_keys) == 50
    assert end == nxt + 4 * 50


def test_decode_rule_reproduces_the_reference():
    assert len(CASES["decode"]) >= 2000
    for key_hex, ok, length in CASES["decode"]:
        key = bytes.fromhex(key_hex)
        assert HU.decode_result(key) == (bool(ok), length), key
        assert HU.key_valid(key) == (bool(ok) and length == 16), key


def test_decode_fixture_covers_the_rule():
    verdict = {bytes.fromhex(h): bool(ok) and length == 16 for h, ok, length in CASES["decode"]}
    rfc = b"dGhlIHNhbXBsZSBub25jZQ=="
    assert verdict[rfc] and verdict[rfc[:22]] and verdict[rfc[:23]]
    assert not verdict[b"A" * 21] and verdict[b"A" * 22] and not verdict[b"A" * 23]
    assert verdict[b"\x80" * 22] and verdict[b"A" * 266 + b"=" * 734]
    assert not verdict[rfc[:10] + b"\r\n" + rfc[10:]] and verdict[rfc[:22] + b"\r\n"]
    assert not verdict[b"="] and not verdict[b"=" * 24 + b"A" * 8] and not verdict[rfc[:22] + b"\0"]
    share = sum(verdict.values()) / len(verdict)
    assert .25 <= share <= .75, share


def test_decode_rule_against_the_reference_live(ref_lib):
    rng = random.Random(0x11FE)
    keys = HU.edited_keys(rng, 20000)
    keys += [rng.randbytes(rng.randrange(0, 40)) for _ in range(2000)]
    valid = 0
    for k in keys:
        got = HU.ref_decode(ref_lib, k)
        assert HU.decode_result(k) == got, k
        valid += HU.key_valid(k)
    assert 5000 <= valid <= 15000                      # both verdicts well covered


def test_client_keys_against_the_reference_live(ref_lib):
    O.srandom(ref_lib, 77)
    HU.ref_random(ref_lib, 5)
    want = [HU.ref_client_key(ref_lib) for _ in range(100)]
    assert HU.client_keys(77, 5, 100)[0] == want


def test_check_restates_strcmp():
    a = b"s3pPLMBiTxaQ9kYGzzhZRbK+xOo="
    assert HU.check(a, a) and HU.check(a + b"\0\0\0", a) and HU.check(a, a + b"\0junk")
    assert not HU.check(a, a[:-1]) and not HU.check(a, a + b"=") and not HU.check(a, b"")
    assert HU.check(b"", b"") and HU.check(b"\0", b"")


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "cfws.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in cfws.BATCH_SYMBOLS
    assert re.search(r"#define\s+CFWS_WS_KEY_SLOT\s+32\b", text) and cfws.WS_KEY_SLOT == 32


def test_library_exports_the_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported


@pytest.mark.skipif(gpu_present(), reason="checks the no-device return")
def test_calls_without_a_device():
    L = ctypes.CDLL(LIB)
    buf = (ctypes.c_uint8 * 4096)()
    off = (ctypes.c_uint64 * 2)(0, 24)
    u64, sz = ctypes.c_uint64, ctypes.c_size_t
    assert L.cfws_ws_client_keys_batch(ctypes.c_uint32(1), u64(0), sz(1), buf, None, None, None) == -4
    assert L.cfws_ws_upgrade_keys_batch(buf, off, sz(1), buf, None, None, None) == -4
    assert L.cfws_ws_check_accept_batch(buf, buf, off, sz(1), buf, None, None) == -4   # CFWS_ERROR_NO_DEVICE
    assert not np.frombuffer(buf, np.uint8).any()
    L.cfws_ws_client_keys_group_conns.restype = sz
    assert L.cfws_ws_client_keys_group_conns() % 512 == 0
