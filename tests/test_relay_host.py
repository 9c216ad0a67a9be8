"""CPU checks of the relay (cfws_relay_batch, include/cfws.h): the
expectation the GPU tests compare with (tests/relay_util.expect_relay, built
from the oracle only) reproduces what the reference's own deserialize +
serialize produced (tests/golden/relay_cases.json), and the host-only parts
of the ABI: exports, workspace size, the no-device return."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import relay_util as RU
from conftest import ROOT, golden, gpu_present

LIB = os.path.join(ROOT, "coldforce_amd", "libcfws.so")
CASES = golden("relay_cases.json")


def _lib():
    L = ctypes.CDLL(LIB)
    L.cfws_workspace_size.restype = ctypes.c_size_t
    L.cfws_workspace_size.argtypes = [ctypes.c_size_t, ctypes.c_uint64]
    L.cfws_relay_workspace_size.restype = ctypes.c_size_t
    L.cfws_relay_workspace_size.argtypes = [ctypes.c_size_t, ctypes.c_uint64]
    return L


@pytest.mark.parametrize("case", CASES, ids=[f"seed{c['seed']}" for c in CASES])
def test_expectation_reproduces_the_reference(case):
    wire, wire_size, starts, max_payload = RU.golden_input(case["seed"], case["n"], case["cut"])
    assert hashlib.sha256(wire.tobytes()).hexdigest() == case["wire_sha256"]
    assert len(case["runs"]) == 4
    for run in case["runs"]:
        keys = np.array([int(k, 16) for k in run["out_keys"]], dtype=np.uint32)
        out, offs, desc, status = RU.expect_relay(wire, wire_size, starts, run["policy"], run["out_mask"], keys,
                                                  max_payload)
        what = (case["seed"], run["policy"], run["out_mask"])
        assert [int(s) for s in status] == run["status"], what
        assert len(out) == run["out_total"], what
        assert hashlib.sha256(out.tobytes()).hexdigest() == run["sha256"], what
        # the literal frames: the first emitted frames of at most 40 bytes, in order
        ends = list(offs[1:]) + [len(out)]
        short = [out[int(a):int(b)].tobytes().hex() for a, b in zip(offs, ends) if 0 < int(b) - int(a) <= 40]
        assert short[:len(run["first_frames"])] == run["first_frames"], what


def test_golden_cases_cover_every_outcome():
    st = {s for c in CASES for r in c["runs"] for s in r["status"]}
    assert {O.PARSE_COMPLETE, O.PARSE_MORE_DATA, O.ERROR_INVALID_FRAME, O.ERROR_DATA_TOO_BIG} <= st
    assert any(r["out_frames"] < sum(s == 0 for s in r["status"]) for c in CASES for r in c["runs"]
               if r["policy"] == RU.ECHO_SERVER)


def test_library_exports_the_relay():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"cfws_relay_batch", "cfws_relay_workspace_size"} <= exported


def test_relay_workspace_size():
    L = _lib()
    shapes = [(0, 0), (1, 1), (64, 4096), (65536, 1 << 32), (4 << 20, 1 << 32), (524296, 4 << 20)]
    for n, cap in shapes:
        assert L.cfws_relay_workspace_size(n, cap) >= L.cfws_workspace_size(n, cap) + 32 * n, (n, cap)
    ns = [0, 1, 255, 256, 257, 65536, 524288, 524289, 4 << 20]
    caps = [0, 1, 4095, 4096, 4097, 1 << 20, 1 << 32]
    for cap in caps:
        sizes = [L.cfws_relay_workspace_size(n, cap) for n in ns]
        assert sizes == sorted(sizes), cap
    for n in ns:
        sizes = [L.cfws_relay_workspace_size(n, cap) for cap in caps]
        assert sizes == sorted(sizes), n


@pytest.mark.skipif(gpu_present(), reason="checks the no-device return")
def test_relay_without_a_device():
    L = _lib()
    buf = (ctypes.c_uint8 * 4096)()
    rc = L.cfws_relay_batch(buf, ctypes.c_uint64(0), None, ctypes.c_size_t(0), ctypes.c_uint64(1 << 20),
                            ctypes.c_uint32(0), ctypes.c_uint8(0), None, None, None, None, ctypes.c_uint64(0),
                            None, buf, ctypes.c_size_t(4096), None)
    assert rc == -4                                        # CFWS_ERROR_NO_DEVICE
