"""Randomised parity sweep and API edge cases on the MI355X.

* 48 seeds of small mixed batches through serialize and deserialize: frame
  sizes from 0 B to 70 KB weighted to the sizes that hit the edge paths
  (0-20 B frames, several frames per 16-byte chunk, every header form),
  unaligned payload offsets, random fin/opcode/mask, random capacities,
  alignments and reassembly; deserialize indices include frame starts,
  mid-frame positions and positions past the end. Every result equals the
  oracle's.
* Empty batches and the error codes of the batch ABI.
"""
import random

import numpy as np
import pytest

import oracle as O
from conftest import gpu_present

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_present(), reason="needs the MI355X")]

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from test_gpu_batch import check_deserialize, check_serialize, random_desc, wire_stream  # noqa: E402

FUZZ_SIZES = [0, 0, 1, 2, 3, 5, 7, 11, 13, 14, 15, 16, 17, 20, 31, 33, 100, 125, 126, 127, 500,
              4095, 4096, 4097, 20000, 65535, 65536, 70000]


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()


@pytest.mark.parametrize("seed", range(48))
def test_fuzz_serialize_deserialize(seed):
    rng = random.Random(1000 + seed)
    payload = O.fill_splitmix(300000, seed, 0)
    n = rng.choice([1, 2, 3, 7, 64, 257, 1000, 2500])
    desc = random_desc(rng, n, payload.size, sizes=FUZZ_SIZES)
    slack = rng.choice([0, 16, 4096])
    wire, total = check_serialize(payload, desc, slack=slack, plan_execute=seed % 2 == 1)
    wire = wire[:total].copy()
    starts, _ = O.index_frames(wire, n + 1)
    idx = list(starts)
    for _ in range(rng.randrange(0, 20)):            # mid-frame and past-the-end indices
        idx.insert(rng.randrange(len(idx) + 1), rng.randrange(0, total + 40))
    idx = np.array(sorted(idx) if rng.random() < 0.5 else idx, dtype=np.uint64)
    align = rng.choice([1, 2, 16, 64, 4096])
    flags = O.DESERIALIZE_REASSEMBLE if rng.random() < 0.3 else 0
    full = int(total) + 4096 * (len(idx) + 1)
    cap = rng.choice([full, full, total // 2 + 1, 17])
    check_deserialize(wire, idx, align=align, capacity=cap, flags=flags,
                      max_payload=rng.choice([O.DEFAULT_MAX_PAYLOAD, 1000, 0]),
                      plan_execute=seed % 3 == 0)


def test_empty_batches():
    dev = torch.device("cuda")
    wire = torch.zeros(64, dtype=torch.uint8, device=dev)
    pay = torch.zeros(64, dtype=torch.uint8, device=dev)
    d = torch.zeros((0, 32), dtype=torch.uint8, device=dev)
    assert int(cfws.serialize(pay, d, wire).item()) == 0
    idx = torch.zeros(0, dtype=torch.int64, device=dev)
    _, st, tot = cfws.deserialize(wire, 64, idx, pay)
    assert int(tot.item()) == 0 and st.numel() == 0
    e = torch.zeros(0, dtype=torch.int64, device=dev)
    starts, first, consumed, stop, total = cfws.index_frames_batch(wire, e, e)
    assert total == 0
    assert cfws.ws_accept_keys([]) == []


def test_error_codes():
    L = cfws.lib()
    dev = torch.device("cuda")
    s = torch.cuda.current_stream().cuda_stream
    pay = torch.zeros(4096, dtype=torch.uint8, device=dev)
    wire = torch.zeros(4096, dtype=torch.uint8, device=dev)
    desc = cfws.desc_to_device(np.zeros(4, dtype=cfws.DESC_DTYPE), dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = cfws.workspace(4, 4096, dev)
    # workspace too small
    assert L.cfws_serialize_batch(pay.data_ptr(), desc.data_ptr(), 4, wire.data_ptr(), 4096,
                                  tot.data_ptr(), ws.data_ptr(), 8, s) == cfws.ERROR_WORKSPACE
    # alignment must be a power of two <= 4096; flags must be known
    idx = torch.zeros(4, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    for align, flags in ((3, 0), (8192, 0), (16, 4)):
        rc = L.cfws_deserialize_batch(wire.data_ptr(), 4096, idx.data_ptr(), 4,
                                      O.DEFAULT_MAX_PAYLOAD, align, flags, desc.data_ptr(),
                                      st.data_ptr(), pay.data_ptr(), 4096, tot.data_ptr(),
                                      ws.data_ptr(), ws.numel(), s)
        assert rc == cfws.ERROR_INVALID_ARGUMENT, (align, flags)
    # execute on arenas that are not 16-byte aligned
    rc = L.cfws_serialize_execute(pay.data_ptr() + 1, desc.data_ptr(), 4, wire.data_ptr(), 4096,
                                  ws.data_ptr(), s)
    assert rc == cfws.ERROR_INVALID_ARGUMENT
    # HTTP/2 max_frame_size beyond 2^24 - 1
    h2 = torch.zeros(8192, dtype=torch.uint8, device=dev)
    wsh = torch.zeros(cfws.lib().cfws_h2_serialize_workspace_size(4, 4096, 8192, 1 << 24),
                      dtype=torch.uint8, device=dev)
    rc = L.cfws_h2_serialize_batch(pay.data_ptr(), desc.data_ptr(), 4, 1, 1 << 24, wire.data_ptr(),
                                   4096, h2.data_ptr(), 8192, tot.data_ptr(), wsh.data_ptr(),
                                   wsh.numel(), s)
    assert rc == cfws.ERROR_INVALID_ARGUMENT
    assert cfws.lib().cfws_last_error()


def _small_stream(seed, n):
    """n frames of 0-40 payload bytes: (wire, frame starts)."""
    wire, _ = wire_stream(random.Random(seed), n, sizes=list(range(41)))
    starts, _ = O.index_frames(wire, n + 1)
    assert len(starts) == n
    return wire, np.asarray(starts, dtype=np.uint64)


def test_error_codes_across_routes():
    """The argument checks of the batch entry points, whichever form the call
    would have taken: cfws_deserialize_batch at 4 frames (one small-batch
    launch), 1,100 frames of 0-40 B at align 16 (the fused plan + copy) and
    at align 1 (plan + execute), cfws_serialize_batch at 4 and 1,100 frames.
    One call per bad argument: the same code and cfws_last_error text on
    every route, nothing written by a call the plan stage rejects, and a
    valid call on the same buffers afterwards still equals the oracle."""
    L = cfws.lib()
    dev = torch.device("cuda")
    s = torch.cuda.current_stream().cuda_stream
    SENT = 0xA5
    WS, ARG = cfws.ERROR_WORKSPACE, cfws.ERROR_INVALID_ARGUMENT

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == SENT).all()) for t in ts)

    # ---- receive ----
    for n, align in ((4, 16), (1100, 16), (1100, 1)):
        wire, starts = _small_stream(100 + n + align, n)
        cap = len(wire) + 16 * n + 16
        e_out, e_d, e_st, e_tot = O.deserialize_batch(wire, starts, align=align, capacity=cap)
        w = torch.from_numpy(np.concatenate([wire, np.zeros(16, np.uint8)])).to(dev)
        idx = torch.from_numpy(starts.astype(np.int64)).to(dev)
        out = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
        d_t = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        st_t = torch.empty(n, dtype=torch.int32, device=dev)
        tot = torch.empty(1, dtype=torch.int64, device=dev)
        ws = cfws.workspace(n, cap, dev)
        good = dict(d_wire=w.data_ptr(), d_index=idx.data_ptr(), align=align, flags=0,
                    d_desc=d_t.data_ptr(), d_status=st_t.data_ptr(), d_payload=out.data_ptr(),
                    ws=ws.data_ptr(), ws_size=ws.numel())
        assert L.cfws_deserialize_pass_kernel(n, len(wire), align, 0, cap) == {
            (4, 16): b"deserialize_small_kernel", (1100, 16): b"deserialize_plan_single_kernel<true>",
            (1100, 1): b"xform_kernel<1>"}[(n, align)]

        def call(**bad):
            a = dict(good, **bad)
            for t in (d_t, st_t, tot, out):
                t.view(torch.uint8).fill_(SENT)
            return L.cfws_deserialize_batch(a["d_wire"], len(wire), a["d_index"], n,
                                            O.DEFAULT_MAX_PAYLOAD, a["align"], a["flags"], a["d_desc"],
                                            a["d_status"], a["d_payload"], cap, tot.data_ptr(), a["ws"],
                                            a["ws_size"], s)

        def valid():
            assert call() == cfws.OK
            torch.cuda.synchronize()
            assert int(tot.item()) == e_tot
            assert np.array_equal(st_t.cpu().numpy(), e_st)
            d = cfws.desc_from_device(d_t)
            for f in ("payload_off", "wire_off", "payload_size", "mask_key", "fin", "opcode", "mask",
                      "header_size"):
                assert np.array_equal(d[f], e_d[f]), (n, align, f)
            assert np.array_equal(out[:e_tot].cpu().numpy(), e_out[:e_tot]), (n, align)

        valid()
        plan_stage = (
            (dict(ws_size=8), WS, b"workspace too small"),
            (dict(ws=None), WS, b"workspace too small"),
            (dict(align=3), ARG, b"align must be a power of two <= 4096"),
            (dict(align=8192), ARG, b"align must be a power of two <= 4096"),
            (dict(flags=4), ARG, b"unknown flags"),
            (dict(d_desc=None), ARG, b"null pointer"),
            (dict(d_status=None), ARG, b"null pointer"),
            (dict(d_index=None), ARG, b"null pointer"),
            (dict(d_wire=None), ARG, b"null pointer"),
        )
        execute_stage = (
            (dict(d_payload=None), ARG, b"null pointer"),
            (dict(d_payload=out.data_ptr() + 1), ARG, b"arenas must be 16-byte aligned"),
        )
        for bad, code, text in plan_stage + execute_stage:
            assert call(**bad) == code, (n, align, bad)
            assert text in L.cfws_last_error(), (n, align, bad, L.cfws_last_error())
            if (bad, code, text) in plan_stage:
                assert untouched(d_t, st_t, tot), (n, align, bad)
            valid()

    # ---- send ----
    for n in (4, 1100):
        rng = random.Random(200 + n)
        payload = O.fill_splitmix(4096, n, 0)
        desc = random_desc(rng, n, payload.size, sizes=list(range(41)))
        exp, d_exp = O.serialize_batch(payload, desc.view(O.DESC_DTYPE))
        total = len(exp)
        cap = (total + 15) // 16 * 16
        desc["wire_off"] = 0xA5A5A5A5A5A5A5A5             # the plan's outputs, sentinel-filled
        desc["header_size"] = SENT
        d_in = cfws.desc_to_device(desc, dev)
        d_t = torch.empty_like(d_in)
        pay = torch.from_numpy(np.concatenate([payload, np.zeros(16, np.uint8)])).to(dev)
        out = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
        tot = torch.empty(1, dtype=torch.int64, device=dev)
        ws = cfws.workspace(n, cap, dev)
        good = dict(d_payload=pay.data_ptr(), d_desc=d_t.data_ptr(), ws=ws.data_ptr(), ws_size=ws.numel())

        def call(**bad):
            a = dict(good, **bad)
            d_t.copy_(d_in)
            for t in (tot, out):
                t.view(torch.uint8).fill_(SENT)
            return L.cfws_serialize_batch(a["d_payload"], a["d_desc"], n, out.data_ptr(), cap,
                                          tot.data_ptr(), a["ws"], a["ws_size"], s)

        def valid():
            assert call() == cfws.OK
            torch.cuda.synchronize()
            assert int(tot.item()) == total
            d = cfws.desc_from_device(d_t)
            assert np.array_equal(d["wire_off"], d_exp["wire_off"])
            assert np.array_equal(d["header_size"], d_exp["header_size"])
            assert np.array_equal(out[:total].cpu().numpy(), exp), n

        valid()
        plan_stage = (
            (dict(ws_size=8), WS, b"workspace too small"),
            (dict(ws=None), WS, b"workspace too small"),
            (dict(d_desc=None), ARG, b"null descriptor table"),
        )
        execute_stage = (
            (dict(d_payload=None), ARG, b"null pointer"),
            (dict(d_payload=pay.data_ptr() + 1), ARG, b"arenas must be 16-byte aligned"),
        )
        for bad, code, text in plan_stage + execute_stage:
            assert call(**bad) == code, (n, bad)
            assert text in L.cfws_last_error(), (n, bad, L.cfws_last_error())
            if (bad, code, text) in plan_stage:
                assert untouched(tot) and torch.equal(d_t, d_in), (n, bad)
            valid()
