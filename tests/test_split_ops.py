"""The split ops of include/cfws.h -- cfws_encode_headers, cfws_parse_headers,
cfws_mask_batch, cfws_unmask_batch: the header and payload passes of
co_ws_frame.c (:34-91, :93-97, :131-213, :232-242) over caller-laid-out
frames.

CPU: the oracle's split restatements compose back to the oracle's serialize
/ deserialize (which the reference's own vectors pin, test_oracle.py).
GPU: the device ops equal the oracle byte for byte on packed and scattered
layouts, with gaps left untouched, capacity cuts, non-COMPLETE frames
skipped, and the config-2 batch at full size equal to the reference digest.
"""
import hashlib
import random

import numpy as np
import pytest

import oracle as O
from conftest import golden


def random_frames(rng, n, payload_len, sizes=None):
    d = np.zeros(n, dtype=O.DESC_DTYPE)
    for i in range(n):
        sz = min(rng.choice(sizes) if sizes else rng.randrange(0, 3000), payload_len)
        d[i]["payload_off"] = rng.randrange(0, payload_len - sz + 1)
        d[i]["payload_size"] = sz
        d[i]["fin"] = rng.random() < 0.7
        d[i]["opcode"] = rng.randrange(256) if rng.random() < 0.1 else rng.choice([0, 1, 2, 8, 9])
        d[i]["mask"] = rng.random() < 0.6
        d[i]["mask_key"] = rng.getrandbits(32) if d[i]["mask"] else 0
    return d


def scattered_wire_offsets(rng, desc, max_gap=40):
    """Frames placed in order with random gaps (any alignment): no overlap."""
    off = rng.randrange(0, 16)
    out = np.zeros(len(desc), dtype=np.uint64)
    for i, d in enumerate(desc):
        out[i] = off
        off += O.header_size(int(d["payload_size"]), bool(d["mask"])) + int(d["payload_size"])
        off += rng.randrange(0, max_gap)
    return out, off


# ---- CPU: the oracle's split ops against its pinned serialize / deserialize ----

@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_split_composes_to_serialize(seed):
    rng = random.Random(seed)
    payload = O.fill_splitmix(200000, 0x5EED + seed)
    desc = random_frames(rng, 300, len(payload), sizes=[0, 1, 125, 126, 127, 4096, 65535,
                                                         65536, 65537, rng.randrange(70000)])
    wire, d_exp = O.serialize_batch(payload, desc)
    d = desc.copy()
    d["wire_off"] = d_exp["wire_off"]
    w2 = np.zeros(len(wire), np.uint8)
    d2 = O.encode_headers(d, w2)
    O.mask_batch(payload, d2, w2)
    assert np.array_equal(w2, wire)
    assert np.array_equal(d2["header_size"], d_exp["header_size"])
    pd, st = O.parse_headers(wire, d_exp["wire_off"])
    _, dd, st_d, _ = O.deserialize_batch(wire, d_exp["wire_off"], align=1)
    assert np.array_equal(st, st_d)          # opcode bytes > 0x0f (RSV bits) -> -7001
    for f in ("payload_size", "mask_key", "fin", "opcode", "mask", "header_size"):
        assert np.array_equal(pd[f], dd[f]), f
    ok = st == 0
    # (fin / opcode: b0 = opcode | fin << 7 verbatim, so opcode bit 7 reads back as fin)
    for f in ("payload_size", "mask_key", "mask", "header_size"):
        assert np.array_equal(pd[f][ok], d_exp[f][ok]), f
    out = np.zeros(len(payload), np.uint8)
    pd["payload_off"] = desc["payload_off"]
    O.unmask_batch(wire, pd, st, out)
    for d0, good in zip(desc, ok):
        a, n = int(d0["payload_off"]), int(d0["payload_size"])
        if good:
            assert np.array_equal(out[a:a + n], payload[a:a + n])


def test_oracle_parse_headers_golden():
    for c in golden("deserialize_cases.json"):
        if c["wire_hex"] is None:
            continue
        raw = np.frombuffer(bytes.fromhex(c["wire_hex"]), dtype=np.uint8).copy()
        d, st = O.parse_headers(raw, np.array([c["index"]], np.uint64), c["max_payload"])
        exp = O.PARSE_MORE_DATA if len(raw) - c["index"] < 2 else c["rc"]
        assert st[0] == exp, c["name"]
        if exp == 0:
            assert int(d["payload_size"][0]) == c["payload_size"]


# ---- GPU -------------------------------------------------------------------

def _torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    torch = _torch()
    from coldforce_amd import cfws
    cfws.init()
    return torch.device("cuda", 0)


def gpu_encode_mask(payload, desc, wire_len, fill=0xA5, capacity=None, max_payload=None,
                    headers=True, packed=False):
    torch = _torch()
    from coldforce_amd import cfws
    pay = torch.from_numpy(payload).cuda()
    d_t = cfws.desc_to_device(desc.view(cfws.DESC_DTYPE))
    wire = torch.full((wire_len,), fill, dtype=torch.uint8, device="cuda")
    cap = wire_len if capacity is None else capacity
    if headers:
        cfws.encode_headers(d_t, wire, cap)
    mp = int(desc["payload_size"].max()) if max_payload is None else max_payload
    cfws.mask_batch(pay, d_t, wire, mp, cap, packed=packed)
    torch.cuda.synchronize()
    return wire.cpu().numpy(), cfws.desc_from_device(d_t)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 4, 5])
def test_encode_mask_scattered(dev, seed):
    rng = random.Random(seed)
    payload = O.fill_splitmix(300000, seed)
    desc = random_frames(rng, 500, len(payload), sizes=[0, 1, 2, 3, 15, 16, 17, 125, 126, 1000,
                                                         4096, 65535, 65536, 70000])
    desc["wire_off"], total = scattered_wire_offsets(rng, desc)
    wlen = total + 64
    got, d_got = gpu_encode_mask(payload, desc, wlen)
    exp = np.full(wlen, 0xA5, np.uint8)
    d_exp = O.encode_headers(desc, exp)
    O.mask_batch(payload, d_exp, exp)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
    assert np.array_equal(d_got["header_size"], d_exp["header_size"])


@pytest.mark.gpu
def test_encode_mask_packed_equals_serialize(dev):
    rng = random.Random(11)
    payload = O.fill_splitmix(1 << 20, 11)
    desc = random_frames(rng, 2000, len(payload))
    wire, d_exp = O.serialize_batch(payload, desc)
    d = desc.copy()
    d["wire_off"] = d_exp["wire_off"]
    got, _ = gpu_encode_mask(payload, d, len(wire) + 16)
    assert np.array_equal(got[:len(wire)], wire)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [12, 13])
def test_mask_packed(dev, seed):
    """cfws_mask_batch_packed: frames packed back to back (the serialize
    layout) of every size class -- 0-15-byte payloads whose boundaries fall
    back to byte stores, 16-31, 1 KiB, 64 KiB, 16- and 64-bit lengths,
    masked and unmasked -- give the serialize wire exactly, as do capacity
    cuts inside a boundary chunk and inside a payload; a batch with gaps
    (not packed) equals cfws_mask_batch's bytes, gaps untouched."""
    rng = random.Random(seed)
    payload = O.fill_splitmix(1 << 21, seed)
    desc = random_frames(rng, 3000, len(payload), sizes=[0, 1, 5, 15, 16, 17, 31, 32, 100, 125, 126,
                                                          1000, 1024, 4095, 65535, 65536, 70000])
    wire, d_exp = O.serialize_batch(payload, desc)
    d = desc.copy()
    d["wire_off"] = d_exp["wire_off"]
    got, _ = gpu_encode_mask(payload, d, len(wire) + 16, packed=True)
    bad = np.nonzero(got[:len(wire)] != wire)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:8]}"
    assert (got[len(wire):] == 0xA5).all()
    for cap in (len(wire) // 2 + 7, len(wire) // 3 // 16 * 16, int(d["wire_off"][1500]) + 5):
        got, _ = gpu_encode_mask(payload, d, len(wire) + 16, capacity=cap, packed=True)
        exp = np.full(len(wire) + 16, 0xA5, np.uint8)
        O.mask_batch(payload, O.encode_headers(d, exp, cap), exp, cap)
        assert np.array_equal(got, exp), cap
    d["wire_off"], total = scattered_wire_offsets(rng, desc)
    got, _ = gpu_encode_mask(payload, d, total + 64, packed=True)
    exp = np.full(total + 64, 0xA5, np.uint8)
    O.mask_batch(payload, O.encode_headers(d, exp), exp)
    assert np.array_equal(got, exp)


# header size -> (smallest payload of the class, masked); a frame of the class
# has one of the 16 sizes from the smallest on
HEADER_CLASSES = {2: (16, False), 6: (16, True), 4: (126, False), 8: (126, True),
                  10: (65536, False), 14: (65536, True)}


def packed_inrun(d, g, cap):
    """cfws_mask_batch_packed's rule (include/cfws.h, cfws_split.hip): frame
    g's boundary chunks are written in its first run."""
    if g == 0:
        return False
    a, b = d[g - 1], d[g]
    a_size, b_size = int(a["payload_size"]), int(b["payload_size"])
    a_end = int(a["wire_off"]) + O.header_size(a_size, bool(a["mask"])) + a_size
    b_dof = int(b["wire_off"]) + O.header_size(b_size, bool(b["mask"]))
    return (a_end == int(b["wire_off"]) and a_size >= 16 and b_size >= 16
            and (b_dof + 15) // 16 * 16 <= cap)


def boundary_class(d, g):
    """(hs_g, t, tph): g's header size, where its header starts in its
    16-byte chunk, and where g - 1's last t payload bytes start in theirs."""
    hs = O.header_size(int(d[g]["payload_size"]), bool(d[g]["mask"]))
    t = int(d[g]["wire_off"]) % 16
    tph = (int(d[g - 1]["payload_off"]) + int(d[g - 1]["payload_size"]) - t) % 16
    return hs, t, tph


def boundary_class_chain(rng, payload_len):
    """One packed chain that meets every boundary class: a frame's size (16
    sizes per header class) steers where the next header starts, its
    payload_off (sources may overlap) where its own tail starts. The 64-bit
    classes appear once per header start; then frames that must not take the
    in-run form. Returns (desc, wire length, indices of those frames)."""
    small = [2, 4, 6, 8]
    targets = []                                    # (hs, t, tph) of frames 1, 2, ...
    for t in range(16):
        hs_of = [10, 14] + [small[(k + t) % 4] for k in range(14)]
        targets += [(hs_of[(tph + t) % 16], t, tph) for tph in range(16)]
    for t in range(16):                             # again on both sides of tph + t = 16
        targets += [(small[(t + k) % 4], t, (16 - t + k) % 16) for k in range(-4, 5)]
    rng.shuffle(targets)
    n = 1 + len(targets)
    d = np.zeros(n + 5, dtype=O.DESC_DTYPE)
    off = 5                                         # frame 0: never in-run
    plan = [(2, off % 16, 0)] + targets
    for g in range(n):
        hs, t, _ = plan[g]
        lo, masked = HEADER_CLASSES[hs]
        _, t_next, tph_next = plan[g + 1] if g + 1 < n else (0, rng.randrange(16), rng.randrange(16))
        size = lo + (t_next - t - hs - lo) % 16
        res = (tph_next + t_next - size) % 16
        d[g]["payload_size"] = size
        d[g]["payload_off"] = 16 * rng.randrange((payload_len - size - 16) // 16) + res
        d[g]["mask"] = masked
        d[g]["wire_off"] = off
        assert off % 16 == t and O.header_size(size, masked) == hs
        off += hs + size
    # own payload 15; predecessor's payload 15; a packed frame; a 1-byte gap
    # before a header; a packed frame
    not_inrun = [0, n, n + 1, n + 3]
    for g, (size, gap) in enumerate([(15, 0), (20, 0), (20, 0), (20, 1), (20, 0)], start=n):
        masked = bool(g & 1)
        d[g]["payload_size"] = size
        d[g]["payload_off"] = rng.randrange(payload_len - size)
        d[g]["mask"] = masked
        d[g]["wire_off"] = off + gap
        off += gap + O.header_size(size, masked) + size
    for g in range(len(d)):
        d[g]["fin"] = rng.random() < 0.7
        d[g]["opcode"] = rng.choice([0, 1, 2, 8, 9])
        d[g]["mask_key"] = rng.getrandbits(32) if d[g]["mask"] else 0
    return d, off, not_inrun


@pytest.mark.gpu
def test_mask_packed_boundary_classes(dev):
    """cfws_mask_batch_packed over every boundary class (hs_g, t, tph) of an
    in-run frame: all 96 (header size, header start in its chunk) pairs and
    all 256 (header start, start of the predecessor's tail in its source
    block) pairs, which has both sides of tph + t > 16 (one source block or
    two). Frames that must not take the in-run form sit in the same chain:
    frame 0, a 15-byte payload and its successor, a header after a 1-byte
    gap; and a second call cuts the capacity inside a boundary chunk.
    Expected bytes: the oracle's encode_headers + mask_batch; bytes outside
    the frames keep the fill."""
    rng = random.Random(61)
    payload = O.fill_splitmix(1 << 17, 61)
    d, total, not_inrun = boundary_class_chain(rng, len(payload))
    wlen = total + 21
    inrun = [g for g in range(len(d)) if packed_inrun(d, g, wlen)]
    classes = {boundary_class(d, g) for g in inrun}
    assert {(hs, t) for hs, t, _ in classes} == {(hs, t) for hs in HEADER_CLASSES for t in range(16)}
    assert {(t, tph) for _, t, tph in classes} == {(t, tph) for t in range(16) for tph in range(16)}
    assert len(inrun) == len(d) - len(not_inrun) and not set(inrun) & set(not_inrun)
    assert sum(int(x["payload_size"]) >= 65536 for x in d) == 32
    # a capacity that ends inside an in-run frame's boundary chunk
    k = next(g for g in inrun[len(inrun) // 2:]
             if 1 <= (int(d[g]["wire_off"]) + boundary_class(d, g)[0]) % 16 <= 13)
    cut = int(d[k]["wire_off"]) + boundary_class(d, k)[0] + 1
    assert not packed_inrun(d, k, cut) and packed_inrun(d, k - 1, cut)
    for cap in (wlen, cut):
        got, _ = gpu_encode_mask(payload, d, wlen, capacity=cap, packed=True)
        exp = np.full(wlen, 0xA5, np.uint8)
        O.mask_batch(payload, O.encode_headers(d, exp, cap), exp, cap)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"cap {cap}: {bad.size} bytes differ, first at {bad[:8]}"


@pytest.mark.gpu
@pytest.mark.parametrize("max_payload", [0, 1000, 1 << 20])
def test_mask_grid_hint(dev, max_payload):
    # the max_payload_size hint only sizes the grid: any value gives the same bytes
    rng = random.Random(21)
    payload = O.fill_splitmix(3 << 20, 21)
    desc = random_frames(rng, 40, len(payload), sizes=[70000, 1 << 20, (2 << 20) + 5, 3])
    desc["wire_off"], total = scattered_wire_offsets(rng, desc)
    got, _ = gpu_encode_mask(payload, desc, total + 32, max_payload=max_payload)
    exp = np.full(total + 32, 0xA5, np.uint8)
    O.mask_batch(payload, O.encode_headers(desc, exp), exp)
    assert np.array_equal(got, exp)


@pytest.mark.gpu
def test_mask_capacity_cut(dev):
    rng = random.Random(31)
    payload = O.fill_splitmix(100000, 31)
    desc = random_frames(rng, 60, len(payload))
    desc["wire_off"], total = scattered_wire_offsets(rng, desc)
    for cap in (0, 1, 17, total // 3 + 5, total - 1):
        got, _ = gpu_encode_mask(payload, desc, total + 16, capacity=cap)
        exp = np.full(total + 16, 0xA5, np.uint8)
        O.mask_batch(payload, O.encode_headers(desc, exp, cap), exp, cap)
        assert np.array_equal(got, exp), cap


@pytest.mark.gpu
def test_parse_headers_matches_oracle(dev):
    torch = _torch()
    from coldforce_amd import cfws
    rng = random.Random(41)
    payload = O.fill_splitmix(400000, 41)
    desc = random_frames(rng, 700, len(payload), sizes=[0, 1, 125, 126, 127, 65535, 65536, 70000])
    wire, d_exp = O.serialize_batch(payload, desc)
    wire = wire.copy()
    starts = d_exp["wire_off"].astype(np.uint64)
    for i in rng.sample(range(len(desc)), 20):
        wire[int(starts[i])] |= 0x20                       # RSV3 -> INVALID_FRAME
    extra = np.array([len(wire) - 1, len(wire), len(wire) + 9, int(starts[7]) + 1], np.uint64)
    starts = np.concatenate([starts, extra])
    for max_payload in (O.DEFAULT_MAX_PAYLOAD, 1000):
        for size in (len(wire), len(wire) - 70001):
            w_t = torch.from_numpy(wire).cuda()
            i_t = torch.from_numpy(starts.astype(np.int64)).cuda()
            d_t = torch.empty((len(starts), 32), dtype=torch.uint8, device="cuda")
            s_t = torch.empty(len(starts), dtype=torch.int32, device="cuda")
            cfws.parse_headers(w_t, size, i_t, d_t, s_t, max_payload)
            torch.cuda.synchronize()
            d_got, st_got = cfws.desc_from_device(d_t), s_t.cpu().numpy()
            d_o, st_o = O.parse_headers(wire, starts, max_payload, wire_size=size)
            assert np.array_equal(st_got, st_o)
            for f in ("wire_off", "payload_size", "mask_key", "fin", "opcode", "mask",
                      "header_size"):
                assert np.array_equal(d_got[f], d_o[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [51, 52])
def test_unmask_scattered(dev, seed):
    torch = _torch()
    from coldforce_amd import cfws
    rng = random.Random(seed)
    payload = O.fill_splitmix(300000, seed)
    desc = random_frames(rng, 600, len(payload), sizes=[0, 1, 5, 16, 33, 125, 126, 4097, 65536,
                                                         70000])
    wire, d_exp = O.serialize_batch(payload, desc)
    pd, st = O.parse_headers(wire, d_exp["wire_off"])
    # payloads to scattered destinations, any alignment, with gaps
    off = rng.randrange(16)
    for i in range(len(pd)):
        pd[i]["payload_off"] = off
        off += int(pd[i]["payload_size"]) + rng.randrange(0, 24)
    st = st.copy()
    for i in rng.sample(range(len(st)), 40):
        st[i] = rng.choice([O.PARSE_MORE_DATA, O.ERROR_INVALID_FRAME, O.ERROR_DATA_TOO_BIG])
    plen = off + 32
    for cap in (plen, plen // 2 + 3):
        w_t = torch.from_numpy(wire).cuda()
        d_t = cfws.desc_to_device(pd.view(cfws.DESC_DTYPE))
        s_t = torch.from_numpy(st).cuda()
        out_t = torch.full((plen,), 0x5C, dtype=torch.uint8, device="cuda")
        cfws.unmask_batch(w_t, d_t, s_t, out_t, int(pd["payload_size"].max()), cap)
        torch.cuda.synchronize()
        exp = np.full(plen, 0x5C, np.uint8)
        O.unmask_batch(wire, pd, st, exp, cap)
        got = out_t.cpu().numpy()
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, f"cap {cap}: {bad.size} bytes differ, first at {bad[:8]}"


@pytest.mark.gpu
def test_split_config2_full_size_digest(dev):
    """65,536 x 64 KiB through encode_headers + mask_batch: the same wire as
    the reference's serialize (tests/golden/batch_digests.json), and
    parse_headers + unmask_batch restore every payload byte."""
    torch = _torch()
    from coldforce_amd import cfws
    from coldforce_amd import workloads as W
    g = golden("batch_digests.json")[2]
    n, fs = g["n_frames"], g["frame_size"]
    desc = W.uniform_batch(n, fs, g["key_seed"])
    offs, total = W.wire_layout(desc)
    desc["wire_off"] = offs
    payload = torch.empty(n * fs, dtype=torch.uint8, device="cuda")
    cfws.fill_splitmix(payload, g["payload_seed"])
    d_t = cfws.desc_to_device(desc)
    wire = torch.empty(W.round16(total), dtype=torch.uint8, device="cuda")
    cfws.encode_headers(d_t, wire)
    cfws.mask_batch(payload, d_t, wire, fs)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    step = 1 << 28
    for o in range(0, total, step):
        h.update(wire[o:min(total, o + step)].cpu().numpy().tobytes())
    assert h.hexdigest() == g["wire_sha256"]
    idx = torch.from_numpy(offs.astype(np.int64)).cuda()
    pd_t = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    st_t = torch.empty(n, dtype=torch.int32, device="cuda")
    cfws.parse_headers(wire, total, idx, pd_t, st_t)
    pd = cfws.desc_from_device(pd_t)
    assert (st_t == 0).all().item()
    pd["payload_off"] = np.arange(n, dtype=np.uint64) * fs
    back = torch.empty(n * fs, dtype=torch.uint8, device="cuda")
    cfws.unmask_batch(wire, cfws.desc_to_device(pd), st_t, back, fs)
    torch.cuda.synchronize()
    assert torch.equal(back, payload)
