"""The relay against the two-call path, in one process:
  (a) cfws_relay_batch;
  (b) cfws_deserialize_batch (16-byte slots) then cfws_serialize_batch over a
      send table prepared outside the timed loop (the most favourable form of
      (b): no descriptor fix-up between its two calls is timed).
After a warm-up, (a) and (b) alternate for --steps steps, each timed as a
whole call with a pair of events, one synchronise at the end; then (a)'s
streaming pass alone is timed through cfws_time_next_pass for --steps more
calls. Outside the timed loops 1,024 sampled outgoing frames of (a) are
compared with oracle.serialize_keyed over the oracle's unmasked payload.
One JSON line per shape: call and pass times in ms (median and minimum),
payload GiB/s (payload bytes over that time), the algorithmic bytes
n (2 fs + h_in + h_out) of the relay and n (4 fs + h_in + h_out) of the
pair, and the pass's share of 8 TB/s (algorithmic bytes over pass time).
Without a GPU the measured fields read "not measured".
  python3 tools/relay_bench.py [--steps 20] [--warmup 3] [--shape NAME ...]"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import oracle as O  # noqa: E402
from coldforce_amd import cfws  # noqa: E402

SHAPES = {  # name: (frames, payload bytes, out_mask); client-masked in
    "64k_unmasked_out": (65536, 65536, 0),
    "1k_unmasked_out": (4 << 20, 1024, 0),
    "64k_masked_out": (65536, 65536, 1),
}
PEAK = 8e12
SAMPLES = 1024


def header(fs, mask):
    return cfws.uniform_frame_bytes(fs, bool(mask)) - fs


def stats(ms):
    return round(statistics.median(ms), 4), round(min(ms), 4)


def measure(name, n, fs, out_mask, steps, warmup):
    h_in, h_out = header(fs, 1), header(fs, out_mask)
    w_in, w_out = fs + h_in, fs + h_out
    row = {"shape": name, "frames": n, "payload": fs, "in_mask": 1, "out_mask": out_mask, "steps": steps,
           "warmup": warmup, "relay_algorithmic_bytes": n * (2 * fs + h_in + h_out),
           "pair_algorithmic_bytes": n * (4 * fs + h_in + h_out)}
    if not torch.cuda.is_available():
        for k in ("relay_call_ms", "pair_call_ms", "relay_pass_ms", "relay_call_payload_GiBps",
                  "pair_call_payload_GiBps", "relay_pass_payload_GiBps", "relay_pass_frac_of_8TBps",
                  "relay_over_pair", "verified"):
            row[k] = "not measured"
        return row
    cfws.init()
    dev = "cuda"
    pay = torch.empty(n * fs + 16, dtype=torch.uint8, device=dev)
    cfws.fill_splitmix(pay, 0x5EED0012)
    keys_in = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=dev)
    keys_out = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=dev)
    wire = torch.empty(n * w_in + 16, dtype=torch.uint8, device=dev)
    cfws.serialize_uniform(pay, keys_in, n, fs, wire, opcode=cfws.OPCODE_BINARY, mask=True)
    idx = torch.arange(n, dtype=torch.int64, device=dev) * w_in
    out_a = torch.empty(n * w_out + 16, dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(out_a)
    # (a)'s tables
    a_desc = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    a_st = torch.empty(n, dtype=torch.int32, device=dev)
    a_ws = cfws.relay_workspace(n, out_a.numel(), dev)
    a_tot = torch.zeros(1, dtype=torch.int64, device=dev)
    # (b)'s tables; its payload arena is `pay` (the receive writes back the bytes it holds)
    b_desc = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    b_st = torch.empty(n, dtype=torch.int32, device=dev)
    b_ws = cfws.workspace(n, max(pay.numel(), out_b.numel()), dev)
    b_tot = torch.zeros(1, dtype=torch.int64, device=dev)

    def relay():
        cfws.relay(wire, n * w_in, idx, out_a, cfws.RELAY_VERBATIM, bool(out_mask), keys_out if out_mask else None,
                   a_desc, a_st, a_ws, a_tot)

    cfws.deserialize(wire, n * w_in, idx, pay, b_desc, b_st, b_ws, b_tot, align=16)
    send = b_desc.clone()                                      # the send table: mask byte, key
    send[:, 30] = out_mask
    if out_mask:
        send[:, 24:28] = keys_out.view(torch.uint8).view(n, 4)

    def pair():
        cfws.deserialize(wire, n * w_in, idx, pay, b_desc, b_st, b_ws, b_tot, align=16)
        cfws.serialize(pay, send, out_b, b_ws, b_tot)

    for _ in range(warmup):
        relay()
        pair()
    ev = [[cfws.TimingEvent() for _ in range(4)] for _ in range(steps)]
    for e in ev:
        e[0].record()
        relay()
        e[1].record()
        e[2].record()
        pair()
        e[3].record()
    torch.cuda.synchronize()
    a_ms = [e[0].elapsed_time(e[1]) for e in ev]
    b_ms = [e[2].elapsed_time(e[3]) for e in ev]
    pv = [[cfws.TimingEvent(), cfws.TimingEvent()] for _ in range(steps)]
    for p in pv:
        cfws.time_next_pass(p[0], p[1])
        relay()
    torch.cuda.synchronize()
    p_ms = [p[0].elapsed_time(p[1]) for p in pv]
    del ev, pv                                                 # HIP events freed while the runtime is up
    # verification: sampled frames of (a) against the oracle, (a) == (b) on the device
    ok = int(a_tot.item()) == n * w_out and bool((a_st == 0).all()) and torch.equal(out_a[:n * w_out],
                                                                                     out_b[:n * w_out])
    ko = keys_out.cpu().numpy().view(np.uint32)
    for i in np.random.RandomState(12).choice(n, min(SAMPLES, n), replace=False):
        i = int(i)
        frame_in = wire[i * w_in:(i + 1) * w_in].cpu().numpy()
        arena, d, st, _ = O.deserialize_batch(frame_in, np.zeros(1, np.uint64), align=1)
        exp = O.serialize_keyed(bool(d["fin"][0]), int(d["opcode"][0]), bool(out_mask), int(ko[i]) if out_mask else 0,
                                arena[:int(d["payload_size"][0])].tobytes())
        got = out_a[i * w_out:(i + 1) * w_out].cpu().numpy().tobytes()
        ok = ok and int(st[0]) == 0 and got == exp
    gib = n * fs / 2**30
    (a_med, a_min), (b_med, b_min), (p_med, p_min) = stats(a_ms), stats(b_ms), stats(p_ms)
    row.update({
        "relay_call_ms": a_med, "relay_call_ms_min": a_min, "pair_call_ms": b_med, "pair_call_ms_min": b_min,
        "relay_pass_ms": p_med, "relay_pass_ms_min": p_min,
        "relay_call_payload_GiBps": round(gib / (a_med / 1e3), 1),
        "pair_call_payload_GiBps": round(gib / (b_med / 1e3), 1),
        "relay_pass_payload_GiBps": round(gib / (p_med / 1e3), 1),
        "relay_pass_frac_of_8TBps": round(row["relay_algorithmic_bytes"] / (p_med / 1e3) / PEAK, 4),
        "relay_over_pair": round(a_med / b_med, 4),
        "receive_kernel": cfws.lib().cfws_deserialize_pass_kernel(n, n * w_in, 16, 0, pay.numel()).decode(),
        "verified": bool(ok)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", action="append", choices=sorted(SHAPES))
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("at least 20 steps")
    for name in a.shape or list(SHAPES):
        n, fs, out_mask = SHAPES[name]
        print(json.dumps(measure(name, n, fs, out_mask, a.steps, a.warmup)), flush=True)
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
