"""The device key draw against the host draw it replaces,
in one process on one device. Per shape (frames, with or without mask flags
of density 0.6):
  device   cfws_draw_mask_keys_device between two events on the stream;
  host     cfws_draw_mask_keys_seeded of the same batch, wall time of the
           calling thread (the only way to these keys before the device
           form);
  upload   the host's keys, 4 bytes a frame, from pinned memory to the
           device between two events.
--warmup untimed and --steps timed repetitions of each, the three
interleaved step by step. Outside the timed loops the device's keys and next
position are compared with the host's. One JSON line per shape: median,
minimum and maximum of each in ms, and host + upload over device (medians).
Without a GPU the measured fields read "not measured".
  python3 tools/keys_bench.py [--steps 20] [--warmup 3] [--shape NAME ...]"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from coldforce_amd import cfws  # noqa: E402

SHAPES = {  # name: (frames, flag density or None)
    "16m": (16 << 20, None),
    "16m_flags": (16 << 20, 0.6),
    "4m": (4 << 20, None),
    "4m_flags": (4 << 20, 0.6),
}
SEED = 1234
FIRST = 1000003


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def measure(name, n, density, steps, warmup):
    row = {"shape": name, "frames": n, "flag_density": density, "steps": steps, "warmup": warmup,
           "key_bytes": 4 * n, "draws": None}
    flags = None if density is None else (np.random.default_rng(n).random(n) < density).astype(np.uint8)
    row["draws"] = 4 * (n if flags is None else int(flags.sum()))
    if not torch.cuda.is_available():
        for k in ("device_ms", "host_ms", "upload_ms", "host_plus_upload_over_device", "verified"):
            row[k] = "not measured"
        return row
    cfws.init()
    dev = "cuda"
    flags_t = None if flags is None else torch.from_numpy(flags).to(dev)
    keys_t = torch.empty(n, dtype=torch.int32, device=dev)
    up_t = torch.empty(n, dtype=torch.int32, device=dev)
    nxt_t = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_t = None if flags is None else torch.empty(cfws.draw_keys_workspace_size(n), dtype=torch.uint8, device=dev)
    host = torch.empty(n, dtype=torch.int32).pin_memory()
    host_np = host.numpy().view(np.uint32)
    fp = None if flags is None else flags.ctypes.data

    def device():
        cfws.draw_mask_keys_device(n, flags_t, SEED, FIRST, keys_t, nxt_t, ws_t)

    def host_draw():
        # the parent's form draws from the stream's start: the same work per key
        t0 = time.perf_counter()
        cfws._check(cfws.lib().cfws_draw_mask_keys_seeded(SEED, n, fp, host_np.ctypes.data), "seeded")
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        device()
        host_draw()
        up_t.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    ev = [[cfws.TimingEvent() for _ in range(4)] for _ in range(steps)]
    host_ms = []
    for e in ev:
        e[0].record()
        device()
        e[1].record()
        host_ms.append(host_draw())
        e[2].record()
        up_t.copy_(host, non_blocking=True)
        e[3].record()
        torch.cuda.synchronize()
    dev_ms = [e[0].elapsed_time(e[1]) for e in ev]
    up_ms = [e[2].elapsed_time(e[3]) for e in ev]
    del ev                                                     # HIP events freed while the runtime is up
    want, want_next = cfws.draw_mask_keys_at(n, flags, SEED, FIRST)
    ok = bool(np.array_equal(keys_t.cpu().numpy().view(np.uint32), want)) and int(nxt_t.item()) == want_next
    ok = ok and bool(np.array_equal(up_t.cpu().numpy().view(np.uint32), cfws.draw_mask_keys(n, flags, seed=SEED)))
    d, h, u = stats(dev_ms), stats(host_ms), stats(up_ms)
    row.update({"device_ms": d, "host_ms": h, "upload_ms": u,
                "host_plus_upload_over_device": round((h["median"] + u["median"]) / d["median"], 1),
                "device_keys_GBps": round(4 * n / (d["median"] / 1e3) / 1e9, 1), "verified": ok})
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
        n, density = SHAPES[name]
        print(json.dumps(measure(name, n, density, a.steps, a.warmup)), flush=True)
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
