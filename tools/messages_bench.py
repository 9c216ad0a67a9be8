"""Message and control tables of received frames, in one
process, per shape:
  device  cfws_messages_batch over device-resident descriptors and statuses;
  host    what a caller without it does: copy d_desc + d_status to pinned host
          memory (timed between events), then cfws_messages_from_frames from
          native threads, one call per connection, on 1 and on 16 threads
          (tools/messages_host_walk.cpp; median of 5);
  floor   cfws_device_copy of the bytes the call must move (36 B per frame in,
          32 B per message out): the library's copy-kernel rate.
Shapes:
  16m_single  16,777,216 single-frame messages, 16,384 connections of 1,024;
  config3     config 3's batch (Zipf messages of 1-8 fragments, 4 GiB of
              payload), one connection.
Device calls: --warmup calls, then --steps calls each timed as a whole call
between two events, one synchronise at the end; medians. The device table is
compared with the host form's, byte for byte, once per shape. One JSON line
per shape; --out appends them to a file. Without a GPU the device fields read
"not measured".
  python3 tools/messages_bench.py [--steps 20] [--warmup 3] [--out FILE] [--shapes a,b]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coldforce_amd import cfws  # noqa: E402
from coldforce_amd import workloads as W  # noqa: E402


def shape_16m_single():
    n, conns = 1 << 24, 16384
    d = np.zeros(n, dtype=cfws.DESC_DTYPE)
    d["payload_size"] = 1024
    d["payload_off"] = np.arange(n, dtype=np.uint64) * np.uint64(1024)
    d["fin"], d["opcode"], d["mask"], d["header_size"] = 1, 2, 1, 8
    return d, np.zeros(n, np.int32), np.arange(conns, dtype=np.uint64) * np.uint64(n // conns)


def shape_config3():
    c3 = W.CONFIG3
    d, _ = W.zipf_batch(c3["target_bytes"], c3["seed"], c3["key_seed"])
    return d, np.zeros(len(d), np.int32), np.zeros(1, np.uint64)


SHAPES = {"16m_single": shape_16m_single, "config3": shape_config3}


def median_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev = [[cfws.TimingEvent(), cfws.TimingEvent()] for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    del ev
    return statistics.median(ms) * 1e3, min(ms) * 1e3


def host_walk(d, st, cf, threads, reps=5):
    so = os.path.join(ROOT, "build", "libmsghostwalk.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", ROOT, "build/libmsghostwalk.so"], check=True)
    H = C.CDLL(so)
    H.messages_host_walk.restype = C.c_uint64
    H.messages_host_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                     C.POINTER(C.c_uint64)]
    m = C.c_uint64()
    ns = [H.messages_host_walk(d.ctypes.data, st.ctypes.data, len(d), cf.ctypes.data, len(cf), threads, C.byref(m))
          for _ in range(reps)]
    return statistics.median(ns) / 1e3, m.value


def measure(name, steps, warmup):
    d, st, cf = SHAPES[name]()
    n = len(d)
    row = {"shape": name, "frames": n, "conns": len(cf), "steps": steps, "warmup": warmup}
    for threads in (1, 16):
        us, m = host_walk(d, st, cf, threads)
        row[f"host_walk_{threads}t_us"] = round(us, 1)
    row["messages"] = int(m)
    row["min_bytes"] = 36 * n + 32 * int(m)
    dev_fields = ("device_us", "device_us_min", "device_Gframes_s", "d2h_us", "host_total_16t_us",
                  "device_over_host_16t", "copy_floor_us", "device_over_copy_floor", "workspace_bytes", "verified")
    if not torch.cuda.is_available():
        row.update({f: "not measured" for f in dev_fields})
        return row
    cfws.init()
    dev = "cuda"
    desc_t = cfws.desc_to_device(d)
    st_t = torch.from_numpy(st).to(dev)
    cf_t = torch.from_numpy(cf.view(np.int64).copy()).to(dev)
    msgs_t = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    control_t = torch.empty(n, dtype=torch.int32, device=dev)
    cfm_t = torch.empty(len(cf), dtype=torch.int64, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = cfws.messages_workspace(n, len(cf), dev)
    row["workspace_bytes"] = ws.numel()
    L = cfws.lib()
    s = torch.cuda.current_stream().cuda_stream

    def call():
        rc = L.cfws_messages_batch(desc_t.data_ptr(), st_t.data_ptr(), n, cf_t.data_ptr(), len(cf), msgs_t.data_ptr(),
                                   n, cfm_t.data_ptr(), totals.data_ptr(), control_t.data_ptr(), n,
                                   totals.data_ptr() + 8, ws.data_ptr(), ws.numel(), s)
        assert rc == 0, L.cfws_last_error()

    med, lo = median_us(call, steps, warmup)
    row["device_us"], row["device_us_min"] = round(med, 1), round(lo, 1)
    row["device_Gframes_s"] = round(n / med / 1e3, 4)
    # the device table against the host form's
    hm, hcfm, hc, m, nc = cfws.messages_from_frames(d, st, cf)
    ok = totals.tolist() == [m, nc] and cfws.messages_from_device(msgs_t[:m]).tobytes() == hm.tobytes() and \
        np.array_equal(cfm_t.cpu().numpy().view(np.uint64), hcfm)
    row["verified"] = bool(ok)
    del hm, hc

    # today's alternative: D2H of descriptors and statuses into pinned memory, then the host walk
    h_desc = torch.empty((n, 32), dtype=torch.uint8, pin_memory=True)
    h_st = torch.empty(n, dtype=torch.int32, pin_memory=True)

    def d2h():
        h_desc.copy_(desc_t, non_blocking=True)
        h_st.copy_(st_t, non_blocking=True)

    d2h_us, _ = median_us(d2h, max(steps // 4, 5), 2)
    row["d2h_us"] = round(d2h_us, 1)
    row["host_total_16t_us"] = round(d2h_us + row["host_walk_16t_us"], 1)
    row["device_over_host_16t"] = round(med / row["host_total_16t_us"], 4)
    del h_desc, h_st

    # the bytes the call must move, at the library's copy-kernel rate
    nbytes = (row["min_bytes"] // 2 + 15) // 16 * 16            # a copy reads and writes each byte
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    floor_us, _ = median_us(lambda: cfws.device_copy(src, dst, nbytes), steps, warmup)
    row["copy_floor_us"] = round(floor_us, 1)
    row["device_over_copy_floor"] = round(med / floor_us, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("at least 20 steps")
    for name in a.shapes.split(","):
        line = json.dumps(measure(name, a.steps, a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
