"""HTTP/2 DATA frames of many streams, by message, in one
process, per shape:
  device  cfws_h2_streams_batch over device-resident records;
  host    what a caller without it does: copy d_starts, d_info and d_first to
          pinned host memory (timed between events), then
          cfws_h2_streams_from_frames from native threads, one call per
          connection, on 1 and on 16 threads (tools/h2_streams_host_walk.cpp;
          median of 5);
  floor   cfws_device_copy of the bytes the call must move (24 B per record in,
          12 B per frame and 32 B per message out): the library's copy-kernel
          rate.
Shapes:
  16k_x62   16,384 connections of 62 DATA records over 4 interleaved streams;
  16k_x3    16,384 connections of 3 records on one stream;
  one_x1m   the adversarial shape: one connection of 2^20 records, each its
            own stream (descending ids).
Device calls: --warmup calls, then --steps calls each timed as a whole call
between two events, one synchronise at the end; medians. The device tables are
compared with the host form's, byte for byte, once per shape. One JSON line
per shape; --out appends them to a file. Without a GPU the device fields read
"not measured".
  python3 tools/h2_streams_bench.py [--steps 20] [--warmup 3] [--out FILE] [--shapes a,b]"""
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


def records(sid, flags, length, conns):
    n = len(sid)
    info = np.zeros(n, cfws.H2_INFO_DTYPE)
    info["stream_id"], info["flags"], info["length"], info["advance"] = sid, flags, length, 9 + length
    starts = np.arange(n, dtype=np.uint64) * np.uint64(9 + length)
    return starts, info, np.arange(conns, dtype=np.uint64) * np.uint64(n // conns)


def shape_16k_x62():
    conns, per = 16384, 62
    rng = np.random.default_rng(62)
    sid = 1 + 2 * rng.integers(0, 4, conns * per)
    flags = (rng.random(conns * per) < 0.25).astype(np.uint8)
    return records(sid, flags, 1041, conns)


def shape_16k_x3():
    conns, per = 16384, 3
    flags = np.tile(np.array([0, 0, 1], np.uint8), conns)
    return records(np.ones(conns * per, np.uint32), flags, 16384, conns)


def shape_one_x1m():
    n = 1 << 20
    return records(np.arange(n, 0, -1, dtype=np.uint32), np.ones(n, np.uint8), 16, 1)


SHAPES = {"16k_x62": shape_16k_x62, "16k_x3": shape_16k_x3, "one_x1m": shape_one_x1m}


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


def host_walk(starts, info, cf, threads, reps=5):
    so = os.path.join(ROOT, "build", "libh2streamshostwalk.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", ROOT, "build/libh2streamshostwalk.so"], check=True)
    H = C.CDLL(so)
    H.h2_streams_host_walk.restype = C.c_uint64
    H.h2_streams_host_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.POINTER(C.c_uint64)]
    m = C.c_uint64()
    ns = [H.h2_streams_host_walk(starts.ctypes.data, info.ctypes.data, len(info), cf.ctypes.data, len(cf), threads,
                                 C.byref(m)) for _ in range(reps)]
    return statistics.median(ns) / 1e3, m.value


def measure(name, steps, warmup):
    starts, info, cf = SHAPES[name]()
    n = len(info)
    row = {"shape": name, "records": n, "conns": len(cf), "steps": steps, "warmup": warmup}
    for threads in (1, 16):
        us, m = host_walk(starts, info, cf, threads)
        row[f"host_walk_{threads}t_us"] = round(us, 1)
    host = cfws.h2_streams_from_frames(starts, info, cf)
    counts = host[5]
    row["counts"] = counts
    row["min_bytes"] = 24 * n + 12 * (counts[1] + counts[3]) + 32 * (counts[0] + counts[2])
    dev_fields = ("device_us", "device_us_min", "device_Grecords_s", "d2h_us", "host_total_16t_us",
                  "device_over_host_16t", "copy_floor_us", "device_over_copy_floor", "workspace_bytes", "verified")
    if not torch.cuda.is_available():
        row.update({f: "not measured" for f in dev_fields})
        return row
    cfws.init()
    dev = "cuda"
    starts_t = torch.from_numpy(starts.view(np.int64).copy()).to(dev)
    info_t = torch.from_numpy(info.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    cf_t = torch.from_numpy(cf.view(np.int64).copy()).to(dev)
    order_t = torch.empty(n, dtype=torch.int64, device=dev)
    of_t = torch.empty(n, dtype=torch.int32, device=dev)
    msgs_t = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    cfm_t = torch.empty(len(cf), dtype=torch.int64, device=dev)
    sf_t = torch.empty(n, dtype=torch.int64, device=dev)
    counts_t = torch.zeros(5, dtype=torch.int64, device=dev)
    ws = cfws.h2_streams_workspace(n, len(cf), dev)
    row["workspace_bytes"] = ws.numel()
    L = cfws.lib()
    s = torch.cuda.current_stream().cuda_stream

    def call():
        rc = L.cfws_h2_streams_batch(starts_t.data_ptr(), info_t.data_ptr(), n, cf_t.data_ptr(), len(cf),
                                     order_t.data_ptr(), of_t.data_ptr(), msgs_t.data_ptr(), cfm_t.data_ptr(),
                                     sf_t.data_ptr(), counts_t.data_ptr(), ws.data_ptr(), ws.numel(), s)
        assert rc == 0, L.cfws_last_error()

    med, lo = median_us(call, steps, warmup)
    row["device_us"], row["device_us_min"] = round(med, 1), round(lo, 1)
    row["device_Grecords_s"] = round(n / med / 1e3, 4)
    # the device tables against the host form's
    frames, rows = counts[1] + counts[3], counts[0] + counts[2]
    ok = counts_t.tolist() == counts and \
        np.array_equal(order_t[:frames].cpu().numpy().view(np.uint64), host[0]) and \
        np.array_equal(of_t[:frames].cpu().numpy().view(np.uint32), host[1]) and \
        cfws.h2_stream_msgs_from_device(msgs_t[:rows]).tobytes() == host[2].tobytes() and \
        np.array_equal(cfm_t.cpu().numpy().view(np.uint64), host[3]) and \
        np.array_equal(sf_t[:counts[4]].cpu().numpy().view(np.uint64), host[4])
    row["verified"] = bool(ok)
    del host

    # today's alternative: D2H of the records into pinned memory, then the host form
    h_starts = torch.empty(n, dtype=torch.int64, pin_memory=True)
    h_info = torch.empty((n, 16), dtype=torch.uint8, pin_memory=True)
    h_cf = torch.empty(len(cf), dtype=torch.int64, pin_memory=True)

    def d2h():
        h_starts.copy_(starts_t, non_blocking=True)
        h_info.copy_(info_t, non_blocking=True)
        h_cf.copy_(cf_t, non_blocking=True)

    d2h_us, _ = median_us(d2h, max(steps // 4, 5), 2)
    row["d2h_us"] = round(d2h_us, 1)
    row["host_total_16t_us"] = round(d2h_us + row["host_walk_16t_us"], 1)
    row["device_over_host_16t"] = round(med / row["host_total_16t_us"], 4)
    del h_starts, h_info, h_cf

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
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
