"""HTTP/2 receive-buffer indexing, in one process:
  device  cfws_h2_index_frames_batch, select ALL and DATA, with d_info, and
          ALL without it (starts only, as the WS indexer reports);
  ws      cfws_index_frames_batch over the WS-only form of the same frames
          (the hop rate to compare with);
  host    cfws_h2_index_frames over the same bytes in host memory, on 1 and
          on 16 threads (one call per connection, from native threads:
          tools/h2_index_host_walk.cpp; median of 5 ticks).
Shapes: a tick of 16,384 connections x 64 KiB, every buffer cut inside its
last frame:
  1k    DATA frames of one client-masked 1 KiB WS frame (1,041 bytes each);
  16k   16,393-byte DATA frames (config 5's 16,376-byte payload + the 8-byte
        masked WS header + the 9-byte DATA header).
Device calls: --warmup calls, then --steps calls each timed as a whole call
between two events, one synchronise at the end; medians. One JSON line per
shape (G frames/s and us per launch); --out appends them to a file. Without
a GPU the device fields read "not measured".
  python3 tools/h2_index_bench.py [--steps 20] [--warmup 3] [--out FILE]"""
import argparse
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

CONNS, CONN_BYTES = 16384, 65536
SHAPES = {"1k": 1024, "16k": 16376}


def ws_frame(rng, payload: int) -> bytes:
    assert 126 <= payload < 65536
    return bytes([0x82, 0xFE, payload >> 8, payload & 0xff]) + rng.bytes(4) + rng.bytes(payload)


def connection(rng, payload: int):
    """One connection's 64 KiB as HTTP/2 DATA frames and as bare WS frames:
    the same complete frames, then a frame cut short."""
    ws = ws_frame(rng, payload)
    data = (len(ws)).to_bytes(3, "big") + bytes([0, 1, 0, 0, 0, 1]) + ws
    k = CONN_BYTES // len(data)
    h2 = (data * (k + 1))[:CONN_BYTES]
    cut = CONN_BYTES - k * len(data)
    wsb = ws * k + ws[:max(cut - 9, 1)]
    return h2, wsb, k


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


def host_walk(arena: np.ndarray, select: int, threads: int, reps: int = 5):
    """Median us of the native host tick (tools/h2_index_host_walk.cpp)."""
    import ctypes as C
    so = os.path.join(ROOT, "build", "libh2hostwalk.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", ROOT, "build/libh2hostwalk.so"], check=True)
    H = C.CDLL(so)
    H.h2_host_walk.restype = C.c_uint64
    H.h2_host_walk.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    frames = C.c_uint64()
    ns = [H.h2_host_walk(arena.ctypes.data, CONNS, CONN_BYTES, select, threads, C.byref(frames))
          for _ in range(reps)]
    return statistics.median(ns) / 1e3, frames.value


def measure(name, payload, steps, warmup):
    rng = np.random.default_rng(payload)
    h2, wsb, k = connection(rng, payload)
    frames = CONNS * k
    row = {"shape": name, "conns": CONNS, "conn_bytes": CONN_BYTES, "ws_payload": payload,
           "data_frame_bytes": payload + 8 + 9, "frames_per_conn": k, "frames": frames, "steps": steps,
           "warmup": warmup}
    arena = np.tile(np.frombuffer(h2, np.uint8), CONNS)
    for threads in (1, 16):
        us, total = host_walk(arena, cfws.H2_INDEX_ALL, threads)
        assert total == frames
        row[f"host_{threads}t_us"] = round(us, 1)
        row[f"host_{threads}t_Gframes_s"] = round(frames / us / 1e3, 4)
    if not torch.cuda.is_available():
        for f in ("h2_all_us", "h2_data_us", "h2_all_no_info_us", "ws_us", "h2_all_Gframes_s", "h2_data_Gframes_s",
                  "h2_all_no_info_Gframes_s", "ws_Gframes_s", "verified"):
            row[f] = "not measured"
        return row
    cfws.init()
    dev = "cuda"
    buf = torch.from_numpy(arena).to(dev)
    del arena
    wst = torch.zeros(CONNS * CONN_BYTES, dtype=torch.uint8, device=dev).view(CONNS, CONN_BYTES)
    wst[:, :len(wsb)] = torch.from_numpy(np.frombuffer(wsb, np.uint8).copy()).to(dev)
    wst = wst.view(-1)
    begin = torch.arange(CONNS, dtype=torch.int64, device=dev) * CONN_BYTES
    end = begin + CONN_BYTES
    ws_end = begin + len(wsb)
    starts = torch.empty(frames + 16, dtype=torch.int64, device=dev)
    info = torch.empty((frames + 16, 16), dtype=torch.uint8, device=dev)
    h2_ws = torch.empty(cfws.lib().cfws_h2_index_workspace_size(CONNS), dtype=torch.uint8, device=dev)
    ix_ws = torch.empty(cfws.lib().cfws_index_workspace_size(CONNS), dtype=torch.uint8, device=dev)
    outs = [torch.empty(CONNS, dtype=dt, device=dev) for dt in (torch.int64, torch.int64, torch.int32)]
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    L = cfws.lib()
    st = torch.cuda.current_stream().cuda_stream

    def h2(select, with_info=True):
        rc = L.cfws_h2_index_frames_batch(buf.data_ptr(), begin.data_ptr(), end.data_ptr(), CONNS, 0, select, 0,
                                          starts.data_ptr(), info.data_ptr() if with_info else None,
                                          starts.numel(), outs[0].data_ptr(),
                                          outs[1].data_ptr(), outs[2].data_ptr(), total.data_ptr(),
                                          h2_ws.data_ptr(), h2_ws.numel(), st)
        assert rc == 0, L.cfws_last_error()

    def ws():
        rc = L.cfws_index_frames_batch(wst.data_ptr(), begin.data_ptr(), ws_end.data_ptr(), CONNS,
                                       cfws.DEFAULT_MAX_PAYLOAD, starts.data_ptr(), starts.numel(),
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                       total.data_ptr(), ix_ws.data_ptr(), ix_ws.numel(), st)
        assert rc == 0, L.cfws_last_error()

    ok = True
    for key, fn in (("h2_all", lambda: h2(cfws.H2_INDEX_ALL)), ("h2_data", lambda: h2(cfws.H2_INDEX_DATA)),
                    ("h2_all_no_info", lambda: h2(cfws.H2_INDEX_ALL, False)), ("ws", ws)):
        med, lo = median_us(fn, steps, warmup)
        row[f"{key}_us"], row[f"{key}_us_min"] = round(med, 1), round(lo, 1)
        row[f"{key}_Gframes_s"] = round(frames / med / 1e3, 4)
        ok = ok and int(total.item()) == frames and bool((outs[2] == 1).all())      # every buffer is cut
    row["h2_all_over_ws"] = round(row["h2_all_us"] / row["ws_us"], 3)
    row["h2_all_over_host_16t"] = round(row["h2_all_us"] / row["host_16t_us"], 4)
    row["verified"] = bool(ok)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("at least 20 steps")
    for name, payload in SHAPES.items():
        line = json.dumps(measure(name, payload, a.steps, a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
