"""UTF-8 check of received text messages, in one process,
per shape and content:
  device  cfws_utf8_messages_batch over a device-resident arena and rows;
  host    what a caller without it does: copy the text bytes to pinned host
          memory (timed between events), then cfws_utf8_check_messages from
          16 native threads (tools/utf8_host_walk.cpp; median of 3);
  copy    cfws_device_copy of the same number of bytes: it reads and writes
          what the call only reads, so its rate is the yardstick, not a floor.
Shapes (every message TEXT and FINAL, back to back in the arena):
  16m_256   16,777,216 messages of 256 B;
  config3   config 3's message sizes (Zipf, 64 B .. 1 MiB, about 4 GiB);
  64k_64k   65,536 messages of 64 KiB.
Contents: ascii; mixed (1- to 4-byte characters in 4-byte cells, so that every
message, a multiple of 4 bytes at a multiple of 4, is well-formed); mixed_bad
(the same with one FF byte in every 100th message).
Device calls: --warmup calls, then --steps calls each timed as a whole call
between two events, one synchronise at the end; medians. The device rows are
compared with the host form's, byte for byte, for every shape and content. One
JSON line each; --out appends them to a file. There is no CPU fall-back: the
tool needs a GPU.
  python3 tools/utf8_bench.py [--steps 20] [--warmup 3] [--out FILE] [--shapes a,b] [--contents a,b] [--no-host]"""
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

BLOCK_CELLS = 1 << 18           # the content repeats a block of 1 MiB


def sizes_16m_256():
    return np.full(1 << 24, 256, dtype=np.uint64)


def sizes_config3():
    c3 = W.CONFIG3
    _, messages = W.zipf_batch(c3["target_bytes"], c3["seed"], c3["key_seed"])
    return np.asarray(messages["len"], dtype=np.uint64)


def sizes_64k_64k():
    return np.full(1 << 16, 1 << 16, dtype=np.uint64)


SHAPES = {"16m_256": sizes_16m_256, "config3": sizes_config3, "64k_64k": sizes_64k_64k}
CONTENTS = ("ascii", "mixed", "mixed_bad")


def rows_of(sizes):
    assert not (sizes % 4).any()
    r = np.zeros(len(sizes), dtype=cfws.MESSAGE_DTYPE)
    r["payload_size"] = sizes
    r["payload_off"] = np.cumsum(sizes) - sizes
    r["first_frame"], r["n_fragments"] = np.arange(len(sizes), dtype=np.uint32), 1
    r["opcode"], r["flags"] = 1, 1
    return r


def mixed_block(rng):
    """BLOCK_CELLS cells of 4 bytes, each one of 64 drawn cells of whole characters."""
    def char(k):
        lo, hi = [(0x20, 0x7F), (0x80, 0x800), (0x800, 0xD800), (0x10000, 0x110000)][k - 1]
        return chr(int(rng.integers(lo, hi))).encode("utf-8")
    patterns = [(1, 1, 1, 1), (2, 2), (1, 3), (3, 1), (4,), (1, 1, 2), (2, 1, 1), (1, 2, 1)]
    cells = np.array([list(b"".join(char(k) for k in patterns[i % len(patterns)])) for i in range(64)], dtype=np.uint8)
    return cells[rng.integers(0, 64, BLOCK_CELLS)].reshape(-1)


def fill(arena, nbytes, rows, content, rng):
    if content == "ascii":
        arena.fill_(0x61)
        return
    block = torch.from_numpy(mixed_block(rng)).cuda()
    reps = (nbytes + block.numel() - 1) // block.numel()
    arena[:nbytes] = block.repeat(reps)[:nbytes]
    if content == "mixed_bad":
        idx = np.arange(37, len(rows), 100)
        at = rows["payload_off"][idx] + (idx.astype(np.uint64) * np.uint64(2654435761)) % rows["payload_size"][idx]
        arena[torch.from_numpy(at.astype(np.int64)).cuda()] = 0xFF


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


def host_lib():
    so = os.path.join(ROOT, "build", "libutf8hostwalk.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", ROOT, "build/libutf8hostwalk.so"], check=True)
    H = C.CDLL(so)
    H.utf8_host_walk.restype = C.c_uint64
    H.utf8_host_walk.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    return H


def measure(name, contents, steps, warmup, host, out):
    sizes = SHAPES[name]()
    rows = rows_of(sizes)
    n, nbytes = len(rows), int(sizes.sum())
    assert nbytes % 16 == 0
    cfws.init()
    L = cfws.lib()
    s = torch.cuda.current_stream().cuda_stream
    arena = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    msgs_t = torch.from_numpy(rows.view(np.uint8).reshape(-1, 32)).cuda()
    result_t = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    bad_t = torch.empty(n, dtype=torch.int32, device="cuda")
    counts_t = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = cfws.utf8_workspace(n)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    copy_us, _ = median_us(lambda: cfws.device_copy(arena, dst, nbytes), steps, warmup)
    del dst
    h_arena = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if host else None
    h_result = np.zeros(n, dtype=cfws.UTF8_RESULT_DTYPE)
    H = host_lib() if host else None
    rng = np.random.default_rng(18)

    def call():
        rc = L.cfws_utf8_messages_batch(arena.data_ptr(), nbytes, msgs_t.data_ptr(), n, None, result_t.data_ptr(),
                                        bad_t.data_ptr(), n, counts_t.data_ptr(), ws.data_ptr(), ws.numel(), s)
        assert rc == 0, L.cfws_last_error()

    for content in contents:
        fill(arena, nbytes, rows, content, rng)
        row = {"shape": name, "content": content, "messages": n, "bytes": nbytes, "steps": steps, "warmup": warmup,
               "workspace_bytes": ws.numel()}
        med, lo = median_us(call, steps, warmup)
        row["device_us"], row["device_us_min"] = round(med, 1), round(lo, 1)
        row["device_GB_s"] = round(nbytes / med / 1e3, 1)
        row["copy_us"] = round(copy_us, 1)
        row["copy_GB_s_read"] = round(nbytes / copy_us / 1e3, 1)
        row["device_over_copy"] = round(med / copy_us, 2)
        row["checked"], row["bad"] = counts_t.tolist()
        if host:
            d2h_us, _ = median_us(lambda: h_arena.copy_(arena, non_blocking=True), 3, 1)
            counts = np.zeros(2, dtype=np.uint64)
            ns = [H.utf8_host_walk(h_arena.data_ptr(), nbytes, rows.ctypes.data, n, 16, h_result.ctypes.data,
                                   counts.ctypes.data) for _ in range(3)]
            row["d2h_us"], row["host_walk_16t_us"] = round(d2h_us, 1), round(statistics.median(ns) / 1e3, 1)
            row["host_total_16t_us"] = round(row["d2h_us"] + row["host_walk_16t_us"], 1)
            row["device_over_host_16t"] = round(med / row["host_total_16t_us"], 5)
            row["verified"] = bool(counts.tolist() == [row["checked"], row["bad"]] and
                                   result_t.cpu().numpy().tobytes() == h_result.tobytes())
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--contents", default=",".join(CONTENTS))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("utf8_bench: no GPU; nothing is measured without one")
    for name in a.shapes.split(","):
        measure(name, a.contents.split(","), a.steps, a.warmup, not a.no_host, a.out)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
