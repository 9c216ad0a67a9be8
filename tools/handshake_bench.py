"""The upgrade's key calls on one device, n connections each:
  client_keys    cfws_ws_client_keys_batch (keys and expected accepts);
  client_today   what a caller could do before it, device parts only:
                 cfws_draw_mask_keys_device of 4 n words (the nonces) plus
                 cfws_ws_accept_keys_batch over the keys (encoded on the host,
                 not timed, as is the copy between the two);
  upgrade_keys   cfws_ws_upgrade_keys_batch over n valid keys;
  accept_keys    cfws_ws_accept_keys_batch over the same keys.
Each between two events around --steps launches after --warmup untimed ones.
Outside the timed loops the outputs are compared with each other and with the
Python restatement on a sample. One JSON line per call: ms per launch and
keys/s. Without a GPU the measured fields read "not measured".
  python3 tools/handshake_bench.py [--n 1048576] [--steps 20] [--warmup 3]"""
import argparse
import base64
import hashlib
import json
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from coldforce_amd import cfws  # noqa: E402

SEED = 1234
FIRST = 1000003
GUID = b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11"


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = cfws.TimingEvent(), cfws.TimingEvent()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    del a, b
    return ms


def row(name, n, ms, ok, steps, warmup):
    return {"call": name, "n": n, "steps": steps, "warmup": warmup, "ms_per_launch": round(ms, 4),
            "G_keys_per_s": round(n / (ms / 1e3) / 1e9, 2), "verified": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = a.n
    if not torch.cuda.is_available():
        for name in ("client_keys", "client_today", "upgrade_keys", "accept_keys"):
            print(json.dumps({"call": name, "n": n, "ms_per_launch": "not measured"}))
        return
    cfws.init()
    L, st = cfws.lib(), cfws._stream(None)
    keys_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    exp_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    nxt_t = torch.zeros(1, dtype=torch.int64, device="cuda")

    def client():
        cfws.ws_client_keys_into(n, keys_t, exp_t, nxt_t, SEED, FIRST)

    ms = timed(client, a.steps, a.warmup)
    slots = keys_t.cpu().numpy().reshape(n, 32)
    sample = list(range(0, n, max(n // 997, 1))) + [n - 1]
    words, _ = cfws.draw_mask_keys_at(4 * n, None, SEED, FIRST)
    nonces = words.astype("<u4").tobytes()
    exp = exp_t.cpu().numpy().reshape(n, 32)
    ok = int(nxt_t.item()) == FIRST + 16 * n
    for c in sample:
        k = base64.b64encode(nonces[16 * c:16 * c + 16])
        ok = ok and bytes(slots[c]) == k + bytes(8)
        ok = ok and bytes(exp[c]) == base64.b64encode(hashlib.sha1(k + GUID).digest()) + bytes(4)
    print(json.dumps(row("client_keys", n, ms, ok, a.steps, a.warmup)), flush=True)

    # today's route: the nonces drawn on the device, the keys encoded on the host, the accepts on the device
    packed = torch.from_numpy(np.ascontiguousarray(slots[:, :24]).reshape(-1)).cuda()
    off = torch.arange(0, 24 * (n + 1), 24, dtype=torch.int64, device="cuda")
    nonce_t = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    acc_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")

    def today():
        cfws.draw_mask_keys_device(4 * n, None, SEED, FIRST, nonce_t, nxt_t)
        cfws._check(L.cfws_ws_accept_keys_batch(cfws._p(packed), cfws._p(off), n, cfws._p(acc_t), st), "accept")

    ms = timed(today, a.steps, a.warmup)
    ok = torch.equal(acc_t, exp_t) and nonce_t.cpu().numpy().tobytes() == nonces
    print(json.dumps(row("client_today", n, ms, ok, a.steps, a.warmup)), flush=True)

    valid_t = torch.zeros(n, dtype=torch.uint8, device="cuda")
    up_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    cnt_t = torch.zeros(1, dtype=torch.int32, device="cuda")

    def upgrade():
        cfws._check(L.cfws_ws_upgrade_keys_batch(cfws._p(packed), cfws._p(off), n, cfws._p(valid_t), cfws._p(up_t),
                                                 cfws._p(cnt_t), st), "upgrade")

    def accept():
        cfws._check(L.cfws_ws_accept_keys_batch(cfws._p(packed), cfws._p(off), n, cfws._p(acc_t), st), "accept")

    ms = timed(upgrade, a.steps, a.warmup)
    ok = torch.equal(up_t, exp_t) and bool(valid_t.all()) and int(cnt_t.item()) == 0
    print(json.dumps(row("upgrade_keys", n, ms, ok, a.steps, a.warmup)), flush=True)
    ms = timed(accept, a.steps, a.warmup)
    print(json.dumps(row("accept_keys", n, ms, torch.equal(acc_t, exp_t), a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
