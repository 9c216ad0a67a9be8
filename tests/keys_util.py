"""The mask-key stream restated in Python integers: the independent oracle
for positions a sequential draw cannot reach (tests/test_keys_host.py pins it
to tests/golden/keys.json, the reference's own keys, and to libc's
srandom/random before anything is compared with it).

Only the seeded table comes from outside: glibc's initstate_r through ctypes.
With h[0..30] the table's words in draw order from the front pointer, the
t-th random() since srandom(seed) is h[t + 31] >> 1 with
h[t + 31] = h[t + 28] + h[t] (mod 2^32). The recurrence's characteristic
polynomial is p = x^31 - x^28 - 1, and with q = x^k mod p,
h[k + j] = sum_c q[c] h[c + j]. Everything here is mod 2^32 (the library
works mod 2^9)."""
import ctypes as C

import numpy as np

DEG, TAP, M32 = 31, 28, 0xFFFFFFFF


class _RandomData(C.Structure):
    """glibc's struct random_data (stdlib.h)."""
    _fields_ = [("fptr", C.POINTER(C.c_int32)), ("rptr", C.POINTER(C.c_int32)), ("state", C.POINTER(C.c_int32)),
                ("rand_type", C.c_int), ("rand_deg", C.c_int), ("rand_sep", C.c_int),
                ("end_ptr", C.POINTER(C.c_int32))]


def seeded_table(seed: int) -> list:
    """h[0..30] after srandom(seed)."""
    libc = C.CDLL(None)
    table = (C.c_int32 * 32)()
    rd = _RandomData()
    assert libc.initstate_r(C.c_uint(seed), C.cast(table, C.c_char_p), C.c_size_t(128), C.byref(rd)) == 0
    assert (rd.rand_deg, rd.rand_sep) == (DEG, DEG - TAP)
    front = (C.addressof(rd.fptr.contents) - C.addressof(rd.state.contents)) // 4
    return [rd.state[(front + i) % DEG] & M32 for i in range(DEG)]


def draws(h: list, count: int) -> list:
    """The next `count` random() returns from the 31 words h."""
    h = list(h)
    for t in range(count):
        h.append((h[t + TAP] + h[t]) & M32)
    return [x >> 1 for x in h[DEG:]]


def poly_mul(a: list, b: list) -> list:
    r = [0] * (2 * DEG - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                r[i + j] += x * y
    for k in range(2 * DEG - 2, DEG - 1, -1):          # x^k = x^(k - 3) + x^(k - 31)
        r[k - (DEG - TAP)] += r[k]
        r[k - DEG] += r[k]
    return [x & M32 for x in r[:DEG]]


def xpow(k: int) -> list:
    """x^k mod p."""
    q = [1] + [0] * (DEG - 1)
    x = [0, 1] + [0] * (DEG - 2)
    for bit in bin(k)[2:]:
        q = poly_mul(q, q)
        if bit == "1":
            q = poly_mul(q, x)
    return q


def state_at(h: list, k: int) -> list:
    """The 31 words k draws after h."""
    w = list(h)
    for t in range(DEG - 1):
        w.append((w[t + TAP] + w[t]) & M32)
    q = xpow(k)
    return [sum(q[c] * w[c + j] for c in range(DEG)) & M32 for j in range(DEG)]


def keys_at(seed: int, first_draw: int, n: int, mask_flags=None):
    """(keys, next_draw) as cfws_draw_mask_keys_seeded_at defines them."""
    flags = np.ones(n, np.uint8) if mask_flags is None else np.asarray(mask_flags)
    masked = int(np.count_nonzero(flags[:n]))
    r = draws(state_at(seeded_table(seed), first_draw), 4 * masked)
    packed = [(r[4 * m] & 255) | (r[4 * m + 1] & 255) << 8 | (r[4 * m + 2] & 255) << 16 | (r[4 * m + 3] & 255) << 24
              for m in range(masked)]
    keys = np.zeros(n, np.uint32)
    keys[np.nonzero(flags[:n])[0]] = packed
    return keys, first_draw + 4 * masked
