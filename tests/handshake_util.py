"""The upgrade's key handling restated in Python (co_ws_http_extension.c),
for the tests of cfws_ws_client_keys_batch, cfws_ws_upgrade_keys_batch and
cfws_ws_check_accept_batch. tests/test_handshake_rules.py pins every function
here to the reference's own co_random, co_base64_encode, co_base64_decode and
co_ws_frame_serialize (tests/golden/handshake_client_cases.json, and the
reference itself where oracle/_ref is built)."""
import base64
import ctypes as C
import hashlib

import numpy as np

from coldforce_amd import cfws

GUID = b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11"
NONCE = 16

# co_base64_decode's treatment of a byte (co_base64.c:101-119, :128-162)
SKIPPED = frozenset(b"\n\r=")
DATA = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/!-:_") | frozenset(range(128, 256))

# the bytes an edited key draws from: both alphabets' ends, the second
# spellings, the skipped bytes, failing neighbours and the table's upper half
EDIT_BYTES = b"AZaz09+/!-:_=\r\n *@[`{\x7f\x80\xff"


def accept_of(key: bytes) -> str:
    """co_ws_create_base64_accept_key (:26-57)."""
    return base64.b64encode(hashlib.sha1(key + GUID).digest()).decode()


def client_keys(seed: int, first_draw: int, n: int):
    """n sequential co_http_request_create_ws_upgrade keys (:280-290) after
    first_draw calls of random() since srandom(seed): (keys, accepts, next)."""
    words, _ = cfws.draw_mask_keys_at(4 * n, None, seed, first_draw)
    nonces = words.astype("<u4").tobytes()
    keys = [base64.b64encode(nonces[NONCE * c:NONCE * (c + 1)]) for c in range(n)]
    return keys, [accept_of(k) for k in keys], first_draw + NONCE * n


def decode_result(key: bytes):
    """co_base64_decode's (return value, *dest_length) for a key: the length
    starts at (size_t)(L / 4.0 * 3) and drops by 1 per skipped byte up to the
    first failing byte, where the decode stops."""
    length = 3 * len(key) // 4
    for b in key:
        if b in SKIPPED:
            length -= 1
        elif b not in DATA:
            return False, length % 2**64
    return True, length % 2**64                        # size_t: it wraps below zero


def key_valid(key: bytes) -> bool:
    """co_http_request_validate_ws_upgrade's key decision (:156-170)."""
    ok, length = decode_result(key)
    return ok and length == NONCE


def check(expect: bytes, answer: bytes) -> bool:
    """strcmp(answer, expect) == 0 (:247), both read as C strings."""
    return answer.split(b"\0", 1)[0] == expect.split(b"\0", 1)[0]


def edited_keys(rng, count: int) -> list[bytes]:
    """base64 of 16 random bytes with 0-3 edits: a byte of EDIT_BYTES
    replaces one, is inserted, or one is deleted. rng: random.Random."""
    out = []
    for _ in range(count):
        k = bytearray(base64.b64encode(rng.randbytes(NONCE)))
        for _ in range(rng.randrange(4)):
            how = rng.randrange(3)
            if how == 0 and k:
                k[rng.randrange(len(k))] = rng.choice(EDIT_BYTES)
            elif how == 1 and k:
                del k[rng.randrange(len(k))]
            else:
                k.insert(rng.randrange(len(k) + 1), rng.choice(EDIT_BYTES))
        out.append(bytes(k))
    return out


# ---- the reference's own functions, through oracle.ref_lib() -----------------

def _libc_free():
    f = C.CDLL(None).free
    f.argtypes = [C.c_void_p]
    f.restype = None
    return f


def ref_random(R, n: int) -> bytes:
    """co_random(buffer, n): n draws of random() % 256."""
    buf = C.create_string_buffer(max(n, 1))
    R.co_random.argtypes = [C.c_void_p, C.c_size_t]
    R.co_random.restype = None
    R.co_random(buf, n)
    return buf.raw[:n]


def ref_encode(R, data: bytes) -> bytes:
    """co_base64_encode(data, padding = true)."""
    f = R.co_base64_encode
    f.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_bool]
    f.restype = None
    dest, n = C.c_void_p(), C.c_size_t()
    f(data, len(data), C.byref(dest), C.byref(n), True)
    out = C.string_at(dest.value, n.value)
    assert C.string_at(dest.value) == out              # NUL-terminated at its length
    _libc_free()(dest)
    return out


def ref_client_key(R) -> bytes:
    """The key of one co_http_request_create_ws_upgrade (:280-290) from the
    process's random() state."""
    return ref_encode(R, ref_random(R, NONCE))


def ref_decode(R, key: bytes):
    """co_base64_decode(key, len(key)): (return value, *dest_length)."""
    f = R.co_base64_decode
    f.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    f.restype = C.c_bool
    dest, n = C.c_void_p(), C.c_size_t()
    ok = bool(f(key, len(key), C.byref(dest), C.byref(n)))
    _libc_free()(dest)
    return ok, int(n.value)


def slots(strings, slot: int = 32) -> np.ndarray:
    """Strings as NUL-padded slots, the form the device calls write."""
    a = np.zeros((len(strings), slot), np.uint8)
    for i, s in enumerate(strings):
        b = s if isinstance(s, bytes) else s.encode()
        a[i, :len(b)] = np.frombuffer(b, np.uint8)
    return a.reshape(-1)
