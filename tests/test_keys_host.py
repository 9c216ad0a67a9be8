"""CPU checks of the key stream entered at a position
(cfws_draw_mask_keys_seeded_at, include/cfws.h) and of the Python oracle the
GPU tests use for positions no sequential draw reaches (tests/keys_util.py).
The oracle is pinned first: to the reference's own keys
(tests/golden/keys.json) and to libc's srandom/random."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keys_util as KU
from conftest import ROOT, golden

from coldforce_amd import cfws

LIB = os.path.join(ROOT, "coldforce_amd", "libcfws.so")
SEEDS = (0, 1, 2, 1234, 0xFFFFFFFF)
FIRST = (0, 1, 2, 3, 4, 5, 30, 31, 32, 61, 62, 310, 65537, 1000003)
FAR = (2**32 + 1, 2**40 + 3, 2**62)
N = 3000


def _flags(mode, n=N):
    if mode == "none":
        return None
    if mode == "random":
        return (np.random.default_rng(5).random(n) < .6).astype(np.uint8)
    return np.full(n, 1 if mode == "ones" else 0, np.uint8)


def test_oracle_reproduces_the_reference_keys():
    for seed, ks in golden("keys.json").items():
        got, nxt = KU.keys_at(int(seed), 0, len(ks))
        assert [int.from_bytes(bytes.fromhex(k), "little") for k in ks] == [int(x) for x in got], seed
        assert nxt == 4 * len(ks)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_reproduces_libc_random(seed):
    libc = ctypes.CDLL(None)
    libc.random.restype = ctypes.c_long
    libc.srandom(ctypes.c_uint(seed))
    want = [libc.random() for _ in range(3000)]
    h = KU.seeded_table(seed)
    assert KU.draws(h, 3000) == want
    # and entered at a position: the jump against the direct recurrence
    for k in (1, 31, 1000, 2999):
        assert KU.draws(KU.state_at(h, k), 1) == [want[k]], k


@pytest.fixture(scope="module")
def long_stream():
    """One sequential draw per seed, as bytes: draw t is byte t."""
    frames = (max(FIRST) + 4 * N) // 4 + 1
    return {seed: cfws.draw_mask_keys(frames, seed=seed).view(np.uint8) for seed in SEEDS}


@pytest.mark.parametrize("mode", ["none", "random", "zeros", "ones"])
@pytest.mark.parametrize("seed", SEEDS)
def test_at_equals_the_slice_of_one_long_draw(long_stream, seed, mode):
    flags = _flags(mode)
    masked = N if flags is None else int(flags.sum())
    where = np.arange(N) if flags is None else np.nonzero(flags)[0]
    for first in FIRST:
        keys, nxt = cfws.draw_mask_keys_at(N, flags, seed, first)
        assert nxt == first + 4 * masked, (first, nxt)
        want = np.zeros(N, np.uint32)
        want[where] = long_stream[seed][first:first + 4 * masked].copy().view(np.uint32)
        bad = np.nonzero(keys != want)[0]
        assert bad.size == 0, f"first_draw {first}: {bad.size} keys differ, first at {bad[:4]}"


def test_first_draw_zero_is_the_seeded_draw():
    flags = _flags("random")
    for seed in SEEDS:
        keys, _ = cfws.draw_mask_keys_at(N, flags, seed, 0)
        assert np.array_equal(keys, cfws.draw_mask_keys(N, flags, seed=seed))


@pytest.mark.parametrize("first", FAR)
def test_at_equals_the_oracle_far_out(first):
    flags = (np.random.default_rng(first % 1000).random(64) < .6).astype(np.uint8)
    for seed in SEEDS:
        for f in (None, flags):
            keys, nxt = cfws.draw_mask_keys_at(64, f, seed, first)
            want, want_next = KU.keys_at(seed, first, 64, f)
            assert np.array_equal(keys, want) and nxt == want_next, (seed, first)


def test_composition():
    """The tail of _at(a, n) is _at(a + 4 k, n - k)."""
    a, n = 2**40 + 3, 500
    whole, nxt = cfws.draw_mask_keys_at(n, None, 1234, a)
    for k in (1, 7, 31, 499):
        tail, nxt_k = cfws.draw_mask_keys_at(n - k, None, 1234, a + 4 * k)
        assert np.array_equal(whole[k:], tail) and nxt_k == nxt, k
    # with flags: continue at the next position the first part returned
    flags = _flags("random", n)
    whole, nxt = cfws.draw_mask_keys_at(n, flags, 1234, a)
    head, mid = cfws.draw_mask_keys_at(200, flags[:200], 1234, a)
    tail, end = cfws.draw_mask_keys_at(n - 200, flags[200:], 1234, mid)
    assert np.array_equal(np.concatenate([head, tail]), whole) and end == nxt


def test_keeps_the_global_stream():
    libc = ctypes.CDLL(None)
    libc.random.restype = ctypes.c_long
    libc.srandom(ctypes.c_uint(99))
    before = libc.random()
    libc.srandom(ctypes.c_uint(99))
    cfws.draw_mask_keys_at(N, _flags("random"), 7, 1000003)
    assert libc.random() == before


def test_argument_errors():
    L = cfws.lib()
    keys = np.zeros(4, np.uint32)
    nxt = ctypes.c_uint64(123)
    assert L.cfws_draw_mask_keys_seeded_at(1, 2**62 + 1, 4, None, keys.ctypes.data, ctypes.byref(nxt)) == \
        cfws.ERROR_INVALID_ARGUMENT
    assert L.cfws_draw_mask_keys_seeded_at(1, 0, 4, None, None, ctypes.byref(nxt)) == cfws.ERROR_INVALID_ARGUMENT
    assert nxt.value == 123
    # nothing to draw needs no keys; the next position may be left out
    assert L.cfws_draw_mask_keys_seeded_at(1, 5, 0, None, None, ctypes.byref(nxt)) == cfws.OK and nxt.value == 5
    assert L.cfws_draw_mask_keys_seeded_at(1, 2**62, 4, None, keys.ctypes.data, None) == cfws.OK


def test_library_exports_the_key_functions():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    names = {"cfws_draw_mask_keys_seeded_at", "cfws_draw_mask_keys_device", "cfws_draw_keys_workspace_size",
             "cfws_draw_keys_group_frames"}
    assert names <= exported
    assert names <= set(cfws.BATCH_SYMBOLS)


def test_workspace_size_and_group_are_host_only():
    L = cfws.lib()
    G = L.cfws_draw_keys_group_frames()
    assert G > 0 and G % 64 == 0
    sizes = [L.cfws_draw_keys_workspace_size(n) for n in (0, 1, 5, G - 1, G, G + 1, 1 << 20, 16 << 20)]
    assert sizes == sorted(sizes)
    assert all(s >= 4 * n for s, n in zip(sizes, (0, 1, 5, G - 1, G, G + 1, 1 << 20, 16 << 20)))
