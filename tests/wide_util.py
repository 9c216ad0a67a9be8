"""TEST INFRASTRUCTURE ONLY -- the cases of tests/test_gpu_wide.py and their CPU
half tests/test_wide_cases.py: batch entry points run so that one named offset
operand crosses 2^32 -- some frames wholly below the mark, some wholly at or
above it, at least one whose bytes contain byte 2^32 itself.

Two ways across:

* relocation, for offsets the caller supplies: a problem of at most 2 MiB is
  built and given to the oracle as it is; on the device its window lies at
  [2^32 - delta, ...) of an arena of 2^32 + 4 MiB sentinel bytes, the library
  gets the arena's own base pointer and every offset is the problem's plus the
  window's base. The expectation is the oracle's with that base added to each
  offset field it reports;
* ballast, for offsets the library derives (prefix sums, i * slot): frame 0
  is one frame whose output ends delta bytes below 2^32 (or the frame count
  times the slot passes 2^32) and the frames under test follow it. The
  expectation is the oracle's on those frames alone, shifted by the ballast.

Everything a case builds on the CPU (inputs, expectation, the crossing lists,
the device bytes it will hold) is built once per process and shared; run()
needs a device. Every output arena is checked whole: the expected patches are
compared, blanked with the sentinel on the device, and the arena must then be
the sentinel from its first byte to its last -- a write at offset mod 2^32
lands gigabytes below the window and shows there.
"""
from __future__ import annotations

import numpy as np

import carryover_util as CU
import oracle as O
import relay_util as RU
from coldforce_amd import cfws
from coldforce_amd import workloads as W

MARK = 1 << 32
SENT = 0xEE                              # 0xEE 0xEE parses as INVALID_FRAME (reserved bits)
ARENA_BYTES = MARK + (4 << 20)
WINDOW_MAX = 2 << 20
# a multiple of 4,096, and 16 x an odd number: the frames' phases against the
# 4 KiB regions, the 128-byte lines and the 2 KiB pieces differ between the two
DELTAS = {"page": 64 * 4096, "odd16": 16 * 16385}
INDEX_DELTAS = {"page": 32 * 4096, "odd16": 16 * 8193}      # the indexers' 300 connections are about 220 KB
BUDGET = 24 << 30                        # device bytes one case may hold
BIG_PAYLOAD = 1 << 40                    # max_payload of the calls that carry a ballast frame


def _torch():
    import torch
    return torch


def crossing(starts, lengths) -> dict:
    """The frames (of one byte or more) wholly below 2^32, wholly at or above
    it, and those whose byte range contains byte 2^32; `inside`: the latter
    that also start below it."""
    s = np.asarray(starts).astype(np.uint64).astype(np.int64)
    ln = np.asarray(lengths).astype(np.uint64).astype(np.int64)
    e, has = s + ln, ln > 0
    return dict(below=np.nonzero(has & (e <= MARK))[0], above=np.nonzero(has & (s >= MARK))[0],
                across=np.nonzero(has & (s <= MARK) & (e > MARK))[0],
                inside=np.nonzero(has & (s < MARK) & (e > MARK))[0])


def crosses(c: dict) -> bool:
    return len(c["below"]) > 0 and len(c["above"]) > 0 and len(c["across"]) > 0


# ---- device helpers -----------------------------------------------------------------

def sentinel_arena(nbytes: int, sent: int = SENT):
    torch = _torch()
    t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    t.fill_(sent)
    return t


def put(arena, off: int, data: np.ndarray) -> None:
    arena[off:off + len(data)] = CU._up(np.ascontiguousarray(data, dtype=np.uint8))


def get(arena, off: int, n: int) -> np.ndarray:
    return arena[off:off + n].cpu().numpy()


def assert_all(arena, what: str, lo: int = 0, hi: int | None = None, sent: int = SENT) -> None:
    """arena[lo:hi] is the sentinel, checked in 1 GiB chunks of 8-byte words."""
    torch = _torch()
    hi = arena.numel() if hi is None else hi
    if hi <= lo:
        return
    a, b = min((lo + 7) // 8 * 8, hi), max(hi // 8 * 8, min((lo + 7) // 8 * 8, hi))
    word = int.from_bytes(bytes([sent]) * 8, "little", signed=True)
    spans = [(arena[lo:a], lo, sent), (arena[b:hi], b, sent)]
    words = arena[a:b].view(torch.int64)
    step = 1 << 27
    spans += [(words[i:i + step], a + 8 * i, word) for i in range(0, words.numel(), step)]
    for t, at, v in spans:
        if t.numel() and not bool((t == v).all()):
            bad = torch.nonzero(t != v).reshape(-1)
            first = at + int(bad[0]) * t.element_size()
            raise AssertionError(f"{what}: {bad.numel()} {t.element_size()}-byte units of [{lo}, {hi}) are not the "
                                 f"sentinel, first near byte {first} (2^32 {first - MARK:+d})")


def checksum(t) -> int:
    """A sum over an input arena's words: the same before and after a call."""
    torch = _torch()
    n8 = t.numel() // 8 * 8
    return int(t[:n8].view(torch.int64).sum().item()) + int(t[n8:].sum().item())


def _s64(x: int) -> int:
    return x - (1 << 64) if x >= 1 << 63 else x


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _idx_t(a):
    return CU._up(_u64(a).view(np.int64))


def _sync():
    """The device is idle before a case returns and its tensors go."""
    _torch().cuda.synchronize()


# ---- cases --------------------------------------------------------------------------

class WideCase:
    """name; operand: the offset that crosses 2^32, named in every failure;
    claim: the route the case is there for (None: decided by thresholds only)."""
    operand = ""
    claim = None

    def __init__(self, name):
        self.name = name
        self._b = None

    def built(self) -> dict:
        if self._b is None:
            self._b = self.build()
        return self._b

    def release(self):
        self._b = None

    def msg(self, what):
        return f"{self.name}: {self.operand}: {what}"


# ---- the slot and scatter receives ---------------------------------------------------

W3_LOOSE = ~((0xFF << 32) | (0xFF << 48)) & 0xFFFFFFFFFFFFFFFF     # a frame that is not COMPLETE: fin and mask unspecified
INFO_LOOSE = ~(0xFF << 32) & 0xFFFFFFFFFFFFFFFF


class SlotCase(WideCase):
    """cfws_deserialize_slots / _slots_info, or with scatter _scatter /
    _scatter_info. K distinct frames (a wire window of at most 2 MiB, the
    oracle's problem), n >= K index entries that repeat them in turn.

    wire_delta: the window at 2^32 - delta of a 2^32 + 4 MiB wire arena (d_frame_index
    relocated), None: at 0 of an arena of wire_claim bytes (wire_size = the
    claim, which sets the batch's average frame and with it the route).
    scatter: destinations shuffled in a window at 2^32 - out_delta of a 2^32 +
    4 MiB payload arena (d_payload_off relocated); otherwise i * slot, which
    crosses 2^32 when n * slot does (the ballast form)."""

    def __init__(self, name, operand, claim, slot, sizes, n=None, wire_delta=None, wire_claim=None, scatter=False,
                 out_delta=None, piece_loop=None, seed=1):
        super().__init__(name)
        self.operand, self.claim, self.slot, self.sizes = operand, claim, slot, list(sizes)
        self.K = len(self.sizes)
        self.n = self.K if n is None else n
        self.wire_delta, self.wire_claim, self.scatter, self.out_delta = wire_delta, wire_claim, scatter, out_delta
        self.piece_loop, self.seed = piece_loop, seed
        self.relocated = wire_delta is not None

    def build(self):
        from test_gpu_slots import expect_slots
        rng = np.random.default_rng(self.seed)
        K, sizes = self.K, np.array(self.sizes, dtype=np.uint64)
        room = CU.PAYLOAD_BYTES - int(sizes.max()) - 16
        d = CU._frames_desc(rng, sizes, rng.integers(0, room, K).astype(np.uint64))
        big = sizes > 125
        d["opcode"][big & (d["opcode"] > 2)] = 2
        wire, d = O.serialize_batch(CU.payload_np(), d.view(O.DESC_DTYPE))
        wire = wire.copy()
        starts = d["wire_off"].astype(np.uint64)
        bad = np.arange(3, K, 96)
        wire[starts[bad].astype(np.int64)] |= 0x40                       # reserved bit: INVALID_FRAME
        assert len(wire) <= WINDOW_MAX
        if self.relocated:
            # the wire ends one byte early (the last frame MORE_DATA) and one
            # entry points at its last byte
            wsize = len(wire) - 1
            starts[K // 2] = wsize - 1
            base = MARK - self.wire_delta
            wire_size, wire_bytes = base + wsize, ARENA_BYTES
        else:
            wsize, base = len(wire), 0
            wire_size = wsize if self.wire_claim is None else self.wire_claim
            wire_bytes = W.round16(wire_size) + 16
        # the row of a frame: its slot, or for slots past 2 MiB the part any payload here reaches
        RW = self.slot if self.slot <= WINDOW_MAX else W.round16(int(sizes.max())) + 16
        assert RW == self.slot or int(sizes.max()) <= RW < self.slot      # the slot rule decides alike at RW
        if self.scatter:
            stride = RW + 64
            perm, jit = rng.permutation(K), rng.integers(0, 4, K)
            # a frame that fills its slot goes where byte 2^32 lies, so that its payload holds that byte
            p, r = divmod(self.out_delta, stride)
            fi = int([i for i in np.nonzero(sizes == RW)[0] if i not in bad and i != K // 2][0])
            j = int(np.nonzero(perm == p)[0][0])
            perm[j], perm[fi] = perm[fi], perm[j]
            jit[fi] = min(4, max(r - 1, 0) // 16)
            rel = perm.astype(np.uint64) * np.uint64(stride) + jit.astype(np.uint64) * np.uint64(16)
            wincap = K * stride - 3 * stride - 5                         # the capacity cuts the last slots
            arena, e_d, e_st, _ = expect_slots(wire, wsize, starts, RW, wincap, offs=rel)
            obase = MARK - self.out_delta
            dests, cap, out_bytes, total = rel + np.uint64(obase), obase + wincap, ARENA_BYTES, None
            arena = np.concatenate([arena, np.full(K * stride + RW - len(arena), SENT, np.uint8)])
            rows = np.stack([arena[int(r):int(r) + RW] for r in rel])
        else:
            arena, e_d, e_st, _ = expect_slots(wire, wsize, starts, RW, K * RW)
            rows = arena[:K * RW].reshape(K, RW)
            dests = np.arange(self.n, dtype=np.uint64) * np.uint64(self.slot)
            cap = self.n * self.slot
            out_bytes, total = cap + 4096, cap
        kidx = np.arange(self.n, dtype=np.int64) % K
        index = starts[kidx] + np.uint64(base)
        e_d = e_d.copy()
        e_d["wire_off"] += np.uint64(base)
        plen = np.where(e_st == O.PARSE_COMPLETE, e_d["payload_size"], 0)
        # what the frames occupy of the named operand's arena
        if self.operand == "d_frame_index":
            span = (index, (e_d["payload_size"] + e_d["header_size"].astype(np.uint64))[kidx] *
                    np.isin(e_st, (O.PARSE_COMPLETE, O.ERROR_OUT_OF_MEMORY))[kidx])
        else:
            span = (dests, plen[kidx])
        info = np.zeros(K, dtype=cfws.INFO_DTYPE)
        info["payload_size"] = np.minimum(e_d["payload_size"], np.uint64(0xFFFFFFFF)).astype(np.uint32)
        info["fin"], info["opcode"], info["status"] = e_d["fin"], e_d["opcode"], e_st.astype(np.int16)
        return dict(wire=wire, wsize=wsize, base=base, wire_size=wire_size, wire_bytes=wire_bytes, starts=starts,
                    index=index, kidx=kidx, RW=RW, rows=rows, desc=e_d, status=e_st, info=info, dests=dests, cap=cap,
                    out_bytes=out_bytes, total=total, cross=crossing(*span))

    def route(self) -> str:
        b = self.built()
        return cfws.lib().cfws_deserialize_slots_pass_kernel(self.n, b["wire_size"], self.slot).decode()

    def piece_form(self) -> str | None:
        """deserialize_slots_piece_kernel's form as slots_impl picks it: a
        wave per piece of the slot (straight), or of the average frame (loop)."""
        b, piece = self.built(), 2048
        slot_pieces = (self.slot + piece - 1) // piece
        avg_pieces = (b["wire_size"] // self.n + piece - 1) // piece
        return "loop" if max(avg_pieces, 1) < slot_pieces else "straight"

    def device_bytes(self) -> int:
        b = self.built()
        n = self.n
        # wire, payload arena, index, destinations, descriptors + statuses or infos, and their expectations
        return b["wire_bytes"] + b["out_bytes"] + 8 * n * (2 if self.scatter else 1) + 2 * (36 * n) + (1 << 30)

    # -- the device half --
    def run(self):
        torch = _torch()
        b = self.built()
        n, K, RW, slot = self.n, self.K, b["RW"], self.slot
        wire = sentinel_arena(b["wire_bytes"])
        put(wire, b["base"], b["wire"])
        idx, kidx = _idx_t(b["index"]), CU._up(b["kidx"])
        dests = _idx_t(b["dests"])
        rows = CU._up(b["rows"])
        ok = CU._up(b["status"] == O.PARSE_COMPLETE)[kidx]
        e_st = CU._up(b["status"])[kidx]
        e_desc = CU._up(b["desc"].view(np.int64).reshape(K, 4))[kidx]
        e_desc[:, 0] = dests
        e_info = CU._up(b["info"].view(np.int64))[kidx]
        full = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        loose = torch.tensor([-1, -1, -1, _s64(W3_LOOSE)], dtype=torch.int64, device="cuda")
        iloose = torch.tensor(_s64(INFO_LOOSE), dtype=torch.int64, device="cuda")
        out = sentinel_arena(b["out_bytes"])
        for form in ("desc", "info"):
            tot = None
            if form == "desc":
                d_t = torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
                st_t = torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda")
                if self.scatter:
                    cfws.deserialize_scatter(wire, b["wire_size"], idx, dests, out, slot, d_t, st_t,
                                             max_payload=BIG_PAYLOAD, payload_capacity=b["cap"])
                else:
                    tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
                    cfws.deserialize_slots(wire, b["wire_size"], idx, out, slot, d_t, st_t, tot,
                                           max_payload=BIG_PAYLOAD, payload_capacity=b["cap"])
                torch.cuda.synchronize()
                CU._eq(st_t, e_st, self.msg("statuses"))
                diff = (d_t.view(torch.int64).reshape(n, 4) ^ e_desc) & torch.where(ok[:, None], full[None, :], loose[None, :])
                bad = torch.nonzero(diff.any(dim=1)).reshape(-1)
                assert bad.numel() == 0, self.msg(f"{bad.numel()} descriptors differ, first frames {bad[:6].tolist()}")
                del d_t, st_t, diff
            else:
                i_t = torch.full((n, 8), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
                if self.scatter:
                    cfws.deserialize_scatter_info(wire, b["wire_size"], idx, dests, out, slot, i_t,
                                                  max_payload=BIG_PAYLOAD, payload_capacity=b["cap"])
                else:
                    tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
                    cfws.deserialize_slots_info(wire, b["wire_size"], idx, out, slot, i_t, tot,
                                                max_payload=BIG_PAYLOAD, payload_capacity=b["cap"])
                torch.cuda.synchronize()
                diff = (i_t.view(torch.int64).reshape(n) ^ e_info) & torch.where(ok, full[0], iloose)
                bad = torch.nonzero(diff).reshape(-1)
                assert bad.numel() == 0, self.msg(f"{bad.numel()} info entries differ, first frames {bad[:6].tolist()}")
                del i_t, diff
            if tot is not None:
                assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
            self._check_rows(out, dests, rows, kidx, form)
            assert_all(out, self.msg(f"payload arena outside the frames' rows ({form})"))
        # the wire arena: the window unchanged, everything else still the sentinel
        got = get(wire, b["base"], len(b["wire"]))
        assert np.array_equal(got, b["wire"]), self.msg("the wire window changed")
        wire[b["base"]:b["base"] + len(b["wire"])].fill_(SENT)
        assert_all(wire, self.msg("wire arena"))
        _sync()

    def _check_rows(self, out, dests, rows, kidx, form):
        """Every frame's row of RW bytes against the oracle's, then blanked."""
        torch = _torch()
        n, RW, slot = self.n, self.built()["RW"], self.slot
        step = max(1, (1 << 28) // RW)
        ar = torch.arange(RW, device="cuda")
        for a in range(0, n, step):
            z = min(a + step, n)
            want = rows[kidx[a:z]]
            if self.scatter:
                at = (dests[a:z, None] + ar[None, :]).reshape(-1)
                got = out[at].reshape(z - a, RW)
            else:
                got = out[a * slot:z * slot].view(z - a, slot)[:, :RW]
            if not torch.equal(got, want):
                bad = torch.nonzero((got != want).any(dim=1)).reshape(-1) + a
                f = int(bad[0])
                raise AssertionError(self.msg(f"{bad.numel()} frames' payload rows differ ({form}), first frame {f} at "
                                              f"payload offset {int(dests[f])} (2^32 {int(dests[f]) - MARK:+d})"))
            if self.scatter:
                out[at] = SENT
            else:
                out[a * slot:z * slot].view(z - a, slot)[:, :RW].fill_(SENT)


def _slot_sizes(seed, K, lo, hi, some=()):
    rng = np.random.default_rng(seed)
    s = rng.integers(lo, hi + 1, K)
    s[rng.choice(K, len(some), replace=False)] = some
    return s


def _straddling(name, claim, slot, K, hi, avg, seed):
    """i * slot across 2^32 with a slot that does not divide it: the frame
    whose slot holds byte 2^32 gets a payload that reaches it."""
    at = MARK // slot
    n = at + 4096
    sizes = _slot_sizes(seed, K, 0, hi, (slot, slot + 1))
    sizes[at % K] = hi
    return SlotCase(name, "i * slot_bytes", claim, slot, sizes, n=n, wire_claim=None if avg is None else n * avg,
                    seed=seed)


def _slot_cases():
    cs = []
    for dn, delta in DELTAS.items():
        # d_frame_index across 2^32 (the wire arena), one shape per kernel of slots_route
        cs += [SlotCase(f"slots_index_window256_{dn}", "d_frame_index", "deserialize_slots_window_kernel", 256,
                        _slot_sizes(11, 4100, 0, 250, (256, 257, 300, 5000)), wire_delta=delta, seed=11),
               SlotCase(f"slots_index_window4064_{dn}", "d_frame_index", "deserialize_slots_window_kernel", 4064,
                        _slot_sizes(12, 300, 0, 4064, (4064, 4065, 9000)), wire_delta=delta, seed=12),
               SlotCase(f"slots_index_piece16384_{dn}", "d_frame_index", "deserialize_slots_piece_kernel", 16384,
                        _slot_sizes(13, 64, 0, 16384, (16384, 16385, 20000)), wire_delta=delta, piece_loop="straight",
                        seed=13),
               # d_payload_off across 2^32 too (the payload arena)
               SlotCase(f"scatter_off_window256_{dn}", "d_payload_off", "deserialize_slots_window_kernel", 256,
                        _slot_sizes(14, 4100, 0, 250, (256, 257, 300)), wire_delta=delta, scatter=True, out_delta=delta,
                        seed=14),
               SlotCase(f"scatter_off_piece16384_{dn}", "d_payload_off", "deserialize_slots_piece_kernel", 16384,
                        _slot_sizes(15, 64, 0, 16384, (16384, 16385)), wire_delta=delta, scatter=True, out_delta=delta,
                        piece_loop="straight", seed=15)]
    # i * slot across 2^32: the index repeats K frames, so the wire stays small where the route allows
    mib = 1 << 20
    cs += [SlotCase("slots_dest_2gib_n5", "i * slot_bytes", "deserialize_slots_piece_kernel", 1 << 31,
                    [mib, 5000, 70000, 0, 1041], n=5, piece_loop="loop", seed=21),
           SlotCase("slots_dest_1mib16_loop", "i * slot_bytes", "deserialize_slots_piece_kernel", mib + 16,
                    [mib + 16, 5000, 0, 70000, 1041], n=4100, wire_claim=4100 * 1041, piece_loop="loop", seed=22),
           SlotCase("slots_dest_1mib16_straight", "i * slot_bytes", "deserialize_slots_piece_kernel", mib + 16,
                    [mib + 16, 5000, 0, 70000, 1041], n=4100, wire_claim=4100 * (mib + 16), piece_loop="straight",
                    seed=22),
           _straddling("slots_dest_window272", "deserialize_slots_window_kernel", 272, 4099, 272, 136, 23),
           _straddling("slots_dest_perframe2064", "deserialize_slots_kernel", 2064, 1021, 1000, None, 24)]
    return cs


# ---- cfws_index_frames_batch / cfws_h2_index_frames_batch ---------------------------

class IndexCase(WideCase):
    """d_begin / d_end across 2^32: carryover_util's 300 connections (none to
    200 frames each, errors, cuts) in a window of the 2^32 + 4 MiB receive
    arena."""
    operand = "d_begin / d_end"

    def __init__(self, name, delta, h2=False, with_info=True):
        super().__init__(name)
        self.delta, self.h2, self.with_info = delta, h2, with_info
        self.inner = CU.IndexCase(name, h2, with_info)

    def build(self):
        i, e = self.inner.inputs("B"), self.inner.expect("B")
        window = i["arena"]
        assert self.delta < len(window) <= WINDOW_MAX
        base = MARK - self.delta
        e_starts = (e["starts"].view(np.uint64) + np.uint64(base)).view(np.int64)
        return dict(window=window, base=base, begin=i["begin"] + base, end=i["end"] + base, starts=e_starts,
                    info=e["info"], first=e["first"], consumed=e["consumed"] + base, stop=e["stop"],
                    counts=e["counts"], total=e["total"], cross=crossing(i["begin"] + base, i["end"] - i["begin"]))

    def device_bytes(self):
        b = self.built()
        return ARENA_BYTES + 64 * self.inner.n + 24 * (b["total"] + 3) + self.inner.ws_bytes()

    def run(self):
        torch = _torch()
        b, n = self.built(), self.inner.n
        cap = b["total"] + 3
        buf = sentinel_arena(ARENA_BYTES)
        put(buf, b["base"], b["window"])
        starts = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
        info = torch.full((cap, 16), 0xFF, dtype=torch.uint8, device="cuda")
        first, consumed = (torch.full((n,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
        stop = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = torch.empty(self.inner.ws_bytes(), dtype=torch.uint8, device="cuda")
        kw = dict(starts_t=starts, ws_t=ws, first_t=first, consumed_t=consumed, stop_t=stop, total_t=total)
        begin, end = CU._up(b["begin"]), CU._up(b["end"])
        if self.h2:
            import h2_index_util as HU
            cfws.h2_index_frames_batch(buf, begin, end, 16384, HU.ALL, 0, info_t=info if self.with_info else None,
                                       with_info=self.with_info, **kw)
        else:
            cfws.index_frames_batch(buf, begin, end, **kw)
        torch.cuda.synchronize()
        assert int(total.item()) == b["total"], self.msg(f"total {int(total.item())} != {b['total']}")
        CU._eq(first, CU._up(b["first"]), self.msg("first"))
        CU._eq(consumed, CU._up(b["consumed"]), self.msg("consumed"))
        CU._eq(stop, CU._up(b["stop"]), self.msg("stop"))
        CU._eq(starts[:b["total"]], CU._up(b["starts"]), self.msg("starts"))
        CU._all(starts[b["total"]:], -1, self.msg("starts past the total"))
        if self.h2 and self.with_info:
            CU._eq(info[:b["total"]], CU._up(b["info"].view(np.uint8).reshape(-1, 16)), self.msg("info"))
            CU._all(info[b["total"]:], 0xFF, self.msg("info past the total"))
        else:
            CU._all(info, 0xFF, self.msg("info without d_info"))
        assert np.array_equal(get(buf, b["base"], len(b["window"])), b["window"]), self.msg("the window changed")
        buf[b["base"]:b["base"] + len(b["window"])].fill_(SENT)
        assert_all(buf, self.msg("receive arena"))
        _sync()


# ---- the send behind a ballast frame -------------------------------------------------

BALLAST_KEY = 0x9A3F17C5
SAMPLES = 64


def ballast_header(size: int, key: int | None, fin=1, opcode=2) -> bytes:
    """A frame header with the 64-bit length form, from the oracle's first two
    bytes (as tests/test_large.py builds its one)."""
    b0 = O.serialize_keyed(bool(fin), opcode, key is not None, key or 0, b"")[0]
    return bytes([b0, (0x80 if key is not None else 0) | 127]) + size.to_bytes(8, "big") + \
        (key.to_bytes(4, "little") if key is not None else b"")


def sample_offsets(size: int, seed: int) -> list:
    """The ballast windows that are compared: its first and last 64 KiB and 64
    drawn 4 KiB windows."""
    rng = np.random.default_rng(seed)
    return [(0, 65536), (size - 65536, 65536)] + [(int(o), 4096) for o in rng.integers(0, size - 4096, SAMPLES)]


def check_ballast(case, dst, dst_off, src, src_off, size, key, what):
    """dst[dst_off + k] == src[src_off + k] ^ key[k % 4] over the sampled windows."""
    for o, ln in sample_offsets(size, 7):
        got, s = get(dst, dst_off + o, ln), get(src, src_off + o, ln)
        kb = np.frombuffer(int(key).to_bytes(4, "little"), np.uint8)
        want = s ^ kb[(o + np.arange(ln)) % 4]
        assert np.array_equal(got, want), case.msg(f"{what}: the ballast frame's bytes at {o} differ")


SER_STYLES = {"mixed2500": (2500, None), "single_tiny": (CU.BIG_N, "tiny"), "single_inreg": (CU.BIG_N, "inreg")}
_ser_shared = {}


def ser_tail(style: str) -> dict:
    """The frames behind the ballast and the oracle's wire of them alone
    (shared by every case of the style)."""
    if style not in _ser_shared:
        n, send = SER_STYLES[style]
        if send is None:
            from test_gpu_fuzz import FUZZ_SIZES
            rng = np.random.default_rng(2500)
            sizes = rng.choice(FUZZ_SIZES, n).astype(np.uint64)
            d = CU._frames_desc(rng, sizes, rng.integers(0, CU.PAYLOAD_BYTES - 70000, n).astype(np.uint64))
        else:
            d = CU.send_desc(send, n, 4242)
        wire, e = O.serialize_batch(CU.payload_np(), d.view(O.DESC_DTYPE))
        _ser_shared[style] = dict(desc=d, wire=wire, e_desc=e)
    return _ser_shared[style]


class SerBallastCase(WideCase):
    """cfws_serialize_batch (pe: plan + execute): frame 0 ends delta bytes
    below 2^32 of the wire, the style's frames follow."""
    operand = "wire_off"

    def __init__(self, name, style, delta, pe):
        super().__init__(name)
        self.style, self.delta, self.pe = style, delta, pe
        self.n = SER_STYLES[style][0] + 1

    def build(self):
        t = ser_tail(self.style)
        shift = MARK - self.delta
        b0 = shift - 14
        d = np.zeros(self.n, dtype=cfws.DESC_DTYPE)
        d[0] = (0, 0, b0, BALLAST_KEY, 1, 2, 1, 0)
        d[1:] = t["desc"]
        e = d.copy()
        e[1:] = t["e_desc"].view(cfws.DESC_DTYPE)
        e["wire_off"][1:] += np.uint64(shift)
        e["header_size"][0] = 14
        total = shift + len(t["wire"])
        cap = W.round16(total) + 64
        ln = t["e_desc"]["payload_size"] + t["e_desc"]["header_size"].astype(np.uint64)
        return dict(desc=d, e_desc=e, shift=shift, b0=b0, total=total, cap=cap, tail=t["wire"],
                    cross=crossing(e["wire_off"][1:], ln))

    def single_pass(self) -> bool:
        k = CU.code_constants()
        return CU.blocks(self.n, k["plan_block"]) > k["self_scan_blocks"]

    def device_bytes(self):
        b = self.built()
        return MARK + (8 << 20) + b["cap"] + 4096 + 64 * self.n + cfws.lib().cfws_workspace_size(self.n, b["cap"]) + \
            len(b["tail"])

    def run(self):
        torch = _torch()
        b, n = self.built(), self.n
        # the ballast reads whatever the payload arena holds; the frames behind it read its first 4 MiB
        payload = torch.empty(MARK + (8 << 20), dtype=torch.uint8, device="cuda")
        put(payload, 0, CU.payload_np())
        before = checksum(payload)
        wire = sentinel_arena(b["cap"] + 4096)
        d_in = b["desc"].copy()
        d_in["wire_off"], d_in["header_size"] = 0x5A5A5A5A5A5A5A5A, CU.DESC_POISON
        d_t = CU._up(CU._desc_bytes(d_in))
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = cfws.workspace(n, b["cap"])
        if self.pe:
            cfws.serialize_plan(d_t, b["cap"], tot, ws)
            cfws.serialize_execute(payload, d_t, wire[:b["cap"]], ws, b["cap"])
        else:
            cfws.serialize(payload, d_t, wire[:b["cap"]], ws, tot)
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(d_t, CU._up(CU._desc_bytes(b["e_desc"])), self.msg("descriptors"))
        assert get(wire, 0, 14).tobytes() == ballast_header(b["b0"], BALLAST_KEY), self.msg("the ballast's header")
        check_ballast(self, wire, 14, payload, 0, b["b0"], BALLAST_KEY, "wire")
        CU._eq(wire[b["shift"]:b["total"]], CU._up(b["tail"]), self.msg("the wire behind the ballast"))
        CU._all(wire[b["total"]:W.round16(b["total"])], 0, self.msg("bytes up to round16(total)"))
        assert_all(wire, self.msg("wire arena past the total"), lo=W.round16(b["total"]))
        assert checksum(payload) == before, self.msg("the payload arena changed")
        _sync()


# ---- the relay behind a ballast frame -------------------------------------------------

RELAY_FORMS = {"unmask": (True, 0), "mask": (False, 1), "remask": (True, 1)}   # (incoming masked, out_mask)


class RelayBallastCase(WideCase):
    """cfws_relay_batch: frame 0's outgoing frame ends delta bytes below 2^32
    of the outgoing wire; 3,000 frames follow."""
    operand = "outgoing payload_off"

    def __init__(self, name, form, policy, delta, n=3000):
        super().__init__(name)
        self.form, self.policy, self.delta, self.n = form, policy, delta, n + 1

    def build(self):
        in_masked, out_mask = RELAY_FORMS[self.form]
        n = self.n - 1
        rng = np.random.default_rng(self.delta + len(self.form))
        sizes = rng.integers(0, 1501, n)
        ops = rng.choice([0, 1, 2, 8, 9, 10], n)
        sizes[ops >= 8] = np.minimum(sizes[ops >= 8], 125)
        wire, starts = RU.frames_wire(sizes, np.full(n, in_masked), rng.random(n) < .7, ops, 99,
                                      [int(i) for i in range(3, n, 96)])
        keys = (O.splitmix_words(0x99, 0, self.n) >> np.uint64(7)).astype(np.uint32)
        wsize = len(wire) - 1                                          # the last frame MORE_DATA
        out, offs, desc, status = RU.expect_relay(wire, wsize, starts, self.policy, out_mask, keys[1:])
        in_h, out_h = (14 if in_masked else 10), (14 if out_mask else 10)
        out_base = MARK - self.delta
        b0 = out_base - out_h
        in_base = in_h + b0
        e = np.zeros(self.n, dtype=cfws.DESC_DTYPE)
        e[0] = (0, 0, b0, BALLAST_KEY if in_masked else 0, 1, 2, 1 if in_masked else 0, in_h)
        e[1:] = desc.view(cfws.DESC_DTYPE)
        e["payload_off"][1:] += np.uint64(out_base)
        e["wire_off"][1:] += np.uint64(in_base)
        e_st = np.concatenate([[0], status]).astype(np.int32)
        index = np.concatenate([[0], starts + np.uint64(in_base)]).astype(np.uint64)
        total = out_base + len(out)
        nbytes = np.diff(np.concatenate([offs, [len(out)]]).astype(np.int64))
        return dict(wire=wire, in_base=in_base, wire_size=in_base + wsize, index=index, keys=keys, out=out,
                    out_base=out_base, b0=b0, in_h=in_h, out_h=out_h, desc=e, status=e_st, total=total,
                    cap=W.round16(total) + 64, in_masked=in_masked, out_mask=out_mask,
                    cross=crossing(e["payload_off"][1:], nbytes))

    def device_bytes(self):
        b = self.built()
        return W.round16(b["wire_size"]) + 32 + b["cap"] + 4096 + 48 * self.n + \
            cfws.lib().cfws_relay_workspace_size(self.n, b["cap"])

    def run(self):
        torch = _torch()
        b, n = self.built(), self.n
        win = torch.empty(W.round16(b["wire_size"]) + 32, dtype=torch.uint8, device="cuda")
        put(win, 0, np.frombuffer(ballast_header(b["b0"], BALLAST_KEY if b["in_masked"] else None), np.uint8))
        put(win, b["in_base"], b["wire"])
        before = checksum(win)
        out = sentinel_arena(b["cap"] + 4096)
        keys = CU._up(b["keys"].view(np.int32))
        d_t = torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
        st_t = torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = cfws.relay_workspace(n, b["cap"])
        cfws.relay(win, b["wire_size"], _idx_t(b["index"]), out[:b["cap"]], self.policy, b["out_mask"],
                   keys if b["out_mask"] else None, d_t, st_t, ws, tot, max_payload=BIG_PAYLOAD, out_capacity=b["cap"])
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(st_t, CU._up(b["status"]), self.msg("statuses"))
        CU._eq(d_t, CU._up(CU._desc_bytes(b["desc"])), self.msg("descriptors"))
        kout = int(b["keys"][0]) if b["out_mask"] else None
        assert get(out, 0, b["out_h"]).tobytes() == ballast_header(b["b0"], kout), self.msg("the ballast's header")
        kx = (BALLAST_KEY if b["in_masked"] else 0) ^ (kout or 0)
        check_ballast(self, out, b["out_h"], win, b["in_h"], b["b0"], kx, "outgoing wire")
        CU._eq(out[b["out_base"]:b["total"]], CU._up(b["out"]), self.msg("the outgoing wire behind the ballast"))
        assert_all(out, self.msg("outgoing wire arena past the total"), lo=W.round16(b["total"]))
        assert checksum(win) == before, self.msg("the incoming wire changed")
        _sync()


# ---- the fused receive: payload_off across 2^32 without a ballast ---------------------

class FusedCase(WideCase):
    """cfws_deserialize_batch, one call, fused route: 2^20 + 4,096 frames of
    0-100 B at align = 4096 (a ballast would lift the average frame over the
    fused route's 512 B). The oracle runs on the frames from 64 before the
    crossing on; its offsets are shifted by the 4 KiB slots before them."""
    operand = "payload_off (fused route)"
    claim = "deserialize_plan_single_kernel<true>"
    N, ALIGN, BACK = (1 << 20) + 4096, 4096, 64

    def build(self):
        n, A = self.N, self.ALIGN
        rng = np.random.default_rng(4096)
        sizes = rng.integers(1, 101, n).astype(np.uint64)
        sizes[rng.choice(n, 500, replace=False)] = 0
        d = CU._frames_desc(rng, sizes, rng.integers(0, CU.PAYLOAD_BYTES - 70000, n).astype(np.uint64), opcodes=(0, 1, 2))
        wire, d = O.serialize_batch(CU.payload_np(), d.view(O.DESC_DTYPE))
        wsize = W.round16(len(wire)) + 16
        buf = np.zeros(wsize + 16, np.uint8)
        buf[:len(wire)] = wire
        index = d["wire_off"].astype(np.uint64)
        bad = np.arange(3, n, 2048)
        buf[index[bad].astype(np.int64)] |= 0x40
        index[np.arange(7, n, 200_000)] = wsize - 1                      # MORE_DATA
        p_d, p_st = O.parse_headers(buf[:wsize], index)
        slots = np.where((p_st == O.PARSE_COMPLETE) & (p_d["payload_size"] > 0), A, 0).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.uint64)
        total = int(slots.sum())
        c = int(np.nonzero(offs + slots > MARK)[0][0])
        t0 = c - self.BACK
        shift = int(offs[t0])
        t_out, t_d, t_st, t_tot = O.deserialize_batch(buf[:wsize], index[t0:], align=A, capacity=total - shift + 64)
        assert t_tot == total - shift and np.array_equal(t_st, p_st[t0:])
        t_d = t_d.copy()
        t_d["payload_off"] += np.uint64(shift)
        # the frames below the tail: the oracle at align = 128 lays out the same
        # payloads 128 B apart, and reports the other descriptor fields alike
        l_out, l_d, l_st, l_tot = O.deserialize_batch(buf[:wsize], index[:t0], align=128, capacity=128 * t0 + 64)
        assert np.array_equal(l_st, p_st[:t0]) and l_tot * (A // 128) == shift
        e = np.concatenate([l_d, t_d])
        e["payload_off"] = offs                                         # the tail's: the oracle's own, shifted
        assert np.array_equal(e[t0:], t_d)
        return dict(wire=buf, wsize=wsize, index=index, desc=e, status=p_st, tail_desc=t_d, t0=t0, shift=shift,
                    tail_out=t_out[:t_tot], low_out=l_out[:l_tot], total=total, cap=W.round16(total) + 64,
                    cross=crossing(offs, np.where(slots > 0, p_d["payload_size"], 0)))

    def route(self):
        b = self.built()
        return cfws.lib().cfws_deserialize_pass_kernel(self.N, b["wsize"], self.ALIGN, 0, b["cap"]).decode()

    def device_bytes(self):
        b = self.built()
        return b["cap"] + 4096 + 2 * len(b["wire"]) + 2 * 44 * self.N + len(b["tail_out"]) + len(b["low_out"]) + \
            cfws.lib().cfws_workspace_size(self.N, b["cap"])

    def run(self):
        torch = _torch()
        b, n = self.built(), self.N
        wire, keep = CU._up(b["wire"]), CU._up(b["wire"])
        out = sentinel_arena(b["cap"] + 4096)
        d_t = torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
        st_t = torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = cfws.workspace(n, b["cap"])
        cfws.deserialize(wire, b["wsize"], _idx_t(b["index"]), out[:b["cap"]], d_t, st_t, ws, tot, align=self.ALIGN)
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(st_t, CU._up(b["status"]), self.msg("statuses"))
        CU._eq(d_t[b["t0"]:], CU._up(CU._desc_bytes(b["tail_desc"])), self.msg("descriptors from 64 before the crossing on"))
        CU._eq(d_t, CU._up(CU._desc_bytes(b["desc"])), self.msg("descriptors"))
        CU._eq(out[b["shift"]:b["total"]], CU._up(b["tail_out"]), self.msg("payload arena from 64 before the crossing on"))
        low = out[:b["shift"]].view(-1, self.ALIGN)
        CU._eq(low[:, :128].contiguous(), CU._up(b["low_out"]), self.msg("payload arena below the crossing"))
        CU._all(low[:, 128:], 0, self.msg("slot padding below the crossing"))
        assert_all(out, self.msg("payload arena past the total"), lo=b["total"])
        assert torch.equal(wire, keep), self.msg("the wire changed")
        _sync()


# ---- offsets the caller supplies, relocated: the batch receive, the batch send, the relay ----

def _window(arena, base, data):
    """The window's bytes are unchanged; then blanked for the whole-arena check."""
    ok = np.array_equal(get(arena, base, len(data)), data)
    arena[base:base + len(data)].fill_(SENT)
    return ok


def last_chunk_end(total: int, flags: int) -> int:
    """Where a receive's writes end at the latest (all below the capacity): a
    pass writes whole 16-byte chunks, so up to round16(total); the control
    pass of a reassembly starts at the data pass's total, which need not be a
    multiple of 16, and its last chunk may end up to 16 bytes later."""
    return W.round16(total) + (16 if flags else 0)


class DeRelocCase(WideCase):
    """cfws_deserialize_batch (pe: plan + execute) with d_frame_index across
    2^32: K frames in a window of the wire arena, n >= K index entries that
    repeat them (any index is a frame start to the library), with INVALID,
    DATA_TOO_BIG and MORE_DATA frames and an index at wire_size - 1."""
    operand = "d_frame_index"
    MAXP = 1000

    def __init__(self, name, claim, n, K, hi, align, flags, pe, delta):
        super().__init__(name)
        self.claim, self.n, self.K, self.hi, self.align, self.flags, self.pe, self.delta = \
            claim, n, K, hi, align, flags, pe, delta

    def build(self):
        n, K = self.n, self.K
        rng = np.random.default_rng(K + self.hi)
        sizes = rng.integers(0, self.hi + 1, K).astype(np.uint64)
        d = CU._frames_desc(rng, sizes, rng.integers(0, CU.PAYLOAD_BYTES - 70000, K).astype(np.uint64),
                            opcodes=(0, 1, 2))
        if self.flags:
            ctl = rng.random(K) < 0.2
            d["opcode"][ctl] = rng.choice([8, 9, 10], int(ctl.sum())).astype(np.uint8)
            d["fin"][ctl] = 1
            d["payload_size"][ctl] = np.minimum(d["payload_size"][ctl], 125)
        wire, d = O.serialize_batch(CU.payload_np(), d.view(O.DESC_DTYPE))
        wire = wire.copy()
        assert self.delta < len(wire) <= WINDOW_MAX
        starts = d["wire_off"].astype(np.uint64)
        wire[starts[np.arange(3, K, 96)].astype(np.int64)] |= 0x40
        wsize = len(wire) - 1
        rel = starts[np.arange(n) % K]
        rel[np.arange(7, n, 192)] = wsize - 1
        base = MARK - self.delta
        whole = O.deserialize_batch(wire[:wsize], rel, align=self.align, max_payload=self.MAXP,
                                    capacity=len(wire) * (n // K + 1) + self.align * n + 64, flags=self.flags)[3]
        cap = W.round16(whole) + 64
        out, e, st, tot = O.deserialize_batch(wire[:wsize], rel, align=self.align, max_payload=self.MAXP, capacity=cap,
                                              flags=self.flags)
        e = e.copy()
        e["wire_off"] += np.uint64(base)
        ln = (d["payload_size"] + d["header_size"].astype(np.uint64))
        return dict(wire=wire, wsize=wsize, base=base, wire_size=base + wsize, rel=rel, index=rel + np.uint64(base),
                    desc=e, status=st, total=tot, out=out[:tot], cap=cap, cross=crossing(starts + np.uint64(base), ln))

    def route(self):
        b = self.built()
        return cfws.lib().cfws_deserialize_pass_kernel(self.n, b["wire_size"], self.align, self.flags, b["cap"]).decode()

    def device_bytes(self):
        b = self.built()
        return ARENA_BYTES + 2 * (b["cap"] + 4096) + 2 * 44 * self.n + cfws.lib().cfws_workspace_size(self.n, b["cap"])

    def run(self):
        torch = _torch()
        b, n = self.built(), self.n
        wire = sentinel_arena(ARENA_BYTES)
        put(wire, b["base"], b["wire"])
        out = sentinel_arena(b["cap"] + 4096)
        idx = _idx_t(b["index"])
        d_t = torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
        st_t = torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = cfws.workspace(n, b["cap"])
        if self.pe:
            cfws.deserialize_plan(wire, b["wire_size"], idx, d_t, st_t, b["cap"], tot, ws, max_payload=self.MAXP,
                                  align=self.align, flags=self.flags)
            cfws.deserialize_execute(wire, d_t, st_t, out[:b["cap"]], ws, b["cap"], flags=self.flags)
        else:
            cfws.deserialize(wire, b["wire_size"], idx, out[:b["cap"]], d_t, st_t, ws, tot, max_payload=self.MAXP,
                             align=self.align, flags=self.flags)
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(st_t, CU._up(b["status"]), self.msg("statuses"))
        CU._eq(d_t, CU._up(CU._desc_bytes(b["desc"])), self.msg("descriptors"))
        CU._eq(out[:b["total"]], CU._up(b["out"]), self.msg("payload arena"))
        assert_all(out, self.msg("payload arena past the pass's last chunk"), lo=last_chunk_end(b["total"], self.flags))
        assert _window(wire, b["base"], b["wire"]), self.msg("the wire window changed")
        assert_all(wire, self.msg("wire arena"))
        _sync()


class SerRelocCase(WideCase):
    """cfws_serialize_batch (pe: plan + execute) with desc.payload_off across
    2^32: carryover_util's send shapes, their 4 MiB of payload in a window of
    the payload arena."""
    operand = "desc.payload_off"

    def __init__(self, name, n, style, pe, delta, small=False):
        super().__init__(name)
        self.n, self.style, self.pe, self.delta, self.small = n, style, pe, delta, small

    def build(self):
        d = CU.send_desc(self.style, self.n, 777)
        aligned = CU.SEND_STYLES.get(self.style, (0, 0, "any"))[2] == "aligned"
        # one frame of at least two bytes starts below the mark and ends above it
        f = int(np.nonzero(d["payload_size"] >= (32 if aligned else 2))[0][0])
        d["payload_off"][f] = self.delta - (16 if aligned else 1)
        wire, e = O.serialize_batch(CU.payload_np(), d.view(O.DESC_DTYPE))
        base = MARK - self.delta
        e = e.copy().view(cfws.DESC_DTYPE)
        e["payload_off"] += np.uint64(base)
        d_in = d.copy()
        d_in["payload_off"] += np.uint64(base)
        cap = (4 << 20) if self.small else W.round16(len(wire)) + 64
        assert len(wire) <= cap and base + CU.PAYLOAD_BYTES <= ARENA_BYTES
        return dict(desc=d, d_in=d_in, e_desc=e, wire=wire, base=base, cap=cap, total=len(wire),
                    cross=crossing(d_in["payload_off"], d["payload_size"]))

    def device_bytes(self):
        b = self.built()
        return ARENA_BYTES + 2 * (b["cap"] + 4096) + 64 * self.n + cfws.lib().cfws_workspace_size(self.n, b["cap"])

    def run(self):
        torch = _torch()
        b, n = self.built(), self.n
        payload = sentinel_arena(ARENA_BYTES)
        put(payload, b["base"], CU.payload_np())
        wire = sentinel_arena(b["cap"] + 4096)
        d_in = b["d_in"].copy()
        d_in["wire_off"], d_in["header_size"] = 0x5A5A5A5A5A5A5A5A, CU.DESC_POISON
        d_t = CU._up(CU._desc_bytes(d_in))
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = cfws.workspace(n, b["cap"])
        if self.pe:
            cfws.serialize_plan(d_t, b["cap"], tot, ws)
            cfws.serialize_execute(payload, d_t, wire[:b["cap"]], ws, b["cap"])
        else:
            cfws.serialize(payload, d_t, wire[:b["cap"]], ws, tot)
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(d_t, CU._up(CU._desc_bytes(b["e_desc"])), self.msg("descriptors"))
        CU._eq(wire[:b["total"]], CU._up(b["wire"]), self.msg("wire"))
        CU._all(wire[b["total"]:W.round16(b["total"])], 0, self.msg("bytes up to round16(total)"))
        assert_all(wire, self.msg("wire arena past the total"), lo=W.round16(b["total"]))
        assert _window(payload, b["base"], CU.payload_np()), self.msg("the payload window changed")
        assert_all(payload, self.msg("payload arena"))
        _sync()


class RelayRelocCase(WideCase):
    """cfws_relay_batch with d_frame_index across 2^32: 3,000 frames in a
    window of the incoming wire arena, indexed in reverse order and, past
    3,000 entries, again and again."""
    operand = "d_frame_index"
    K = 3000

    def __init__(self, name, n, policy, out_mask, delta):
        super().__init__(name)
        self.n, self.policy, self.out_mask, self.delta = n, policy, out_mask, delta

    def build(self):
        n, K = self.n, self.K
        rng = np.random.default_rng(n)
        sizes = rng.integers(0, 401, K)
        ops = rng.choice([0, 1, 2, 8, 9, 10], K)
        sizes[ops >= 8] = np.minimum(sizes[ops >= 8], 125)
        wire, starts = RU.frames_wire(sizes, rng.random(K) < .6, rng.random(K) < .7, ops, 55,
                                      [int(i) for i in range(3, K, 96)])
        assert self.delta < len(wire) <= WINDOW_MAX
        wsize = len(wire) - 1
        rel = starts[::-1][np.arange(n) % K].copy()
        keys = (O.splitmix_words(0x77, 0, n) >> np.uint64(7)).astype(np.uint32)
        out, offs, desc, status = RU.expect_relay(wire, wsize, rel, self.policy, self.out_mask, keys)
        base = MARK - self.delta
        e = desc.copy().view(cfws.DESC_DTYPE)
        e["wire_off"] += np.uint64(base)
        p_d, p_st = O.parse_headers(wire[:wsize], starts)
        ln = np.where(np.isin(p_st, (0,)), p_d["payload_size"] + p_d["header_size"].astype(np.uint64), 0)
        return dict(wire=wire, wsize=wsize, base=base, wire_size=base + wsize, rel=rel, index=rel + np.uint64(base),
                    keys=keys, out=out, desc=e, status=status, total=len(out), cap=W.round16(len(out)) + 64,
                    cross=crossing(starts + np.uint64(base), ln))

    def device_bytes(self):
        b = self.built()
        return ARENA_BYTES + 2 * (b["cap"] + 4096) + 2 * 48 * self.n + cfws.lib().cfws_relay_workspace_size(self.n, b["cap"])

    def run(self):
        torch = _torch()
        b, n = self.built(), self.n
        win = sentinel_arena(ARENA_BYTES)
        put(win, b["base"], b["wire"])
        out = sentinel_arena(b["cap"] + 4096)
        keys = CU._up(b["keys"].view(np.int32))
        d_t = torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
        st_t = torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = cfws.relay_workspace(n, b["cap"])
        cfws.relay(win, b["wire_size"], _idx_t(b["index"]), out[:b["cap"]], self.policy, self.out_mask,
                   keys if self.out_mask else None, d_t, st_t, ws, tot, out_capacity=b["cap"])
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(st_t, CU._up(b["status"]), self.msg("statuses"))
        CU._eq(d_t, CU._up(CU._desc_bytes(b["desc"])), self.msg("descriptors"))
        CU._eq(out[:b["total"]], CU._up(b["out"]), self.msg("outgoing wire"))
        assert_all(out, self.msg("outgoing wire arena past the total"), lo=W.round16(b["total"]))
        assert _window(win, b["base"], b["wire"]), self.msg("the incoming window changed")
        assert_all(win, self.msg("incoming wire arena"))
        _sync()


# ---- the split ops, relocated ----------------------------------------------------------

SPLIT_PAY_DELTAS = {"page": 16 * 4096, "odd16": 16 * 4097}        # the chain's payload is 128 KiB


class SplitSendCase(WideCase):
    """cfws_encode_headers + cfws_mask_batch (packed: _packed over
    test_mask_packed_boundary_classes' chain, else scattered frames with
    gaps): wire_off across 2^32 of the wire arena, payload_off across 2^32 of
    the payload arena. The chain's wire is 2.2 MiB: every boundary class once."""
    operand = "wire_off / payload_off"

    def __init__(self, name, packed, dn):
        super().__init__(name)
        self.packed, self.delta, self.pdelta = packed, DELTAS[dn], SPLIT_PAY_DELTAS[dn]

    def build(self):
        import random

        import test_split_ops as S
        rng = random.Random(61)
        payload = O.fill_splitmix(1 << 17, 61)
        if self.packed:
            d, total, _ = S.boundary_class_chain(rng, len(payload))
        else:
            d = S.random_frames(rng, 500, len(payload), sizes=[0, 1, 15, 16, 17, 125, 126, 127, 1000, 4097, 20000])
            d["wire_off"], total = S.scattered_wire_offsets(rng, d)
        wlen = total + 21
        assert self.delta < wlen <= ARENA_BYTES - MARK and self.pdelta < len(payload)
        exp = np.full(wlen, SENT, np.uint8)
        e = O.encode_headers(d, exp, wlen)
        O.mask_batch(payload, e, exp, wlen)
        wbase, pbase = MARK - self.delta, MARK - self.pdelta
        d_in, e = d.copy(), e.copy()
        for x in (d_in, e):
            x["wire_off"] += np.uint64(wbase)
            x["payload_off"] += np.uint64(pbase)
        ln = e["payload_size"] + e["header_size"].astype(np.uint64)
        return dict(payload=payload, desc=d, d_in=d_in, e_desc=e, exp=exp, wlen=wlen, wbase=wbase, pbase=pbase,
                    cross=crossing(e["wire_off"], ln), pcross=crossing(e["payload_off"], e["payload_size"]))

    def device_bytes(self):
        return 2 * ARENA_BYTES + (1 << 24)

    def run(self):
        torch = _torch()
        b = self.built()
        pay = sentinel_arena(ARENA_BYTES)
        put(pay, b["pbase"], b["payload"])
        wire = sentinel_arena(ARENA_BYTES)
        d_in = b["d_in"].copy()
        d_in["header_size"] = CU.DESC_POISON
        d_t = CU._up(CU._desc_bytes(d_in))
        cap = b["wbase"] + b["wlen"]
        cfws.encode_headers(d_t, wire, cap)
        cfws.mask_batch(pay, d_t, wire, int(b["desc"]["payload_size"].max()), cap, packed=self.packed)
        torch.cuda.synchronize()
        CU._eq(d_t, CU._up(CU._desc_bytes(b["e_desc"])), self.msg("descriptors"))
        CU._eq(wire[b["wbase"]:cap], CU._up(b["exp"]), self.msg("wire window"))
        wire[b["wbase"]:cap].fill_(SENT)
        assert_all(wire, self.msg("wire arena"))
        assert _window(pay, b["pbase"], b["payload"]), self.msg("the payload window changed")
        assert_all(pay, self.msg("payload arena"))
        _sync()


class SplitRecvCase(WideCase):
    """cfws_parse_headers + cfws_unmask_batch: the index and wire_off across
    2^32 of the wire arena, payload_off (scattered, any alignment, with gaps)
    across 2^32 of the payload arena."""
    operand = "d_frame_index / wire_off / payload_off"

    def __init__(self, name, dn):
        super().__init__(name)
        self.delta = DELTAS[dn]

    def build(self):
        import random

        import test_split_ops as S
        rng = random.Random(71)
        payload = O.fill_splitmix(400000, 71)
        desc = S.random_frames(rng, 450, len(payload), sizes=[0, 1, 5, 16, 33, 125, 126, 127, 1000, 4097, 20000])
        # the frame that holds byte 2^32 is a valid one
        held = int(np.searchsorted(W.wire_layout(desc.view(cfws.DESC_DTYPE))[0], self.delta, side="right")) - 1
        desc["opcode"][held] = 2
        wire, d_exp = O.serialize_batch(payload, desc)
        wire = wire.copy()
        assert self.delta < len(wire) <= WINDOW_MAX
        starts = d_exp["wire_off"].astype(np.uint64)
        for i in rng.sample([i for i in range(len(desc)) if i != held], 20):
            wire[int(starts[i])] |= 0x20
        wsize = len(wire) - 1
        starts = np.concatenate([starts, np.array([wsize - 1, wsize, wsize + 9, int(starts[7]) + 1], np.uint64)])
        pd, st = O.parse_headers(wire, starts, wire_size=wsize)
        off, rel = rng.randrange(16), np.zeros(len(pd), np.uint64)
        for i in range(len(pd)):
            rel[i] = off
            end = off + (int(pd[i]["payload_size"]) if st[i] == 0 else 0)
            gap = rng.randrange(0, 24)
            off = end if end <= self.delta < end + gap else end + gap      # byte 2^32 lies in a payload, not in a gap
        plen = off + 32
        assert self.delta < plen <= WINDOW_MAX
        un = pd.copy()
        un["payload_off"] = rel
        out = np.full(plen, SENT, np.uint8)
        O.unmask_batch(wire, un, st, out, plen)
        wbase, obase = MARK - self.delta, MARK - self.delta
        e = un.copy()
        e["wire_off"] += np.uint64(wbase)
        e["payload_off"] += np.uint64(obase)
        ok = st == O.PARSE_COMPLETE
        return dict(wire=wire, wsize=wsize, wbase=wbase, obase=obase, starts=starts, index=starts + np.uint64(wbase),
                    parsed=pd, desc=e, status=st, out=out, plen=plen,
                    cross=crossing(e["wire_off"], (pd["payload_size"] + pd["header_size"].astype(np.uint64)) * ok),
                    pcross=crossing(e["payload_off"], pd["payload_size"] * ok))

    def device_bytes(self):
        return 2 * ARENA_BYTES + (1 << 24)

    def run(self):
        torch = _torch()
        b = self.built()
        n = len(b["starts"])
        wire = sentinel_arena(ARENA_BYTES)
        put(wire, b["wbase"], b["wire"])
        out = sentinel_arena(ARENA_BYTES)
        d_t = torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
        st_t = torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda")
        cfws.parse_headers(wire, b["wbase"] + b["wsize"], _idx_t(b["index"]), d_t, st_t)
        torch.cuda.synchronize()
        CU._eq(st_t, CU._up(b["status"]), self.msg("statuses"))
        got = cfws.desc_from_device(d_t)
        for f in ("wire_off", "payload_size", "mask_key", "fin", "opcode", "mask", "header_size"):
            assert np.array_equal(got[f], b["desc"][f]), self.msg(f"parse_headers {f}")
        d_t = CU._up(CU._desc_bytes(b["desc"]))
        cap = b["obase"] + b["plen"]
        cfws.unmask_batch(wire, d_t, st_t, out, int(b["parsed"]["payload_size"].max()), cap)
        torch.cuda.synchronize()
        CU._eq(out[b["obase"]:cap], CU._up(b["out"]), self.msg("payload window"))
        out[b["obase"]:cap].fill_(SENT)
        assert_all(out, self.msg("payload arena"))
        assert _window(wire, b["wbase"], b["wire"]), self.msg("the wire window changed")
        assert_all(wire, self.msg("wire arena"))
        _sync()


def _reloc_cases():
    cs = []
    R = cfws.DESERIALIZE_REASSEMBLE
    for dn, delta in DELTAS.items():
        cs.append(DeRelocCase(f"de_index_small_{dn}", "deserialize_small_kernel", 1000, 1000, 1500, 16, 0, False, delta))
        for pe in (False, True):
            s = ("_pe" if pe else "") + "_" + dn
            cs += [DeRelocCase("de_index_plan3000" + s, "xform_kernel<1>", 3000, 3000, 1200, 1, 0, pe, delta),
                   DeRelocCase("de_index_reasm3000" + s, "xform_kernel<1>", 3000, 3000, 1200, 16, R, pe, delta),
                   DeRelocCase("de_index_single" + s, "xform_kernel<1>", CU.BIG_N, 3000, 1200, 1, 0, pe, delta)]
        cs.append(SerRelocCase(f"ser_off_small_{dn}", 1000, "small_lo", False, delta, small=True))
        for pe in (False, True):
            s = ("_pe" if pe else "") + "_" + dn
            cs += [SerRelocCase("ser_off_mixed" + s, 3000, "mixed", pe, delta),
                   SerRelocCase("ser_off_single_tiny" + s, CU.BIG_N, "tiny", pe, delta),
                   SerRelocCase("ser_off_single_inreg" + s, CU.BIG_N, "inreg_small", pe, delta)]
        cs += [RelayRelocCase(f"relay_index_3000_{dn}", 3000, RU.ECHO_SERVER, 1, delta),
               RelayRelocCase(f"relay_index_big_{dn}", CU.BIG_N, RU.VERBATIM, 0, delta)]
        cs += [SplitSendCase(f"split_send_packed_{dn}", True, dn), SplitSendCase(f"split_send_scattered_{dn}", False, dn),
               SplitRecvCase(f"split_recv_{dn}", dn)]
    return cs


# ---- the receive behind a ballast frame ------------------------------------------------

class DeBallastCase(WideCase):
    """cfws_deserialize_batch (pe: plan + execute): frame 0's payload ends
    delta bytes below 2^32 of the payload arena (only its 14-byte header is
    written in front of whatever the wire arena holds), the frames under test
    follow it; with REASSEMBLE, control frames lie on both sides of the mark."""
    operand = "payload_off"
    claim = "xform_kernel<1>"

    def __init__(self, name, n, hi, align, flags, pe, delta):
        super().__init__(name)
        self.n, self.hi, self.align, self.flags, self.pe, self.delta = n + 1, hi, align, flags, pe, delta

    def build(self):
        n = self.n - 1
        rng = np.random.default_rng(n + self.hi + self.flags)
        sizes = rng.integers(0, self.hi + 1, n).astype(np.uint64)
        d = CU._frames_desc(rng, sizes, rng.integers(0, CU.PAYLOAD_BYTES - 70000, n).astype(np.uint64), opcodes=(0, 1, 2))
        if self.flags:
            ctl = rng.random(n) < 0.6          # the mark falls among the control frames' payloads
            d["opcode"][ctl] = rng.choice([8, 9, 10], int(ctl.sum())).astype(np.uint8)
            d["fin"][ctl] = 1
            d["payload_size"][ctl] = np.minimum(d["payload_size"][ctl], 125)
        wire, d = O.serialize_batch(CU.payload_np(), d.view(O.DESC_DTYPE))
        wire = wire.copy()
        starts = d["wire_off"].astype(np.uint64)
        wire[starts[np.arange(3, n, 96)].astype(np.int64)] |= 0x40
        wsize = len(wire) - 1
        starts[np.arange(7, n, 192)] = wsize - 1
        whole = O.deserialize_batch(wire[:wsize], starts, align=self.align, capacity=len(wire) + self.align * n + 64,
                                    flags=self.flags)[3]
        out, e_t, st, tot = O.deserialize_batch(wire[:wsize], starts, align=self.align, capacity=W.round16(whole) + 64,
                                                flags=self.flags)
        assert tot == whole
        b0 = MARK - self.delta                                         # a multiple of 16: the ballast's slot is its size
        in_base = 14 + b0
        e = np.zeros(self.n, dtype=cfws.DESC_DTYPE)
        e[0] = (0, 0, b0, BALLAST_KEY, 1, 2, 1, 14)
        e[1:] = e_t
        e["payload_off"][1:] += np.uint64(b0)
        e["wire_off"][1:] += np.uint64(in_base)
        plen = np.where(st == O.PARSE_COMPLETE, e_t["payload_size"], 0)
        ctl = e_t["opcode"] >= 8
        return dict(wire=wire, in_base=in_base, wire_size=in_base + wsize, index=np.concatenate([[0], starts + np.uint64(in_base)]),
                    b0=b0, desc=e, status=np.concatenate([[0], st]).astype(np.int32), tail=e_t, out=out[:tot],
                    total=b0 + tot, cap=W.round16(b0 + tot) + 64, cross=crossing(e["payload_off"][1:], plen),
                    ctl_cross=crossing(e["payload_off"][1:][ctl], plen[ctl]))

    def route(self):
        b = self.built()
        return cfws.lib().cfws_deserialize_pass_kernel(self.n, b["wire_size"], self.align, self.flags, b["cap"]).decode()

    def device_bytes(self):
        b = self.built()
        return W.round16(b["wire_size"]) + 32 + b["cap"] + 4096 + 2 * 44 * self.n + len(b["out"]) + \
            cfws.lib().cfws_workspace_size(self.n, b["cap"])

    def run(self):
        torch = _torch()
        b, n = self.built(), self.n
        wire = torch.empty(W.round16(b["wire_size"]) + 32, dtype=torch.uint8, device="cuda")
        put(wire, 0, np.frombuffer(ballast_header(b["b0"], BALLAST_KEY), np.uint8))
        put(wire, b["in_base"], b["wire"])
        before = checksum(wire)
        out = sentinel_arena(b["cap"] + 4096)
        idx = _idx_t(b["index"])
        d_t = torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
        st_t = torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ws = cfws.workspace(n, b["cap"])
        if self.pe:
            cfws.deserialize_plan(wire, b["wire_size"], idx, d_t, st_t, b["cap"], tot, ws, max_payload=BIG_PAYLOAD,
                                  align=self.align, flags=self.flags)
            cfws.deserialize_execute(wire, d_t, st_t, out[:b["cap"]], ws, b["cap"], flags=self.flags)
        else:
            cfws.deserialize(wire, b["wire_size"], idx, out[:b["cap"]], d_t, st_t, ws, tot, max_payload=BIG_PAYLOAD,
                             align=self.align, flags=self.flags)
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(st_t, CU._up(b["status"]), self.msg("statuses"))
        CU._eq(d_t, CU._up(CU._desc_bytes(b["desc"])), self.msg("descriptors"))
        check_ballast(self, out, 0, wire, 14, b["b0"], BALLAST_KEY, "payload arena")
        CU._eq(out[b["b0"]:b["total"]], CU._up(b["out"]), self.msg("the payload arena behind the ballast"))
        assert_all(out, self.msg("payload arena past the pass's last chunk"), lo=last_chunk_end(b["total"], self.flags))
        assert checksum(wire) == before, self.msg("the wire changed")
        _sync()


def _de_ballast_cases():
    cs = []
    R = cfws.DESERIALIZE_REASSEMBLE
    for dn, delta in DELTAS.items():
        for pe in (False, True):
            s = ("_pe" if pe else "") + "_" + dn
            cs += [DeBallastCase("de_off_plan3000" + s, 3000, 1200, 16, 0, pe, delta),
                   DeBallastCase("de_off_reasm8000" + s, 8000, 100, 16, R, pe, delta),
                   DeBallastCase("de_off_single" + s, CU.BIG_N, 40, 1, 0, pe, delta)]
    return cs


# ---- the uniform send and the implicit-index receive ----------------------------------

UNIFORM_SEED = 0x5EED0077


class UniformCase(WideCase):
    """cfws_serialize_uniform, then cfws_deserialize_slots_uniform on its wire:
    n frames of fs bytes with n * W just over 2^32 + 2^24, so i * W, i *
    frame_stride, i * fs and i * slot all pass 2^32. Frames are independent:
    the frames within 64 KiB of the mark on wire and payload, the first and
    last 8 and 256 drawn ones are compared with the oracle frame by frame,
    the round trip whole on the device."""
    operand = "i * W / i * frame_stride / i * slot_bytes"

    def __init__(self, name, claim, fs, mask=True):
        super().__init__(name)
        self.claim, self.fs, self.mask = claim, fs, mask
        self.Wf = fs + O.header_size(fs, mask)
        # n * W just over 2^32 + 2^24; more where the payload arena would otherwise stay below 2^32
        self.n = max((MARK + (1 << 24)) // self.Wf, (MARK + (1 << 20)) // fs) + 1
        self.slot = max(16, W.round16(fs))

    def samples(self) -> np.ndarray:
        n, near = self.n, []
        for stride in (self.Wf, self.fs, self.slot):
            lo, hi = (MARK - 65536) // stride - 1, (MARK + 65536) // stride + 1
            near += list(range(max(lo, 0), min(hi + 1, n)))
        rng = np.random.default_rng(self.fs)
        return np.unique(np.concatenate([near, np.arange(8), np.arange(n - 8, n), rng.integers(0, n, 256)])).astype(np.int64)

    def build(self):
        n = self.n

        def cross(stride, length):     # the first and last frames and those around the mark stand for all
            i = np.unique(np.concatenate([[0, n - 1], np.arange(MARK // stride - 2, MARK // stride + 3)])).astype(np.uint64)
            return crossing(i * np.uint64(stride), np.full(len(i), length))
        return dict(keys=O.keys(77, n) if self.mask else None, total=n * self.Wf, samples=self.samples(), bad=n - 1000,
                    cross=cross(self.Wf, self.Wf), pcross=cross(self.fs, self.fs), scross=cross(self.slot, self.fs))

    def route(self):
        return cfws.lib().cfws_serialize_uniform_pass_kernel(self.fs, int(self.mask)).decode()

    def device_bytes(self):
        n = self.n
        return n * self.fs + 16 + W.round16(n * self.Wf) + 4096 + n * self.slot + 4096 + 12 * n + 2 * n * self.fs // 8

    def run(self):
        torch = _torch()
        b, n, fs, Wf, slot = self.built(), self.n, self.fs, self.Wf, self.slot
        payload = torch.empty(W.round16(n * fs) + 16, dtype=torch.uint8, device="cuda")
        cfws.fill_splitmix(payload, UNIFORM_SEED)
        before = checksum(payload)
        keys = CU._up(b["keys"].view(np.int32)) if self.mask else None
        cap = W.round16(b["total"])
        wire = sentinel_arena(cap + 4096)
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        cfws.serialize_uniform(payload, keys, n, fs, wire, mask=self.mask, total_t=tot, wire_capacity=cap)
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        # the sampled frames, one download per run of consecutive frames
        smp = b["samples"]
        for run in np.split(smp, np.nonzero(np.diff(smp) > 1)[0] + 1):
            lo, cnt = int(run[0]), len(run)
            src, got = get(payload, lo * fs, cnt * fs), get(wire, lo * Wf, cnt * Wf)
            for j in range(cnt):
                f = lo + j
                want = O.serialize_keyed(True, 2, self.mask, int(b["keys"][f]) if self.mask else 0,
                                         src[j * fs:(j + 1) * fs].tobytes())
                assert got[j * Wf:(j + 1) * Wf].tobytes() == want, \
                    self.msg(f"frame {f} at wire offset {f * Wf} (2^32 {f * Wf - MARK:+d}) differs from the oracle's")
        assert_all(wire, self.msg("wire arena past the total"), lo=cap)
        # the round trip, whole
        back = sentinel_arena(n * slot + 4096)
        info = torch.full((n, 8), CU.DESC_POISON, dtype=torch.uint8, device="cuda")
        mism = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        one = np.zeros(1, dtype=cfws.INFO_DTYPE)
        one[0] = (fs, 1, 2, 0)
        word = int(one.view(np.int64)[0])

        def receive():
            tot.fill_(-1)
            cfws.deserialize_slots_uniform(wire, b["total"], n, Wf, back, slot, info, tot, mism, payload_capacity=n * slot)
            torch.cuda.synchronize()
            assert int(tot.item()) == n * slot, self.msg(f"receive total {int(tot.item())}")

        def rows_equal(lo, hi):
            got = back[lo * slot:hi * slot].view(hi - lo, slot)
            src = payload[lo * fs:hi * fs].view(hi - lo, fs)
            return torch.equal(got[:, :fs], src) and bool((got[:, fs:] == 0).all())

        receive()
        assert int(mism.item()) == 0, self.msg(f"mismatch count {int(mism.item())}")
        CU._all(info.view(torch.int64).reshape(-1), word, self.msg("info entries"))
        step = max(1 << 16, (1 << 28) // slot)
        for lo in range(0, n, step):
            assert rows_equal(lo, min(lo + step, n)), self.msg(f"round trip differs in frames [{lo}, {lo + step})")
        assert_all(back, self.msg("payload arena past n * slot"), lo=n * slot)
        # one corrupted frame above 2^32: counted, its slot untouched
        c = b["bad"]
        assert c * Wf > MARK and c * slot > MARK
        wire[c * Wf] |= 0x40
        back.fill_(SENT)
        receive()
        assert int(mism.item()) == 1, self.msg(f"mismatch count {int(mism.item())} with one corrupted frame")
        assert_all(back, self.msg(f"the corrupted frame {c}'s slot"), lo=c * slot, hi=(c + 1) * slot)
        iw = info.view(torch.int64).reshape(-1)
        assert int(iw[c].item()) != word and bool((iw[:c] == word).all()) and bool((iw[c + 1:] == word).all()), \
            self.msg("info entries with one corrupted frame")
        assert rows_equal(c - 64, c) and rows_equal(c + 1, c + 65), self.msg("the corrupted frame's neighbours")
        assert checksum(payload) == before, self.msg("the payload arena changed")
        _sync()


def _uniform_cases():
    return [UniformCase("uniform_small_4096", "serialize_uniform_small_kernel", 4096),
            UniformCase("uniform_general_4100", "serialize_uniform_kernel", 4100),
            # 31 wire bytes a frame, 139 M frames: no keys to draw, the shortest batch the bytes kernel takes across 2^32
            UniformCase("uniform_bytes_29_unmasked", "serialize_uniform_bytes_kernel", 29, mask=False)]


# ---- WebSocket over HTTP/2 -------------------------------------------------------------

H2_S = 16384


class H2DeRelocCase(WideCase):
    """cfws_h2_deserialize_batch with d_h2_index across 2^32: 1,520 messages
    (twenty of them two DATA frames long) in a window of the DATA arena. fast:
    the pool holds every DATA payload (the fused plan, the pool never
    written); general: a pool of half the DATA bytes (the pool materialised,
    frames past it OUT_OF_MEMORY). Every offset the call reports is relative
    to the pool or the payload arena, so the oracle's output stands as it is."""
    operand = "d_h2_index"

    def __init__(self, name, mode, delta):
        super().__init__(name)
        self.mode, self.delta = mode, delta

    def build(self):
        rng = np.random.default_rng(1520)
        sizes = rng.choice([0, 7, 126, 1000, 2000], 1520).astype(np.uint64)
        sizes[rng.choice(1520, 20, replace=False)] = rng.integers(17000, 30000, 20).astype(np.uint64)
        m = len(sizes)
        d = np.zeros(m, dtype=O.DESC_DTYPE)
        d["payload_size"] = sizes
        d["payload_off"] = rng.integers(0, CU.PAYLOAD_BYTES - 40000, m).astype(np.uint64)
        d["fin"], d["opcode"] = 1, 2
        d["mask"] = (rng.random(m) < .5).astype(np.uint8)
        d["mask_key"] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32) * d["mask"]
        h2, _ = O.h2_serialize_batch(CU.payload_np(), d, 1, H2_S)
        h2 = h2.copy()
        assert self.delta < len(h2) <= WINDOW_MAX
        index = O.h2_index(h2)
        held = int(np.searchsorted(index, self.delta, side="right")) - 1
        for k in range(3, len(index), 37):
            if k != held:
                h2[int(index[k]) + 3] = 6                  # not a DATA frame
        n = len(index)
        data = len(h2) - 9 * n
        pool = data // 2 if self.mode == "general" else len(h2)
        whole = O.h2_deserialize_batch(h2, index, H2_S, O.DEFAULT_MAX_PAYLOAD, 16, pool, None)["total"]
        cap = W.round16(whole) + 64
        e = O.h2_deserialize_batch(h2, index, H2_S, O.DEFAULT_MAX_PAYLOAD, 16, pool, cap)
        base = MARK - self.delta
        ln = np.diff(np.concatenate([index, [len(h2)]]).astype(np.int64))
        return dict(h2=h2, rel=index, index=index + np.uint64(base), base=base, h2_size=base + len(h2), n=n, pool=pool,
                    cap=cap, e=e, cross=crossing(index + np.uint64(base), ln))

    def device_bytes(self):
        b = self.built()
        return ARENA_BYTES + b["pool"] + 2 * (b["cap"] + 4096) + 100 * b["n"] + \
            cfws.lib().cfws_h2_deserialize_workspace_size(b["n"], b["pool"], b["cap"])

    def run(self):
        torch = _torch()
        b, e = self.built(), self.built()["e"]
        n, m = b["n"], e["n_msg"]
        h2 = sentinel_arena(ARENA_BYTES)
        put(h2, b["base"], b["h2"])
        pool = sentinel_arena(max(b["pool"], 16) + 4096)
        pay = sentinel_arena(b["cap"] + 4096)
        st, md, ms, tot, n_msg = cfws.h2_deserialize(
            h2, b["h2_size"], _idx_t(b["index"]), pool[:b["pool"]], pay[:b["cap"]], H2_S, all_rows=True,
            h2_status_t=torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda"),
            msg_desc_t=torch.full((n, 32), CU.DESC_POISON, dtype=torch.uint8, device="cuda"),
            msg_status_t=torch.full((n,), CU.STATUS_POISON, dtype=torch.int32, device="cuda"),
            total_t=torch.full((1,), -1, dtype=torch.int64, device="cuda"), n_messages_init=CU.COUNT_SENTINEL)
        torch.cuda.synchronize()
        assert n_msg == m, self.msg(f"{n_msg} messages, the oracle has {m}")
        assert int(tot.item()) == e["total"], self.msg(f"total {int(tot.item())} != {e['total']}")
        CU._eq(st, CU._up(e["h2_status"]), self.msg("DATA statuses"))
        CU._eq(ms[:m], CU._up(e["msg_status"]), self.msg("message statuses"))
        CU._eq(md[:m], CU._up(CU._desc_bytes(e["msg_desc"])), self.msg("message descriptors"))
        CU._all(ms[m:], O.PARSE_MORE_DATA, self.msg("statuses of the empty rows"))
        CU._all(md[m:, 8:], 0, self.msg("empty rows"))
        CU._eq(pay[:e["total"]], CU._up(e["payload"][:e["total"]]), self.msg("payload arena"))
        assert_all(pay, self.msg("payload arena past the pass's last chunk"), lo=last_chunk_end(e["total"], 0))
        assert_all(pool, self.msg("pool past its capacity"), lo=W.round16(b["pool"]))
        assert _window(h2, b["base"], b["h2"]), self.msg("the DATA window changed")
        assert_all(h2, self.msg("DATA arena"))
        _sync()


class H2SerBallastCase(WideCase):
    """cfws_h2_serialize_batch at S = 16,384: frame 0's DATA frames end delta
    bytes below 2^32 of the DATA stream (262,000 rows of the DATA-frame plan),
    2,000 frames follow: their rows' offsets lie past 2^32."""
    operand = "DATA-frame row offsets"
    SID = 5

    def __init__(self, name, delta):
        super().__init__(name)
        self.delta, self.n = delta, 2001

    def build(self):
        S, T = H2_S, MARK - self.delta
        k = -(-T // (S + 9))
        w0 = T - 9 * k                                      # the ballast's WS bytes in k DATA frames
        assert -(-w0 // S) == k
        b0 = w0 - 14
        rng = np.random.default_rng(2000)
        sizes = rng.choice([0, 1, 125, 126, 999, 1000, 16376, 16384, 40000], 2000).astype(np.uint64)
        t = CU._frames_desc(rng, sizes, rng.integers(0, CU.PAYLOAD_BYTES - 70000, 2000).astype(np.uint64))
        h2, te = O.h2_serialize_batch(CU.payload_np(), t.view(O.DESC_DTYPE), self.SID, S)
        d = np.zeros(self.n, dtype=cfws.DESC_DTYPE)
        d[0] = (0, 0, b0, BALLAST_KEY, 1, 2, 1, 0)
        d[1:] = t
        e = d.copy()
        e[1:] = te
        e["wire_off"] = W.wire_layout(d)[0]                 # as cfws_serialize_plan writes them
        e["header_size"][0] = 14
        wcap = W.round16(W.wire_layout(d)[1]) + 16
        hcap = cfws.h2_wrapped_bound(wcap, self.n, S)
        # every frame's DATA frames: one row per S wire bytes; the rows' starts in the stream
        wb = te["payload_size"] + te["header_size"].astype(np.uint64)
        hb = wb + np.uint64(9) * ((wb + np.uint64(S - 1)) // np.uint64(S) + (wb == 0))
        starts = T + np.concatenate([[0], np.cumsum(hb)[:-1]]).astype(np.int64)
        assert int(hb.sum()) == len(h2)
        return dict(desc=d, e_desc=e, tail_desc=te, T=T, k=k, w0=w0, b0=b0, h2=h2, total=T + len(h2), wcap=wcap, hcap=hcap,
                    cross=crossing(starts, hb))

    def device_bytes(self):
        b = self.built()
        return MARK + (8 << 20) + b["wcap"] + b["hcap"] + 4096 + len(b["h2"]) + 64 * self.n + \
            cfws.lib().cfws_h2_serialize_workspace_size(self.n, b["wcap"], b["hcap"], H2_S)

    def run(self):
        torch = _torch()
        b, n, S = self.built(), self.n, H2_S
        payload = torch.empty(MARK + (8 << 20), dtype=torch.uint8, device="cuda")
        put(payload, 0, CU.payload_np())
        before = checksum(payload)
        wire = torch.empty(b["wcap"], dtype=torch.uint8, device="cuda")       # scratch: unused from S = 64 on
        h2 = sentinel_arena(b["hcap"] + 4096)
        d_in = b["desc"].copy()
        d_in["wire_off"], d_in["header_size"] = 0x5A5A5A5A5A5A5A5A, CU.DESC_POISON
        d_t = CU._up(CU._desc_bytes(d_in))
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        cfws.h2_serialize(payload, d_t, wire, h2[:b["hcap"]], self.SID, S, total_t=tot)
        torch.cuda.synchronize()
        assert int(tot.item()) == b["total"], self.msg(f"total {int(tot.item())} != {b['total']}")
        CU._eq(d_t, CU._up(CU._desc_bytes(b["e_desc"])), self.msg("descriptors"))
        # the ballast: its first DATA header's length and the WS header, then payload bytes of sampled windows
        head = get(h2, 0, 23)
        assert head[:3].tobytes() == S.to_bytes(3, "big") and head[3] == 0, self.msg("the ballast's first DATA header")
        assert head[9:].tobytes() == ballast_header(b["b0"], BALLAST_KEY), self.msg("the ballast's WS header")
        kb = np.frombuffer(BALLAST_KEY.to_bytes(4, "little"), np.uint8)
        for o, ln in sample_offsets(b["T"], 7):
            p = o + np.arange(ln)
            ws = p // (S + 9) * S + p % (S + 9) - 9           # the WS byte at stream position p (DATA headers: < 0 mod)
            body = (p % (S + 9) >= 9) & (ws >= 14)
            src = get(payload, max(int(ws[body].min()) - 14, 0), ln + 64) if body.any() else None
            k0 = ws[body] - 14
            want = src[k0 - max(int(k0.min()), 0)] ^ kb[k0 % 4]
            assert np.array_equal(get(h2, o, ln)[body], want), self.msg(f"the ballast's bytes at {o} differ")
        CU._eq(h2[b["T"]:b["total"]], CU._up(b["h2"]), self.msg("the DATA stream behind the ballast"))
        assert_all(h2, self.msg("DATA arena past the total"), lo=W.round16(b["total"]))
        assert checksum(payload) == before, self.msg("the payload arena changed")
        _sync()


# ---- the handshake's key offsets -------------------------------------------------------

class HandshakeCase(WideCase):
    """cfws_ws_accept_keys_batch / _upgrade_keys_batch / _check_accept_batch:
    16,000 keys (or answers) packed in a window of a 2^32 + 4 MiB arena, their
    n + 1 offsets across 2^32."""

    def __init__(self, name, call, delta):
        super().__init__(name)
        self.call, self.delta, self.n = call, delta, 16000
        self.operand = "d_resp_off" if call == "check" else "d_key_off"

    def build(self):
        import random

        import handshake_util as HU
        rng = random.Random(16000)
        keys = HU.edited_keys(rng, self.n)
        accepts = [HU.accept_of(k) for k in keys]
        items = keys
        if self.call == "check":
            # the answers: the expected value, or an edited, cut or lengthened one
            items = []
            for a in accepts:
                a, how = a.encode(), rng.randrange(6)
                items.append(a if how > 2 else a[:-1] if how == 0 else a + b"=" if how == 1
                             else a[:5] + bytes([a[5] ^ 1]) + a[6:])
        raw = np.frombuffer(b"".join(items), np.uint8).copy()
        assert self.delta < len(raw) <= WINDOW_MAX
        base = MARK - self.delta
        off = np.zeros(self.n + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(k) for k in items])
        valid = np.array([HU.key_valid(k) for k in keys], np.uint8)
        ok = np.array([HU.check(a.encode(), r) for a, r in zip(accepts, items)], np.uint8) if self.call == "check" else None
        return dict(raw=raw, base=base, rel=off, off=off + base, keys=keys, accepts=accepts, valid=valid, ok=ok,
                    expect=HU.slots(accepts), cross=crossing(off[:-1] + base, np.diff(off)))

    def device_bytes(self):
        return ARENA_BYTES + 200 * self.n

    def run(self):
        torch = _torch()
        b, n, L = self.built(), self.n, cfws.lib()
        arena = sentinel_arena(ARENA_BYTES)
        put(arena, b["base"], b["raw"])
        off = CU._up(b["off"])
        out = torch.zeros(32 * n + 64, dtype=torch.uint8, device="cuda")
        out[32 * n:].fill_(SENT)
        cnt = torch.full((1,), 0x7badbeef, dtype=torch.int32, device="cuda")
        flag = torch.full((n + 64,), SENT, dtype=torch.uint8, device="cuda")
        s = cfws._stream(None)
        if self.call == "accept":
            cfws._check(L.cfws_ws_accept_keys_batch(cfws._p(arena), cfws._p(off), n, cfws._p(out), s), "accept_keys")
        elif self.call == "upgrade":
            cfws._check(L.cfws_ws_upgrade_keys_batch(cfws._p(arena), cfws._p(off), n, cfws._p(flag), cfws._p(out),
                                                     cfws._p(cnt), s), "upgrade_keys")
        else:
            expect = CU._up(b["expect"])
            cfws._check(L.cfws_ws_check_accept_batch(cfws._p(expect), cfws._p(arena), cfws._p(off), n, cfws._p(flag),
                                                     cfws._p(cnt), s), "check_accept")
        torch.cuda.synchronize()
        if self.call != "check":
            got = cfws._slot_strings(out, n)
            bad = [i for i in range(n) if got[i] != b["accepts"][i]]
            assert not bad, self.msg(f"{len(bad)} accept values differ, first keys {bad[:6]} at offsets "
                                     f"{[int(b['off'][i]) for i in bad[:3]]}")
            CU._all(out[32 * n:], SENT, self.msg("bytes past the last accept slot"))
        if self.call != "accept":
            want = b["valid"] if self.call == "upgrade" else b["ok"]
            CU._eq(flag[:n], CU._up(want), self.msg("verdicts"))
            CU._all(flag[n:], SENT, self.msg("bytes past the last verdict"))
            assert int(cnt.item()) == int((want == 0).sum()), self.msg(f"count {int(cnt.item())}")
        assert _window(arena, b["base"], b["raw"]), self.msg("the window changed")
        assert_all(arena, self.msg("arena"))
        _sync()


def _h2_handshake_cases():
    cs = []
    for dn, delta in DELTAS.items():
        cs += [H2DeRelocCase(f"h2de_index_fast_{dn}", "fast", delta), H2DeRelocCase(f"h2de_index_general_{dn}", "general", delta),
               # d_frame_index across 2^32 on the per-frame slot kernel: 4.2 M entries make the average frame short
               SlotCase(f"slots_index_perframe2064_{dn}", "d_frame_index", "deserialize_slots_kernel", 2064,
                        _slot_sizes(25, 1021, 0, 1000, (2064, 2065)), n=4_200_000, wire_delta=delta, seed=25)]
    cs += [H2SerBallastCase("h2ser_rows_S16384", DELTAS["odd16"]),
           HandshakeCase("handshake_accept_key_off", "accept", DELTAS["page"]),
           HandshakeCase("handshake_upgrade_key_off", "upgrade", DELTAS["odd16"]),
           HandshakeCase("handshake_check_resp_off", "check", DELTAS["odd16"])]
    return cs


# ---- the registry ----------------------------------------------------------------------

def _make_cases():
    cs = _slot_cases()
    for dn, delta in INDEX_DELTAS.items():
        cs += [IndexCase(f"index_ws_{dn}", delta),
               IndexCase(f"index_h2_info_{dn}", delta, True, True),
               IndexCase(f"index_h2_noinfo_{dn}", delta, True, False)]
    for dn, delta in DELTAS.items():
        for style in SER_STYLES:
            for pe in (False, True):
                cs.append(SerBallastCase(f"ser_{style}{'_pe' if pe else ''}_{dn}", style, delta, pe))
    cs += [RelayBallastCase("relay_unmask_verbatim", "unmask", RU.VERBATIM, DELTAS["page"]),
           RelayBallastCase("relay_mask_echo", "mask", RU.ECHO_SERVER, DELTAS["odd16"]),
           RelayBallastCase("relay_remask_verbatim", "remask", RU.VERBATIM, DELTAS["odd16"])]
    cs.append(FusedCase("de_fused_a4096"))
    cs += _reloc_cases()
    cs += _de_ballast_cases()
    cs += _uniform_cases()
    cs += _h2_handshake_cases()
    return {c.name: c for c in cs}


_cases = None


def cases() -> dict:
    global _cases
    if _cases is None:
        _cases = _make_cases()
    return _cases


CASE_NAMES = list(cases())
