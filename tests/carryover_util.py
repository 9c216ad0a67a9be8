"""TEST INFRASTRUCTURE ONLY -- the cases of the carry-over tests
(tests/test_gpu_carryover.py, tests/carryover_parity.py, and their CPU half
tests/test_carryover_cases.py): what a batch call must produce whatever its
workspace and its output arrays held before it. DESIGN.md §2.1 lists, per
workspace region, which kernel or memset writes it before which kernel reads
it within one call; a case here is one row group of that table at the
smallest shape that reaches the route.

A case has variants built from its name's seed: B is the checked batch, A the
batch that ran before it on the same workspace ("prev"), with the same n and
the same capacities, and every device-side decision the other way: a larger
total (above the capacity where B's is below), in-region send edges for every
frame or for none, invalid and incomplete frames at other positions, another
message count. A2 and C are a second A and a second B (graph replays).

Everything is compared bit for bit with the oracle (relay_util and
h2_index_util are written from it); the device key draw against the host
form that tests/test_keys_host.py pins. Inputs and expectations are built
once per process and shared by every test that names the case.
"""
from __future__ import annotations

import os
import random
import re
import zlib

import numpy as np

import h2_index_util as HU
import oracle as O
import relay_util as RU
from coldforce_amd import cfws
from coldforce_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coldforce_amd", "csrc")

PATTERNS = ("00", "ff", "aa", "55", "prev")
VARIANTS = {"B": (0, 0), "A": (1, 1), "A2": (1, 2), "C": (0, 3)}     # (style index, seed step)
ARENA, ARENA2 = 0xEE, 0x11            # two arena poisons (the bytes no call may leave standing below its total)
DESC_POISON = 0x5A
STATUS_POISON = 0x5A5A5A5A
COUNT_SENTINEL = 0x5A5A5A             # the host n_messages word before a call
PAYLOAD_BYTES = 1 << 22
BIG_N = 524_289                       # one frame past 2,048 plan blocks of 256: the single-pass plans


def _torch():
    import torch
    return torch


# ---- the thresholds, read from the code ----------------------------------------

def code_constants() -> dict:
    """The launch thresholds the routes hang on, parsed from the sources."""
    text = "".join(open(os.path.join(CSRC, f)).read()
                   for f in ("cfws_kernels.h", "cfws_device.hip", "cfws_plan.hip"))

    def num(expr):
        expr = re.sub(r"(\d+)(ull|ul|u|ll)\b", r"\1", expr.strip())
        assert re.fullmatch(r"[\d\s<*+()]+", expr), expr
        return int(eval(expr))                                          # digits, <<, *, + only

    def constexpr(name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, name
        return num(m.group(1))

    def define(name):
        m = re.search(r"#define\s+%s\s+(\S+)" % name, text)
        assert m, name
        return num(m.group(1))

    k = dict(threads=constexpr("kThreads"), small_frames=constexpr("kSmallFrames"),
             small_bytes=constexpr("kSmallBytes"), self_scan_blocks=constexpr("kSelfScanBlocks"),
             fused_avg_max=constexpr("kFusedAvgMax"), inreg_max=define("CFWS_SER_INREG_MAX"),
             index_slots=constexpr("kIndexSlots"))
    k["plan_block"] = k["threads"] * define("CFWS_PLAN_ITEMS")
    k["ser_single_block"] = define("CFWS_SER_PLAN_THREADS") * define("CFWS_SINGLE_ITEMS_SER")
    k["de_single_block"] = define("CFWS_DE_PLAN_THREADS") * define("CFWS_SINGLE_ITEMS_DESER")
    k["fused_block"] = define("CFWS_FUSED_THREADS") * define("CFWS_FUSED_ITEMS")
    return k


def blocks(n: int, per: int) -> int:
    return (n + per - 1) // per


# ---- shared inputs -------------------------------------------------------------

_shared = {}


def payload_np() -> np.ndarray:
    if "np" not in _shared:
        _shared["np"] = O.fill_splitmix(PAYLOAD_BYTES, 77, 0)
    return _shared["np"]


def payload_t():
    if "t" not in _shared:
        _shared["t"] = _torch().from_numpy(payload_np()).cuda()
    return _shared["t"]


def _frames_desc(rng, sizes, offs, opcodes=(0, 1, 2, 9)):
    n = len(sizes)
    d = np.zeros(n, dtype=cfws.DESC_DTYPE)
    d["payload_size"] = sizes
    d["payload_off"] = offs
    d["fin"] = (rng.random(n) < 0.8).astype(np.uint8)
    d["opcode"] = rng.choice(list(opcodes), n).astype(np.uint8)
    d["mask"] = (rng.random(n) < 0.7).astype(np.uint8)
    d["mask_key"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) * d["mask"]
    return d


MIXED_SIZES = [0, 1, 3, 4, 5, 15, 16, 17, 124, 125, 126, 127, 128, 1000, 4095, 4096, 4097]

# send styles: (low, high, how the payload offsets sit)
SEND_STYLES = {
    "small_lo": (0, 3000, "any"), "small_hi": (4300, 6000, "any"),
    "inreg": (80, 2000, "aligned"), "inreg_hi": (2000, 3584, "aligned"), "odd_big": (2001, 4000, "odd"),
    "tiny": (0, 40, "any"), "inreg_small": (80, 120, "aligned"), "odd_mid": (121, 400, "odd"),
}


def send_desc(style: str, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    offs = rng.integers(0, PAYLOAD_BYTES - 70000, n).astype(np.uint64)
    if style == "mixed":              # every region class; one 64 KiB frame in a hundred
        sizes = rng.choice(MIXED_SIZES, n)
        sizes[rng.random(n) < 0.01] = 65536
        return _frames_desc(rng, sizes.astype(np.uint64), offs)
    base = "inreg" if style == "inreg_one_bad" else style
    lo, hi, where = SEND_STYLES[base]
    sizes = rng.integers(lo, hi + 1, n).astype(np.uint64)
    if where == "aligned":
        offs &= ~np.uint64(15)
    elif where == "odd":
        offs |= np.uint64(1)
    if style == "inreg_one_bad":
        sizes[n // 2] = 10
    return _frames_desc(rng, sizes, offs)


def inreg_ok(desc: np.ndarray, inreg_max: int) -> np.ndarray:
    """ser_inreg_frame_ok of every frame (cfws_plan.hip)."""
    s = desc["payload_size"]
    return (s >= 80) & (s <= inreg_max) & (desc["payload_off"] % 16 == 0)


# ---- cases ---------------------------------------------------------------------

class Case:
    kind = ""
    graph = None                       # "serialize" / "deserialize": cfws.Graph captures it

    def __init__(self, name):
        self.name = name
        self._in, self._exp, self._dev, self._devx, self._ar = {}, {}, {}, {}, None

    def seed(self, variant):
        return (zlib.crc32(self.name.encode()) & 0xFFFFFF) * 8 + VARIANTS[variant][1]

    def style(self, variant):
        return self.styles[VARIANTS[variant][0]]

    def inputs(self, variant):
        if variant not in self._in:
            self._in[variant] = self.build(variant)
        return self._in[variant]

    def expect(self, variant):
        if variant not in self._exp:
            self._exp[variant] = self.oracle(variant)
        return self._exp[variant]

    def dev(self, variant):
        """The variant's inputs on the device."""
        if variant not in self._dev:
            self._dev[variant] = self.upload(variant)
        return self._dev[variant]

    def devx(self, variant):
        """The variant's expectation on the device."""
        if variant not in self._devx:
            self._devx[variant] = self.upload_expect(variant)
        return self._devx[variant]

    def arenas(self):
        if self._ar is None:
            self._ar = self.alloc()
        return self._ar

    def release(self):
        self._in, self._exp, self._dev, self._devx, self._ar = {}, {}, {}, {}, None

    # one call: load the variant and poison every output, launch, wait, check
    def run(self, variant, ws, arena=ARENA, stream=None, check=True):
        torch = _torch()
        self.load(variant, arena)
        torch.cuda.synchronize()
        self.launch(ws, stream)
        (stream.synchronize() if stream is not None else torch.cuda.synchronize())
        if check:
            self.check(variant, arena)


def _eq(got, want, what):
    torch = _torch()
    if got.dtype != want.dtype:
        want = want.view(got.dtype)
    if not torch.equal(got.reshape(-1), want.reshape(-1)):
        bad = torch.nonzero(got.reshape(-1) != want.reshape(-1)).reshape(-1)
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} entries differ, first at {bad[:8].tolist()}")


def _all(t, value, what):
    torch = _torch()
    if t.numel() and not bool((t == value).all()):
        bad = torch.nonzero(t.reshape(-1) != value).reshape(-1)
        raise AssertionError(f"{what}: {bad.numel()} entries are not {value:#x}, first at {bad[:8].tolist()}")


def _up(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _desc_bytes(d):
    return np.ascontiguousarray(d, dtype=cfws.DESC_DTYPE).view(np.uint8).reshape(-1, 32)


class SerCase(Case):
    """cfws_serialize_batch, or with pe cfws_serialize_plan + cfws_serialize_execute."""
    kind, graph = "ser", "serialize"

    def __init__(self, name, n, styles, pe=False, cap=None):
        super().__init__(name)
        self.n, self.styles, self.pe, self._cap = n, styles, pe, cap

    def build(self, variant):
        return send_desc(self.style(variant), self.n, self.seed(variant))

    @property
    def cap(self):                     # B fits, with a little room; A does not
        if self._cap is None:
            self._cap = W.round16(W.wire_layout(self.inputs("B"))[1]) + 64
        return self._cap

    def oracle(self, variant):
        wire, d = O.serialize_batch(payload_np(), self.inputs(variant).view(O.DESC_DTYPE))
        return dict(wire=wire, desc=d, total=len(wire))

    def ws_bytes(self):
        return cfws.lib().cfws_workspace_size(self.n, self.cap)

    def alloc(self):
        torch = _torch()
        return dict(desc=torch.empty((self.n, 32), dtype=torch.uint8, device="cuda"),
                    wire=torch.empty(self.cap + 4096, dtype=torch.uint8, device="cuda"),
                    total=torch.empty(1, dtype=torch.int64, device="cuda"))

    def upload(self, variant):
        d = self.inputs(variant).copy()
        d["wire_off"] = 0x5A5A5A5A5A5A5A5A          # the descriptor's two output fields, poisoned
        d["header_size"] = DESC_POISON
        return dict(desc_in=_up(_desc_bytes(d)))

    def upload_expect(self, variant):
        e = self.expect(variant)
        return dict(wire=_up(e["wire"][:self.cap]), desc=_up(_desc_bytes(e["desc"])))

    def load(self, variant, arena):
        ar = self.arenas()
        ar["desc"].copy_(self.dev(variant)["desc_in"])
        ar["wire"].fill_(arena)
        ar["total"].fill_(-1)

    def launch(self, ws, stream=None):
        ar = self.arenas()
        wire = ar["wire"][:self.cap]
        if self.pe:
            cfws.serialize_plan(ar["desc"], self.cap, ar["total"], ws, stream=stream)
            cfws.serialize_execute(payload_t(), ar["desc"], wire, ws, self.cap, stream=stream)
        else:
            cfws.serialize(payload_t(), ar["desc"], wire, ws, ar["total"], stream=stream)

    def capture(self, ws):
        ar = self.arenas()
        return cfws.Graph.serialize(payload_t(), ar["desc"], ar["wire"][:self.cap], ws, ar["total"])

    def check(self, variant, arena):
        ar, e, dv = self.arenas(), self.expect(variant), self.devx(variant)
        total = int(ar["total"].item())
        assert total == e["total"], (self.name, variant, total, e["total"])     # the unclamped total
        _eq(ar["desc"], dv["desc"], f"{self.name}/{variant} descriptors")
        w = min(total, self.cap)
        _eq(ar["wire"][:w], dv["wire"][:w], f"{self.name}/{variant} wire")
        _all(ar["wire"][w:min(W.round16(w), self.cap)], 0, f"{self.name}/{variant} bytes up to round16(total)")
        _all(ar["wire"][self.cap:], arena, f"{self.name}/{variant} bytes past the capacity")

    def outputs(self, variant):
        ar = self.arenas()
        return [ar["desc"], ar["total"], ar["wire"][:min(self.expect(variant)["total"], self.cap)]]


class DeCase(Case):
    """cfws_deserialize_batch (pe: plan + execute) over a wire arena of a
    fixed size: frames from its start, zeros after them (not indexed)."""
    kind, graph = "de", "deserialize"

    def __init__(self, name, n, ranges, align, flags=0, cut=False, pe=False):
        super().__init__(name)
        self.n, self.styles, self.align, self.flags, self.cut, self.pe = n, ranges, align, flags, cut, pe
        self.wsize = W.round16(n * (max(r[1] for r in ranges) + 14))
        self._cap = None

    def build(self, variant):
        lo, hi = self.style(variant)
        a = VARIANTS[variant][0]
        n = self.n
        rng = np.random.default_rng(self.seed(variant))
        sizes = rng.integers(lo, hi + 1, n).astype(np.uint64)
        offs = rng.integers(0, PAYLOAD_BYTES - 70000, n).astype(np.uint64)
        d = _frames_desc(rng, sizes, offs, opcodes=(0, 1, 2))
        if self.flags:                 # control frames between the fragments, elsewhere in A
            ctl = rng.random(n) < (0.3 if a else 0.15)
            d["opcode"][ctl] = rng.choice([8, 9, 10], int(ctl.sum())).astype(np.uint8)
            d["fin"][ctl] = 1
            d["payload_size"][ctl] = np.minimum(d["payload_size"][ctl], 125)
        wire, d = O.serialize_batch(payload_np(), d.view(O.DESC_DTYPE))
        index = d["wire_off"].astype(np.uint64)
        buf = np.zeros(self.wsize + 16, np.uint8)
        buf[:len(wire)] = wire
        bad = np.arange(51 if a else 3, n, 96)                            # RSV2: INVALID_FRAME
        buf[index[bad].astype(np.int64)] |= 0x40
        more = np.arange(103 if a else 7, n, 192)                         # one byte before the end: MORE_DATA
        index[more] = self.wsize - 1
        return dict(wire=buf, index=index, bad=bad, more=more)

    def _oracle(self, variant, cap):
        i = self.inputs(variant)
        return O.deserialize_batch(i["wire"][:self.wsize], i["index"], align=self.align, capacity=cap,
                                   flags=self.flags)

    @property
    def cap(self):
        if self._cap is None:
            whole = self._oracle("B", self.wsize + self.align * self.n + 64)[3]
            self._cap = whole // 3 + 5 if self.cut else W.round16(whole) + 64
            self.whole_b = whole
        return self._cap

    def oracle(self, variant):
        out, d, st, tot = self._oracle(variant, self.cap)
        return dict(out=out[:tot], desc=d, status=st, total=tot)

    def route(self):
        return cfws.lib().cfws_deserialize_pass_kernel(self.n, self.wsize, self.align, self.flags, self.cap).decode()

    def ws_bytes(self):
        return cfws.lib().cfws_workspace_size(self.n, self.cap)

    def alloc(self):
        torch = _torch()
        return dict(wire=torch.empty(self.wsize + 16, dtype=torch.uint8, device="cuda"),
                    index=torch.empty(self.n, dtype=torch.int64, device="cuda"),
                    desc=torch.empty((self.n, 32), dtype=torch.uint8, device="cuda"),
                    status=torch.empty(self.n, dtype=torch.int32, device="cuda"),
                    out=torch.empty(self.cap + 4096, dtype=torch.uint8, device="cuda"),
                    total=torch.empty(1, dtype=torch.int64, device="cuda"))

    def upload(self, variant):
        i = self.inputs(variant)
        return dict(wire=_up(i["wire"]), index=_up(i["index"].view(np.int64)))

    def upload_expect(self, variant):
        e = self.expect(variant)
        return dict(out=_up(e["out"]), desc=_up(_desc_bytes(e["desc"])), status=_up(e["status"]))

    def load(self, variant, arena):
        ar, dv = self.arenas(), self.dev(variant)
        ar["wire"].copy_(dv["wire"])
        ar["index"].copy_(dv["index"])
        ar["desc"].fill_(DESC_POISON)
        ar["status"].fill_(STATUS_POISON)
        ar["out"].fill_(arena)
        ar["total"].fill_(-1)

    def launch(self, ws, stream=None):
        ar = self.arenas()
        out = ar["out"][:self.cap]
        if self.pe:
            cfws.deserialize_plan(ar["wire"], self.wsize, ar["index"], ar["desc"], ar["status"], self.cap,
                                  ar["total"], ws, align=self.align, flags=self.flags, stream=stream)
            cfws.deserialize_execute(ar["wire"], ar["desc"], ar["status"], out, ws, self.cap, flags=self.flags,
                                     stream=stream)
        else:
            cfws.deserialize(ar["wire"], self.wsize, ar["index"], out, ar["desc"], ar["status"], ws, ar["total"],
                             align=self.align, flags=self.flags, stream=stream)

    def capture(self, ws):
        ar = self.arenas()
        return cfws.Graph.deserialize(ar["wire"], self.wsize, ar["index"], ar["desc"], ar["status"],
                                      ar["out"][:self.cap], ws, ar["total"], align=self.align, flags=self.flags)

    def check(self, variant, arena):
        ar, e, dv = self.arenas(), self.expect(variant), self.devx(variant)
        total = int(ar["total"].item())
        assert total == e["total"], (self.name, variant, total, e["total"])
        _eq(ar["status"], dv["status"], f"{self.name}/{variant} statuses")
        _eq(ar["desc"], dv["desc"], f"{self.name}/{variant} descriptors")
        _eq(ar["out"][:total], dv["out"], f"{self.name}/{variant} payload arena")     # padding: zeros
        _all(ar["out"][self.cap:], arena, f"{self.name}/{variant} bytes past the capacity")

    def outputs(self, variant):
        ar = self.arenas()
        return [ar["desc"], ar["status"], ar["total"], ar["out"][:self.expect(variant)["total"]]]


class RelayCase(Case):
    kind = "relay"

    def __init__(self, name, n, ranges, policy, out_mask):
        super().__init__(name)
        self.n, self.styles, self.policy, self.out_mask = n, ranges, policy, out_mask
        self._cap = None

    def build(self, variant):
        lo, hi = self.style(variant)
        a, n = VARIANTS[variant][0], self.n
        rng = np.random.default_rng(self.seed(variant))
        sizes = rng.integers(lo, hi + 1, n)
        ops = rng.choice([0, 1, 2, 8, 9, 10], n)
        bad = np.arange(51 if a else 3, n, 96)
        wire, starts = RU.frames_wire(sizes, rng.random(n) < .6, rng.random(n) < .7, ops, self.seed(variant),
                                      [int(i) for i in bad])
        keys = (O.splitmix_words(self.seed(variant) ^ 0x99, 0, n) >> np.uint64(7)).astype(np.uint32)
        # B's wire ends one byte early (its last frame MORE_DATA), A's is whole
        return dict(wire=wire, wire_size=len(wire) - (0 if a else 1), starts=starts, keys=keys)

    def _expect(self, variant):
        i = self.inputs(variant)
        return RU.expect_relay(i["wire"], i["wire_size"], i["starts"], self.policy, self.out_mask, i["keys"])

    @property
    def cap(self):
        if self._cap is None:
            self._cap = W.round16(self.expect("B")["total"]) + 64
        return self._cap

    def oracle(self, variant):
        out, _, desc, status = self._expect(variant)
        return dict(out=out, desc=desc, status=status, total=len(out))

    def ws_bytes(self):
        return cfws.lib().cfws_relay_workspace_size(self.n, self.cap)

    def alloc(self):
        torch = _torch()
        return dict(desc=torch.empty((self.n, 32), dtype=torch.uint8, device="cuda"),
                    status=torch.empty(self.n, dtype=torch.int32, device="cuda"),
                    out=torch.empty(self.cap + 4096, dtype=torch.uint8, device="cuda"),
                    total=torch.empty(1, dtype=torch.int64, device="cuda"))

    def upload(self, variant):
        i = self.inputs(variant)
        buf = np.zeros(W.round16(len(i["wire"])) + 16, np.uint8)
        buf[:len(i["wire"])] = i["wire"]
        return dict(wire=_up(buf), index=_up(i["starts"].view(np.int64)), keys=_up(i["keys"].view(np.int32)))

    def upload_expect(self, variant):
        e = self.expect(variant)
        return dict(out=_up(e["out"][:self.cap]), desc=_up(_desc_bytes(e["desc"])), status=_up(e["status"]))

    def load(self, variant, arena):
        ar = self.arenas()
        self._v = variant
        ar["desc"].fill_(DESC_POISON)
        ar["status"].fill_(STATUS_POISON)
        ar["out"].fill_(arena)
        ar["total"].fill_(-1)

    def launch(self, ws, stream=None):
        ar, dv, i = self.arenas(), self.dev(self._v), self.inputs(self._v)
        cfws.relay(dv["wire"], i["wire_size"], dv["index"], ar["out"][:self.cap], self.policy, self.out_mask,
                   dv["keys"] if self.out_mask else None, ar["desc"], ar["status"], ws, ar["total"],
                   out_capacity=self.cap, stream=stream)

    def check(self, variant, arena):
        ar, e, dv = self.arenas(), self.expect(variant), self.devx(variant)
        total = int(ar["total"].item())
        assert total == e["total"], (self.name, variant, total, e["total"])
        _eq(ar["status"], dv["status"], f"{self.name}/{variant} statuses")
        _eq(ar["desc"], dv["desc"], f"{self.name}/{variant} descriptors")
        w = min(total, self.cap)
        _eq(ar["out"][:w], dv["out"][:w], f"{self.name}/{variant} outgoing wire")
        _all(ar["out"][self.cap:], arena, f"{self.name}/{variant} bytes past the capacity")

    def outputs(self, variant):
        ar = self.arenas()
        return [ar["desc"], ar["status"], ar["total"], ar["out"][:min(self.expect(variant)["total"], self.cap)]]


class H2SerCase(Case):
    kind = "h2ser"
    SID = 5

    def __init__(self, name, n, S, styles):
        super().__init__(name)
        self.n, self.S, self.styles = n, S, styles
        self._caps = None

    def build(self, variant):
        rng = np.random.default_rng(self.seed(variant))
        sizes = rng.choice(self.style(variant), self.n).astype(np.uint64)
        offs = rng.integers(0, PAYLOAD_BYTES - 70000, self.n).astype(np.uint64)
        return _frames_desc(rng, sizes, offs)

    @property
    def caps(self):                    # (WS wire scratch, DATA stream): B fits both
        if self._caps is None:
            wcap = W.round16(W.wire_layout(self.inputs("B"))[1]) + 16
            self._caps = (wcap, cfws.h2_wrapped_bound(wcap, self.n, self.S))
        return self._caps

    def oracle(self, variant):
        d = self.inputs(variant)
        h2, dexp = O.h2_serialize_batch(payload_np(), d.view(O.DESC_DTYPE), self.SID, self.S)
        dexp = dexp.copy()
        dexp["wire_off"] = W.wire_layout(d)[0]          # as cfws_serialize_plan writes them
        return dict(h2=h2, desc=dexp, total=len(h2))

    def ws_bytes(self):
        return cfws.lib().cfws_h2_serialize_workspace_size(self.n, self.caps[0], self.caps[1], self.S)

    def alloc(self):
        torch = _torch()
        return dict(desc=torch.empty((self.n, 32), dtype=torch.uint8, device="cuda"),
                    wire=torch.empty(self.caps[0], dtype=torch.uint8, device="cuda"),
                    h2=torch.empty(self.caps[1] + 4096, dtype=torch.uint8, device="cuda"),
                    total=torch.empty(1, dtype=torch.int64, device="cuda"))

    def upload(self, variant):
        d = self.inputs(variant).copy()
        d["wire_off"] = 0x5A5A5A5A5A5A5A5A
        d["header_size"] = DESC_POISON
        return dict(desc_in=_up(_desc_bytes(d)))

    def upload_expect(self, variant):
        e = self.expect(variant)
        return dict(h2=_up(e["h2"][:self.caps[1]]), desc=_up(_desc_bytes(e["desc"])))

    def load(self, variant, arena):
        ar = self.arenas()
        ar["desc"].copy_(self.dev(variant)["desc_in"])
        ar["wire"].fill_(arena)
        ar["h2"].fill_(arena)
        ar["total"].fill_(-1)

    def launch(self, ws, stream=None):
        ar = self.arenas()
        cfws.h2_serialize(payload_t(), ar["desc"], ar["wire"], ar["h2"][:self.caps[1]], self.SID, self.S, ws,
                          ar["total"], stream=stream)

    def check(self, variant, arena):
        ar, e, dv = self.arenas(), self.expect(variant), self.devx(variant)
        total = int(ar["total"].item())
        assert total == e["total"], (self.name, variant, total, e["total"])
        _eq(ar["desc"], dv["desc"], f"{self.name}/{variant} descriptors")
        w = min(total, self.caps[1])
        _eq(ar["h2"][:w], dv["h2"][:w], f"{self.name}/{variant} DATA stream")
        _all(ar["h2"][self.caps[1]:], arena, f"{self.name}/{variant} bytes past the capacity")

    def outputs(self, variant):
        ar = self.arenas()
        return [ar["desc"], ar["total"], ar["h2"][:min(self.expect(variant)["total"], self.caps[1])]]


H2_FRAME = 16384
H2_STYLES = {            # message payload sizes; "two": every message is two DATA frames
    "one": lambda rng: rng.choice([0, 7, 126, 1000, 5000], 3000),
    "two": lambda rng: rng.integers(17000, 30000, 1500),
    "one_big": lambda rng: rng.integers(6000, 12000, 3000),
    # 2,000 one-frame and 500 two-frame messages, the last message never closed
    "mix_open": lambda rng: np.where(np.arange(2500) % 5 == 4, rng.integers(17000, 30000, 2500),
                                     rng.choice([0, 7, 126, 1000, 5000], 2500)),
}
H2_DATA_FRAMES = 3000


class H2DeCase(Case):
    """cfws_h2_deserialize_batch: fast (the pool holds every DATA payload),
    general (pool_capacity at half the DATA bytes), open (the last message
    never sees END_STREAM: n_messages < n_h2)."""
    kind = "h2de"

    def __init__(self, name, mode, styles):
        super().__init__(name)
        self.mode, self.styles, self.n = mode, styles, H2_DATA_FRAMES
        self._caps = None

    def build(self, variant):
        style, a = self.style(variant), VARIANTS[variant][0]
        rng = np.random.default_rng(self.seed(variant))
        sizes = H2_STYLES[style](rng).astype(np.uint64)
        m = len(sizes)
        d = np.zeros(m, dtype=O.DESC_DTYPE)
        d["payload_size"] = sizes
        d["payload_off"] = rng.integers(0, PAYLOAD_BYTES - 40000, m).astype(np.uint64)
        d["fin"], d["opcode"] = 1, 2
        d["mask"] = (rng.random(m) < .5).astype(np.uint8)
        d["mask_key"] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32) * d["mask"]
        h2, _ = O.h2_serialize_batch(payload_np(), d, 1, H2_FRAME)
        h2 = h2.copy()
        index = O.h2_index(h2)
        for k in (range(5, len(index), 41) if a else range(3, len(index), 37)):
            h2[int(index[k]) + 3] = 6                  # not a DATA frame
        if style == "mix_open":
            h2[int(index[-1]) + 4] &= 0xFE             # END_STREAM cleared
        return dict(h2=h2, index=index, messages=m)

    def _oracle(self, variant, pool_cap, payload_cap):
        i = self.inputs(variant)
        return O.h2_deserialize_batch(i["h2"], i["index"], H2_FRAME, O.DEFAULT_MAX_PAYLOAD, 16, pool_cap, payload_cap)

    @property
    def caps(self):                    # (pool, payload)
        if self._caps is None:
            i = self.inputs("B")
            data = len(i["h2"]) - 9 * len(i["index"])
            pool = data // 2 if self.mode == "general" else len(i["h2"])
            whole = self._oracle("B", pool, None)["total"]
            self._caps = (pool, W.round16(whole) + 64)
        return self._caps

    def oracle(self, variant):
        return self._oracle(variant, *self.caps)

    def ws_bytes(self):
        return cfws.lib().cfws_h2_deserialize_workspace_size(self.n, *self.caps)

    def alloc(self):
        torch = _torch()
        n = self.n
        return dict(h2_status=torch.empty(n, dtype=torch.int32, device="cuda"),
                    msg_desc=torch.empty((n, 32), dtype=torch.uint8, device="cuda"),
                    msg_status=torch.empty(n, dtype=torch.int32, device="cuda"),
                    total=torch.empty(1, dtype=torch.int64, device="cuda"),
                    pool=torch.empty(max(self.caps[0], 16), dtype=torch.uint8, device="cuda"),
                    pay=torch.empty(self.caps[1] + 4096, dtype=torch.uint8, device="cuda"))

    def upload(self, variant):
        i = self.inputs(variant)
        buf = np.concatenate([i["h2"], np.zeros(16, np.uint8)])
        return dict(h2=_up(buf), index=_up(i["index"].view(np.int64)))

    def upload_expect(self, variant):
        e = self.expect(variant)
        return dict(h2_status=_up(e["h2_status"]), msg_desc=_up(_desc_bytes(e["msg_desc"])),
                    msg_status=_up(e["msg_status"]), pay=_up(e["payload"][:e["total"]]))

    def load(self, variant, arena):
        ar = self.arenas()
        self._v = variant
        ar["h2_status"].fill_(STATUS_POISON)
        ar["msg_desc"].fill_(DESC_POISON)
        ar["msg_status"].fill_(STATUS_POISON)
        ar["total"].fill_(-1)
        ar["pool"].fill_(arena)
        ar["pay"].fill_(arena)
        self.n_messages = None

    def launch(self, ws, stream=None):
        ar, dv, i = self.arenas(), self.dev(self._v), self.inputs(self._v)
        *_, self.n_messages = cfws.h2_deserialize(
            dv["h2"], len(i["h2"]), dv["index"], ar["pool"][:self.caps[0]], ar["pay"][:self.caps[1]], H2_FRAME,
            ws_t=ws, stream=stream, all_rows=True, h2_status_t=ar["h2_status"], msg_desc_t=ar["msg_desc"],
            msg_status_t=ar["msg_status"], total_t=ar["total"], n_messages_init=COUNT_SENTINEL)

    def check(self, variant, arena):
        ar, e, dv = self.arenas(), self.expect(variant), self.devx(variant)
        m = e["n_msg"]
        assert self.n_messages == m, (self.name, variant, self.n_messages, m)
        total = int(ar["total"].item())
        assert total == e["total"], (self.name, variant, total, e["total"])
        _eq(ar["h2_status"], dv["h2_status"], f"{self.name}/{variant} DATA statuses")
        _eq(ar["msg_status"][:m], dv["msg_status"], f"{self.name}/{variant} message statuses")
        _eq(ar["msg_desc"][:m], dv["msg_desc"], f"{self.name}/{variant} message descriptors")
        # rows n_messages..n_h2-1: MORE_DATA, no payload, no header (payload_off unspecified)
        _all(ar["msg_status"][m:], O.PARSE_MORE_DATA, f"{self.name}/{variant} statuses of the empty rows")
        _all(ar["msg_desc"][m:, 8:], 0, f"{self.name}/{variant} empty rows")
        _eq(ar["pay"][:total], dv["pay"], f"{self.name}/{variant} payload arena")
        _all(ar["pay"][self.caps[1]:], arena, f"{self.name}/{variant} bytes past the capacity")

    def outputs(self, variant):
        ar, m = self.arenas(), self.expect(variant)["n_msg"]
        return [ar["h2_status"], ar["msg_status"], ar["msg_desc"][:m], ar["msg_desc"][m:, 8:], ar["total"],
                ar["pay"][:self.expect(variant)["total"]]]


class H2CountCase(H2DeCase):
    """One call of the count hand-off sequence: `messages` one-frame messages
    (0: a 40,000-byte message cut after two of its three DATA frames, so no
    message at all). general: one more DATA frame without END_STREAM that
    overflows a pool sized for the messages alone -- the general form, the
    same message count."""

    def __init__(self, name, messages, general):
        Case.__init__(self, name)
        self.messages, self.mode, self.styles = messages, "general" if general else "fast", (0, 0)
        self._caps = None
        self.n = len(self.inputs("B")["index"])

    def build(self, variant):
        rng = np.random.default_rng(self.seed(variant))
        m = max(self.messages, 1)
        d = np.zeros(m, dtype=O.DESC_DTYPE)
        d["payload_size"] = rng.choice([0, 7, 126, 1000], m) if self.messages else 40000
        d["payload_off"] = rng.integers(0, PAYLOAD_BYTES - 40000, m).astype(np.uint64)
        d["fin"], d["opcode"] = 1, 2
        d["mask"] = (rng.random(m) < .5).astype(np.uint8)
        d["mask_key"] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32) * d["mask"]
        h2, _ = O.h2_serialize_batch(payload_np(), d, 1, H2_FRAME)
        if not self.messages:
            h2 = h2[:int(O.h2_index(h2)[2])]
        self.closed_bytes = len(h2) - 9 * len(O.h2_index(h2))
        if self.mode == "general":
            tail = HU.frame(HU.T_DATA, 0, 1, bytes(rng.integers(0, 256, 5000, dtype=np.uint8)))
            h2 = np.concatenate([h2, np.frombuffer(tail, np.uint8)])
        h2 = h2.copy()
        return dict(h2=h2, index=O.h2_index(h2), messages=self.messages)

    @property
    def caps(self):
        if self._caps is None:
            i = self.inputs("B")
            pool = self.closed_bytes + 100 if self.mode == "general" else len(i["h2"])
            self._caps = (pool, W.round16(self._oracle("B", pool, None)["total"]) + 64)
        return self._caps


INDEX_CONNS = 300
INDEX_COUNTS = ([0, 1, 5, 63, 64, 65, 100, 0, 200, 3], [100, 65, 0, 2, 130, 64, 1, 70, 0, 90])


class IndexCase(Case):
    """cfws_index_frames_batch / cfws_h2_index_frames_batch over 300
    connections: none to 200 frames each (past the 64 kept starts: the rest
    walk), every seventh stopping on an error, every seventh cut mid-frame."""
    kind = "index"

    def __init__(self, name, h2, with_info=True):
        super().__init__(name)
        self.h2, self.with_info, self.n, self.styles = h2, with_info, INDEX_CONNS, (0, 1)
        self._cap = None

    def _conn(self, c, k, rng, nprng):
        if self.h2:
            blob = HU.random_buffer(nprng, k, max_payload=12)
            if c % 7 == 3:
                blob += HU.frame(12, 0, 1, b"abc") + HU.random_buffer(nprng, 2, max_payload=12)   # type > 9: ERROR
            if c % 7 == 5:
                blob += HU.frame(HU.T_DATA, 0, 1, rng.randbytes(20))[:rng.choice([1, 8, 9, 15])]
            return blob
        mk = lambda: O.serialize_keyed(True, rng.choice([1, 2, 9]), rng.random() < .7, rng.getrandbits(32),
                                       rng.randbytes(rng.randrange(0, 20)))
        blob = b"".join(mk() for _ in range(k))
        if c % 7 == 3:
            blob += b"\xf2\x00" + mk() + mk()                                                     # RSV bits: INVALID
        if c % 7 == 5:
            blob += rng.choice([b"\x82", b"\x82\xfe\x01"])
        return blob

    def build(self, variant):
        a = VARIANTS[variant][0]
        rng, nprng = random.Random(self.seed(variant)), np.random.default_rng(self.seed(variant))
        counts = INDEX_COUNTS[a]
        parts, begin, end, at = [b"\xee" * 5], [], [], 5
        for c in range(self.n):
            blob = self._conn(c, counts[c % len(counts)], rng, nprng)
            begin.append(at)
            end.append(at + len(blob))
            gap = b"\xee" * rng.randrange(0, 13)
            parts += [blob, gap]
            at += len(blob) + len(gap)
        arena = np.frombuffer(b"".join(parts) + b"\0" * 16, np.uint8).copy()
        return dict(arena=arena, begin=np.array(begin, np.int64), end=np.array(end, np.int64))

    def oracle(self, variant):
        i = self.inputs(variant)
        S, I, cons, stop = [], [], [], []
        for b, e in zip(i["begin"], i["end"]):
            if self.h2:
                s, info, c, st = HU.expect_h2_index(i["arena"], int(b), int(e), 16384, HU.ALL, 0)
                I.append(info)
            else:
                s, c, st = O.index_stream(i["arena"], int(b), int(e))
            S.append(np.asarray(s, np.uint64))
            cons.append(c)
            stop.append(st)
        counts = np.array([len(s) for s in S], np.int64)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        return dict(starts=np.concatenate(S).view(np.int64), info=np.concatenate(I) if self.h2 else None,
                    first=first, consumed=np.array(cons, np.int64), stop=np.array(stop, np.int32),
                    counts=counts, total=int(counts.sum()))

    @property
    def cap(self):                     # B's starts and three more; A has more frames than that
        if self._cap is None:
            self._cap = self.expect("B")["total"] + 3
        return self._cap

    def ws_bytes(self):
        L = cfws.lib()
        return (L.cfws_h2_index_workspace_size if self.h2 else L.cfws_index_workspace_size)(self.n)

    def alloc(self):
        torch = _torch()
        n = self.n
        return dict(starts=torch.empty(self.cap, dtype=torch.int64, device="cuda"),
                    info=torch.empty((self.cap, 16), dtype=torch.uint8, device="cuda"),
                    first=torch.empty(n, dtype=torch.int64, device="cuda"),
                    consumed=torch.empty(n, dtype=torch.int64, device="cuda"),
                    stop=torch.empty(n, dtype=torch.int32, device="cuda"),
                    total=torch.empty(1, dtype=torch.int64, device="cuda"))

    def upload(self, variant):
        i = self.inputs(variant)
        return dict(arena=_up(i["arena"]), begin=_up(i["begin"]), end=_up(i["end"]))

    def upload_expect(self, variant):
        e = self.expect(variant)
        w = min(self.cap, e["total"])
        dv = dict(starts=_up(e["starts"][:w]), first=_up(e["first"]), consumed=_up(e["consumed"]),
                  stop=_up(e["stop"]))
        if self.h2:
            dv["info"] = _up(e["info"][:w].view(np.uint8).reshape(-1, 16))
        return dv

    def load(self, variant, arena):
        self._v = variant
        for t in self.arenas().values():
            t.fill_(-1 if t.dtype != _torch().uint8 else 0xFF)

    def launch(self, ws, stream=None):
        ar, dv = self.arenas(), self.dev(self._v)
        kw = dict(starts_t=ar["starts"], ws_t=ws, stream=stream, first_t=ar["first"], consumed_t=ar["consumed"],
                  stop_t=ar["stop"], total_t=ar["total"])
        if self.h2:
            cfws.h2_index_frames_batch(dv["arena"], dv["begin"], dv["end"], 16384, HU.ALL, 0,
                                       info_t=ar["info"] if self.with_info else None, with_info=self.with_info, **kw)
        else:
            cfws.index_frames_batch(dv["arena"], dv["begin"], dv["end"], **kw)

    def check(self, variant, arena):
        ar, e, dv = self.arenas(), self.expect(variant), self.devx(variant)
        total = int(ar["total"].item())
        assert total == e["total"], (self.name, variant, total, e["total"])
        _eq(ar["first"], dv["first"], f"{self.name}/{variant} first")
        _eq(ar["consumed"], dv["consumed"], f"{self.name}/{variant} consumed")
        _eq(ar["stop"], dv["stop"], f"{self.name}/{variant} stop")
        w = min(self.cap, total)
        _eq(ar["starts"][:w], dv["starts"], f"{self.name}/{variant} starts")
        _all(ar["starts"][w:], -1, f"{self.name}/{variant} starts past the total")
        if self.h2 and self.with_info:
            _eq(ar["info"][:w], dv["info"], f"{self.name}/{variant} info")
            _all(ar["info"][w:], 0xFF, f"{self.name}/{variant} info past the total")
        else:
            _all(ar["info"], 0xFF, f"{self.name}/{variant} info without d_info")

    def outputs(self, variant):
        ar = self.arenas()
        return [ar["starts"], ar["info"], ar["first"], ar["consumed"], ar["stop"], ar["total"]]


KEY_SENT = -286331154                  # 0xEEEEEEEE


class KeysCase(Case):
    """cfws_draw_mask_keys_device with mask flags (the form with a workspace)
    against the host draw."""
    kind = "keys"
    FIRST = 1000003

    def __init__(self, name, n):
        super().__init__(name)
        self.n, self.styles = n, (0.3, 0.9)

    def build(self, variant):
        rng = np.random.default_rng(self.seed(variant))
        return (rng.random(self.n) < self.style(variant)).astype(np.uint8)

    def oracle(self, variant):
        keys, nxt = cfws.draw_mask_keys_at(self.n, self.inputs(variant), 1234, self.FIRST)
        return dict(keys=keys, next=nxt)

    def ws_bytes(self):
        return cfws.draw_keys_workspace_size(self.n)

    def alloc(self):
        torch = _torch()
        return dict(keys=torch.empty(self.n + 64, dtype=torch.int32, device="cuda"),
                    next=torch.empty(1, dtype=torch.int64, device="cuda"))

    def upload(self, variant):
        f = np.full(max(W.round16(self.n), 16), 0xEE, np.uint8)         # the padding non-zero
        f[:self.n] = self.inputs(variant)
        return dict(flags=_up(f))

    def upload_expect(self, variant):
        return dict(keys=_up(self.expect(variant)["keys"].view(np.int32)))

    def load(self, variant, arena):
        self._v = variant
        self.arenas()["keys"].fill_(KEY_SENT)
        self.arenas()["next"].fill_(-1)

    def launch(self, ws, stream=None):
        ar = self.arenas()
        cfws.draw_mask_keys_device(self.n, self.dev(self._v)["flags"], 1234, self.FIRST, ar["keys"], ar["next"], ws,
                                   stream=stream)

    def check(self, variant, arena):
        ar = self.arenas()
        _eq(ar["keys"][:self.n], self.devx(variant)["keys"], f"{self.name}/{variant} keys")
        _all(ar["keys"][self.n:], KEY_SENT, f"{self.name}/{variant} past 4 n bytes")
        assert int(ar["next"].item()) == self.expect(variant)["next"]

    def outputs(self, variant):
        return list(self.arenas().values())


# ---- the registry -----------------------------------------------------------------

def _make_cases():
    cs = []
    small = 4 << 20
    cs.append(SerCase("ser_small", 1000, ("small_lo", "small_hi"), cap=small))
    for pe in (False, True):
        s = "_pe" if pe else ""
        cs += [SerCase("ser_mixed" + s, 3000, ("mixed", "inreg_hi"), pe),
               SerCase("ser_inreg_clear" + s, 3000, ("inreg", "odd_big"), pe),
               SerCase("ser_inreg_set" + s, 3000, ("inreg_one_bad", "inreg_hi"), pe),
               SerCase("ser_single_tiny" + s, BIG_N, ("tiny", "inreg_small"), pe),
               SerCase("ser_single_inreg" + s, BIG_N, ("inreg_small", "odd_mid"), pe)]
    cs.append(SerCase("ser_one", 1, ("inreg", "odd_big")))
    for cut in (False, True):
        s = "_cut" if cut else ""
        cs += [DeCase("de_small" + s, 1000, ((0, 2000), (2100, 3400)), 16, cut=cut),
               DeCase("de_fused_2049_a16" + s, 2049, ((0, 300), (200, 480)), 16, cut=cut),
               DeCase("de_fused_133121_a16" + s, 133_121, ((0, 300), (200, 480)), 16, cut=cut),
               DeCase("de_fused_133121_a64" + s, 133_121, ((0, 300), (200, 480)), 64, cut=cut),
               DeCase("de_plan_3000_a1" + s, 3000, ((0, 3000), (3100, 6000)), 1, cut=cut),
               DeCase("de_plan_3000_a1_pe" + s, 3000, ((0, 3000), (3100, 6000)), 1, cut=cut, pe=True),
               DeCase("de_single_a1" + s, BIG_N, ((0, 40), (41, 100)), 1, cut=cut),
               DeCase("de_single_a1_pe" + s, BIG_N, ((0, 40), (41, 100)), 1, cut=cut, pe=True),
               DeCase("de_reasm_3000" + s, 3000, ((0, 3000), (3100, 6000)), 16, flags=cfws.DESERIALIZE_REASSEMBLE,
                      cut=cut)]
    for n, ranges in ((3000, ((0, 1500), (1600, 4000))), (BIG_N, ((0, 40), (41, 100)))):
        for policy, pname in ((RU.VERBATIM, "verbatim"), (RU.ECHO_SERVER, "echo")):
            for out_mask in (0, 1):
                cs.append(RelayCase(f"relay_{n}_{pname}_{'mask' if out_mask else 'plain'}", n, ranges, policy,
                                    out_mask))
    big, little = [0, 1, 125, 126, 999, 1000, 16376, 16384, 40000], [0, 1, 5, 40, 125, 126, 999]
    cs += [H2SerCase("h2ser_S16384", 2000, 16384, (big, [50000, 60000])),
           H2SerCase("h2ser_S100", 2000, 100, (little, [1500, 3000])),
           H2SerCase("h2ser_S16", 2000, 16, (little, [1500, 3000]))]
    cs += [H2DeCase("h2de_fast", "fast", ("one", "two")),
           H2DeCase("h2de_general", "general", ("one", "two")),
           H2DeCase("h2de_open", "open", ("mix_open", "one_big"))]
    cs += [IndexCase("index_ws", False), IndexCase("index_h2_info", True, True),
           IndexCase("index_h2_noinfo", True, False)]
    cs += [KeysCase("keys_24581", 24581), KeysCase("keys_scan_launch", 2048 * 4096 + 4097)]
    return {c.name: c for c in cs}


_cases = None


def cases() -> dict:
    global _cases
    if _cases is None:
        _cases = _make_cases()
    return _cases


CASE_NAMES = sorted(cases())

# the shapes cfws.Graph replays, route by route. Not among them: the fused
# receive (de_fused_133121_a16) and the single-pass receive plan (de_single_a1).
# A replay of either graph over a 0xAA workspace ended in a memory-access fault
# on the MI355X (deserialize_plan_single_kernel<true> and <false>; the same
# calls outside a graph pass every pattern, and so do the send's single-pass
# graphs); the cause is not found, so they stay out until it is.
GRAPH_CASES = ["ser_small", "ser_mixed", "ser_single_tiny", "ser_single_inreg",
               "de_small", "de_plan_3000_a1", "de_reasm_3000"]

# one long-lived workspace: every entry point in turn, n up and down
SEQUENCE = [("ser_single_tiny", "B"), ("de_small", "B"), ("relay_3000_echo_mask", "B"),
            ("de_fused_133121_a16", "B"), ("ser_one", "B"), ("h2de_general", "B"), ("index_ws", "B"),
            ("h2ser_S16", "B"), ("de_single_a1", "B"), ("index_h2_info", "B"), ("keys_24581", "B"),
            ("de_reasm_3000", "B"), ("ser_inreg_clear_pe", "B"), (f"relay_{BIG_N}_verbatim_plain", "B"),
            ("de_plan_3000_a1_pe_cut", "B"), ("h2de_fast", "B"), ("ser_small", "B"), ("h2ser_S16384", "B"),
            ("de_fused_2049_a16_cut", "B"), ("ser_single_inreg", "B"), ("h2de_open", "B"),
            ("ser_inreg_set", "B"), ("de_single_a1_cut", "B"), ("ser_one", "A")]


# ---- the runs ---------------------------------------------------------------------

def fill_pattern(ws, pattern: str) -> None:
    ws.fill_(int(pattern, 16))


def run_dirty(case: Case, patterns=PATTERNS) -> None:
    """Section 1: the call over a workspace holding each pattern; every
    documented output equals the oracle's and the 0x00 run's."""
    torch = _torch()
    ws = torch.empty(case.ws_bytes(), dtype=torch.uint8, device="cuda")
    ref = None
    for p in patterns:
        if p == "prev":
            ws.zero_()
            case.run("A", ws, check=False)             # leaves its state behind
        else:
            fill_pattern(ws, p)
        case.run("B", ws)
        got = case.outputs("B")
        if ref is None:
            ref = [t.clone() for t in got]
        else:
            for k, (g, r) in enumerate(zip(got, ref)):
                _eq(g, r, f"{case.name}: output {k} after a workspace of {p} against the first run")


def run_poisoned(case: Case) -> None:
    """Section 3: a clean workspace, every output prefilled with poison,
    under two arena poisons: every documented entry is overwritten and
    every byte below the reported total is the same in both runs."""
    torch = _torch()
    ws = torch.zeros(case.ws_bytes(), dtype=torch.uint8, device="cuda")
    case.run("B", ws, arena=ARENA)
    ref = [t.clone() for t in case.outputs("B")]
    ws.zero_()
    case.run("B", ws, arena=ARENA2)
    for k, (g, r) in enumerate(zip(case.outputs("B"), ref)):
        _eq(g, r, f"{case.name}: output {k} under the second arena poison")
