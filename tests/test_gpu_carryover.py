"""State that survives from one batch call to the next: every
workspace-taking entry point, on every route, over a workspace and output
arrays that hold something else than a fresh allocation -- a byte pattern,
what the same entry point left there after a different batch, poison -- and
over one workspace and one set of arenas used again and again (a scripted
sequence of calls, replays of captured graphs, the HTTP/2 receive's count
hand-off). A server loop calls the library that way (INTEGRATION.md,
cfws_graph.cpp); DESIGN.md §2.1 is the table of who writes which workspace
region before who reads it, and tests/carryover_util.py holds its cases.
Everything is bit-exact against the oracle.

The patterns: 0xAA makes every 64-bit look-back word of the single-pass
plans read "inclusive prefix published" (low bits 10) with a huge value and
every u32 flag non-zero, 0x55 "sum published"; `prev` is the workspace as a
batch A left it whose total is larger (above the capacity), whose in-region
send decision, invalid and incomplete frames and message count all differ."""
import os
import subprocess
import sys

import numpy as np
import pytest

import carryover_util as U
import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402
from coldforce_amd import workloads as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()
    torch.cuda.synchronize()


# ---- 1. a dirty workspace, every route -----------------------------------------

@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_dirty_workspace(name):
    """The call over a workspace of 0x00, 0xFF, 0xAA, 0x55 and of a previous
    batch's state: each time the outputs equal the oracle's, and every
    documented output array is byte-identical to the first run's."""
    U.run_dirty(U.cases()[name])


# the same under the knobs that move a shape to its other route, one child
# process per setting (the library reads them once)
KNOB_LEGS = [
    ({"CFWS_PLAN_SINGLE": "0"}, ["ser_single", "de_single"]),
    ({"CFWS_FUSED_DESER": "0"}, ["de_fused"]),
    ({"CFWS_SMALL": "0"}, ["ser_small", "ser_one", "de_small"]),
    ({"CFWS_H2_UNITS_MERGED": "0"}, ["h2de"]),
    ({"CFWS_SER_INREG": "0"}, ["ser_inreg", "ser_single_inreg", "ser_mixed"]),
]


@pytest.mark.parametrize("knobs,prefixes", KNOB_LEGS,
                         ids=[",".join(f"{a[5:]}={b}" for a, b in k.items()) for k, _ in KNOB_LEGS])
def test_dirty_workspace_under_knob(knobs, prefixes):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFWS_")}
    env.update(knobs)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "carryover_parity.py")] + prefixes
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"carryover_parity.py {knobs} ran into its time limit: nothing more is started on the GPU\n"
                    f"{(e.stdout or b'')[-2000:]}", returncode=3)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"carryover_parity.py {knobs} died with {r.returncode}: nothing more is started on the GPU\n"
                    f"{r.stdout[-2000:]}{r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0 and "CARRYOVER OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- 2. one long-lived workspace ------------------------------------------------

@pytest.mark.parametrize("order", ["script", "reversed"])
def test_one_workspace_for_every_call(order):
    """One tensor, as large as the largest workspace of the script, filled
    with random bytes once and never cleared, handed to every entry point in
    turn while n goes 524,289 -> 1,000 -> 3,000 -> 133,121 -> 1 -> ...: each
    layout lands on what the layouts before it left. Every call against the
    oracle, in the script's order and in reverse."""
    seq = U.SEQUENCE if order == "script" else U.SEQUENCE[::-1]
    size = max(U.cases()[name].ws_bytes() for name, _ in seq)
    ws = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
    for name, variant in seq:
        U.cases()[name].run(variant, ws)


# ---- 3. poisoned outputs --------------------------------------------------------

@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_poisoned_outputs(name):
    """Every output array prefilled with poison (descriptor bytes 0x5A,
    statuses 0x5A5A5A5A, totals / first / consumed / stop / info -1, the host
    n_messages a sentinel): every documented entry is overwritten, the
    HTTP/2 receive's rows n_messages..n_h2-1 are empty, nothing past a
    capacity is touched; and under a second arena poison every byte below
    the reported total is the same (padding is written)."""
    U.run_poisoned(U.cases()[name])


def test_empty_calls_write_their_totals():
    """n == 0: each entry point still writes its total (the plans'
    zero_totals, the HTTP/2 calls, the indexers, the slot receives), and the
    HTTP/2 receive its message count."""
    dev = "cuda"
    total = lambda: torch.full((1,), -1, dtype=torch.int64, device=dev)
    some = torch.zeros(64, dtype=torch.uint8, device=dev)
    desc0 = torch.empty((0, 32), dtype=torch.uint8, device=dev)
    desc1 = torch.full((1, 32), 0x5A, dtype=torch.uint8, device=dev)
    st1 = torch.full((1,), U.STATUS_POISON, dtype=torch.int32, device=dev)
    idx0 = torch.empty(0, dtype=torch.int64, device=dev)
    out = torch.full((64,), U.ARENA, dtype=torch.uint8, device=dev)
    got = {}
    ws = torch.full((cfws.lib().cfws_workspace_size(0, 64),), 0xAA, dtype=torch.uint8, device=dev)
    t = total()
    cfws.serialize_plan(desc0, 64, t, ws)
    got["serialize_plan"] = t
    got["serialize_batch"] = cfws.serialize(some, desc0, out, ws, total())
    t = total()
    cfws.deserialize_plan(some, 64, idx0, desc1, st1, 64, t, ws)
    got["deserialize_plan"] = t
    got["deserialize_batch"] = cfws.deserialize(some, 64, idx0, out, desc1, st1, ws, total())[2]
    rws = torch.full((cfws.lib().cfws_relay_workspace_size(0, 64),), 0xAA, dtype=torch.uint8, device=dev)
    got["relay_batch"] = cfws.relay(some, 64, idx0, out, desc_t=desc1, status_t=st1, ws_t=rws, total_t=total())[2]
    got["h2_serialize_batch"] = cfws.h2_serialize(some, desc0, some, out, total_t=total())
    *_, t, m = cfws.h2_deserialize(some, 64, idx0, some, out, total_t=total(), n_messages_init=U.COUNT_SENTINEL)
    got["h2_deserialize_batch"] = t
    assert m == 0
    first = torch.full((1,), -1, dtype=torch.int64, device=dev)
    t = total()
    assert cfws.index_frames_batch(some, idx0, idx0, starts_t=first.clone(), first_t=first, total_t=t)[4] == 0
    got["index_frames_batch"] = t
    t = total()
    assert cfws.h2_index_frames_batch(some, idx0, idx0, starts_t=first.clone(), first_t=first, total_t=t)[5] == 0
    got["h2_index_frames_batch"] = t
    got["deserialize_slots"] = cfws.deserialize_slots(some, 64, idx0, out, 16, desc1, st1, total())[2]
    info1 = torch.full((1, 8), 0x5A, dtype=torch.uint8, device=dev)
    got["deserialize_slots_info"] = cfws.deserialize_slots_info(some, 64, idx0, out, 16, info1, total())[1]
    mm = torch.full((1,), -1, dtype=torch.int32, device=dev)
    got["deserialize_slots_uniform"] = cfws.deserialize_slots_uniform(some, 64, 0, 20, out, 16, info1, total(), mm)[1]
    torch.cuda.synchronize()
    for name, t in got.items():
        assert int(t.item()) == 0, name
    assert int(mm.item()) == 0
    # nothing else was written
    assert bool((desc1 == 0x5A).all()) and bool((st1 == U.STATUS_POISON).all()) and bool((out == U.ARENA).all())
    assert bool((first == -1).all()) and bool((info1 == 0x5A).all())


def test_mismatch_counter_starts_from_zero_each_call():
    """cfws_deserialize_slots_uniform's *d_mismatch: the same counter word
    for a stream with 10 odd frames, then one with 3, prefilled with -1 --
    each call reports its own count."""
    n, fs = 3000, 256
    desc = W.uniform_batch(n, fs, 5)
    payload = O.fill_splitmix(n * fs, 5, 0)
    wire, _ = O.serialize_batch(payload, desc.view(O.DESC_DTYPE))
    stride = cfws.uniform_frame_bytes(fs, True)
    w = torch.from_numpy(np.concatenate([wire, np.zeros(32, np.uint8)])).cuda()
    out = torch.empty(n * fs, dtype=torch.uint8, device="cuda")
    info = torch.empty((n, 8), dtype=torch.uint8, device="cuda")
    mm = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    for lost in (10, 3, 0, 10):
        cut = (n - lost) * stride + (1 if lost else 0)          # the last `lost` frames: MORE_DATA
        cfws.deserialize_slots_uniform(w, cut, n, stride, out, fs, info, tot, mm)
        torch.cuda.synchronize()
        assert int(mm.item()) == lost
        st = cfws.info_from_device(info)["status"]
        assert (st[:n - lost] == 0).all() and (st[n - lost:] == O.PARSE_MORE_DATA).all()
        assert torch.equal(out[:(n - lost) * fs], torch.from_numpy(payload[:(n - lost) * fs]).cuda())


# ---- 4. graph replays, route by route -------------------------------------------

@pytest.mark.parametrize("name", U.GRAPH_CASES)
def test_graph_replays_flip_every_decision(name):
    """cfws.Graph.serialize / deserialize captured at the case's shape (a
    single-stream chain, over a workspace of 0xAA) and replayed four times
    with contents A, B, A', C written into the same arenas between launches:
    consecutive replays flip the total against the capacity, the in-region
    decision, where the invalid and incomplete frames sit. The third replay
    runs on a side stream. Each against the oracle. (Send: small, reduce /
    apply, single-pass; receive: small, plan + execute, reassembly. The
    receive's single-pass kernels are left out: carryover_util.GRAPH_CASES.)"""
    case = U.cases()[name]
    ws = torch.full((case.ws_bytes(),), 0xAA, dtype=torch.uint8, device="cuda")
    case.arenas()
    g = case.capture(ws)
    side = torch.cuda.Stream()
    try:
        for k, variant in enumerate(("A", "B", "A2", "C")):
            case.load(variant, U.ARENA)
            torch.cuda.synchronize()
            if k == 2:
                g.launch(stream=side)
                side.synchronize()
            else:
                g.launch()
                torch.cuda.synchronize()
            case.check(variant, U.ARENA)
    finally:
        g.close()


# ---- 5. the HTTP/2 receive's count hand-off -------------------------------------

def test_h2_count_handoff_call_after_call():
    """Six consecutive cfws_h2_deserialize_batch calls on one thread, whose
    message counts are 7, 3,000, 0 (an unterminated stream), 7, 1 and 2,999,
    alternating between the fast and the general form and between two
    streams, over one workspace that is never cleared: each call reports its
    own n_messages (the thread's mapped count words are shared by all of
    them), statuses and payloads. Then again after a call that returns an
    argument error."""
    calls = [U.H2CountCase(f"handoff_{k}", m, general)
             for k, (m, general) in enumerate([(7, False), (3000, True), (0, False), (7, True), (1, False),
                                               (2999, True)])]
    for c in calls:
        assert c.expect("B")["n_msg"] == c.messages, (c.name, c.expect("B")["n_msg"])
        assert ((c.expect("B")["h2_status"] == O.ERROR_OUT_OF_MEMORY).any()) == (c.mode == "general"), c.name
    ws = torch.randint(0, 256, (max(c.ws_bytes() for c in calls),), dtype=torch.uint8, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def six():
        for k, c in enumerate(calls):
            c.run("B", ws, stream=streams[k % 2])
    six()
    c = calls[1]
    with pytest.raises(cfws.CodecError):                   # align 3: refused before anything is queued
        cfws.h2_deserialize(c.dev("B")["h2"], len(c.inputs("B")["h2"]), c.dev("B")["index"],
                            c.arenas()["pool"], c.arenas()["pay"], align=3, ws_t=ws)
    six()
