"""The host-memory pipeline's chunk cuts (coldforce_amd/csrc/cfws_chunks.h;
DESIGN.md §6): the send cut, the receive cut and the HTTP/2 receive cut, as
cfws_pipeline.cpp applies them.

tests/native/chunks_test.cpp checks them by the properties that define them
uniquely (the chunks tile the batch in order, each obeys every limit, each is
maximal, a single frame or message over a limit is the error) on fixed cases
at the smallest chunk and on seeded random batches, built with
-fsanitize=address,undefined into a stand-alone program over exact-size heap
arrays. The pipeline's results through these cuts: tests/test_gpu_pipeline.py.
"""
import os
import subprocess

from conftest import ROOT


def test_sanitized_cuts_tile_obey_and_are_maximal():
    mk = subprocess.run(["make", "-s", "-C", ROOT, "build/chunks_test"], capture_output=True, text=True)
    assert mk.returncode == 0, mk.stdout + mk.stderr
    r = subprocess.run([os.path.join(ROOT, "build", "chunks_test")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    seen = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        seen[w[0]] = dict(zip(w[1::2], map(int, w[2::2])))
    assert set(seen) == {"send", "h2_send", "recv", "h2_recv"}
    # the run was not vacuous: a few thousand batches per direction, chunks of
    # several frames and error returns under every cut
    assert seen["send"]["batches"] + seen["h2_send"]["batches"] >= 6000
    assert seen["recv"]["batches"] >= 3000 and seen["h2_recv"]["batches"] >= 3000
    for cut, s in seen.items():
        assert s["chunks"] >= 2 * s["batches"] and s["multi"] >= 1000 and s["errors"] >= 100, (cut, s)
