"""bench.py --dump-outputs and --full: a plain run times its steps and, when
asked, writes what the last timed step produced (the same arrays on every run
with the same arguments); the check of what was timed, the copy ceiling and
the CPU baseline belong to --full."""
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_small_arrays_whole(bench, tmp_path):
    """Under its share of the budget an array is written whole: bytes as
    float32, 32- and 64-bit integers as float64, value for value."""
    outs = {"bytes": torch.arange(1000, dtype=torch.int64).to(torch.uint8).view(10, 100),
            "codes": torch.tensor([0, -3, 1 << 30], dtype=torch.int32),
            "total": torch.tensor([(1 << 40) + 1], dtype=torch.int64)}
    bench.dump_outputs(str(tmp_path), outs)
    got = _load(tmp_path)
    assert sorted(got) == ["bytes", "codes", "total"]
    assert got["bytes"].dtype == np.float32 and got["codes"].dtype == got["total"].dtype == np.float64
    assert np.array_equal(got["bytes"], np.arange(1000) % 256)
    assert got["codes"].tolist() == [0, -3, 1 << 30] and got["total"].tolist() == [(1 << 40) + 1]


def test_dump_large_array_is_a_fixed_sample(bench, tmp_path):
    """Past its share an array is sampled in DUMP_BLOCK runs at seeded places:
    the same elements on every call, each run contiguous in the source, and
    the files stay under 64 MB in all."""
    n = 12_000_000
    big = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    outs = {"a": big, "b": big[: n // 2], "c": torch.arange(5, dtype=torch.int64)}
    bench.dump_outputs(str(tmp_path / "x"), outs)
    bench.dump_outputs(str(tmp_path / "y"), outs)
    x, y = _load(tmp_path / "x"), _load(tmp_path / "y")
    assert all(np.array_equal(x[k], y[k]) for k in outs)
    assert x["c"].tolist() == [0, 1, 2, 3, 4]
    size = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert size <= 64_000_000
    B = bench.DUMP_BLOCK
    a = x["a"].reshape(-1, B)
    assert a.shape[0] > 1 and x["a"].size * 4 <= bench.DUMP_BUDGET // 3
    src = big.numpy()
    # every sampled run is a run of the source at a multiple of the block, in ascending order
    starts = []
    for row in a[:: max(1, a.shape[0] // 16)]:
        hits = [s for s in range(0, n - B + 1, B) if src[s] == row[0] and np.array_equal(src[s:s + B], row)]
        assert hits
        starts.append(hits[0])
    assert starts == sorted(starts)


def _run(bench, monkeypatch, capsys, argv):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "CFWS_BENCH_LAUNCHER"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("F,fs", [(64, 1000), (96, 65536)])
def test_plain_run_dumps_the_last_step(bench, monkeypatch, capsys, tmp_path, F, fs):
    """A plain run: --steps timed steps, ms_per_step in the line, nothing of
    --full; its dump equals the oracle's wire and payload for the bench's
    seeded inputs (whole at 64 x 1000 B, where the packed receive pads each
    payload to 16; sampled at 96 x 64 KiB) and is the same on a second run."""
    import oracle as O
    from coldforce_amd import shard
    from coldforce_amd import workloads as W
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", str(F), "--frame-size", str(fs)]
    line = _run(bench, monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["verified"] is None and line["copy_ceiling"] is None and line["cpu_baseline"] is None
    _run(bench, monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) == ["frame_desc", "frame_status", "payload", "payload_total", "wire",
                                      "wire_total"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)

    desc, base = shard.uniform_shard(F, fs, bench.KEY_SEED, 0, 1)
    payload = O.fill_splitmix(F * fs, bench.PAYLOAD_SEED, base)
    wire, _ = O.serialize_batch(payload, desc.view(O.DESC_DTYPE))
    assert a["wire_total"].tolist() == [len(wire)] and a["payload_total"].tolist() == [F * W.round16(fs)]
    assert not a["frame_status"].any() and a["frame_status"].size == F
    if F * fs * 4 <= bench.DUMP_BUDGET // 6:
        assert np.array_equal(a["wire"], wire) and np.array_equal(a["payload"], payload)
    else:
        B = bench.DUMP_BLOCK
        assert a["payload"].size % B == 0 and 0 < a["payload"].size * 4 <= bench.DUMP_BUDGET // 6
        for got, exp in ((a["wire"], wire), (a["payload"], payload)):
            rows = got.reshape(-1, B)
            blocks = exp[: len(exp) // B * B].reshape(-1, B)
            at = {bytes(r[:16]): i for i, r in enumerate(blocks)}
            for r in rows[:: max(1, len(rows) // 32)]:
                assert np.array_equal(blocks[at[bytes(r[:16].astype(np.uint8))]], r)


@pytest.mark.gpu
def test_full_run_checks_and_measures_the_rest(bench, monkeypatch, capsys):
    line = _run(bench, monkeypatch, capsys, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "64",
                                             "--frame-size", "4096", "--full", "--no-cpu-baseline"])
    assert line["verified"] is True and line["copy_ceiling"]["GBps"] > 0
    assert line["cpu_baseline"] is None and line["ms_per_step"] > 0
