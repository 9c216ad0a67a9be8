"""Batch entry points with one offset operand across 2^32 (-m gpu).

Almost every other GPU test runs in arenas of a few megabytes, where the
upper 32 bits of every offset, product, difference, shuffle and cast are
zero. Here each case of tests/wide_util.py runs one entry point so that the
operand its name carries has frames wholly below 2^32, wholly at or above it
and one across it: offsets the caller supplies by relocating a small problem
into a 2^32 + 4 MiB arena (the library gets the arena's own base pointer),
offsets the library derives by a ballast frame or by n * slot passing the
mark. Every output the call defines is compared bit for bit with the
existing oracles, every arena is then checked whole for stray writes, and the
route is the one the library's reporters name (tests/test_wide_cases.py, the
CPU half, proves the crossing and the route of every case without a device).

A test holds up to 24 GiB of device memory, runs alone and frees its tensors
before it returns; the module skips on a device with less than 32 GiB free.
"""
import pytest

import wide_util as U
from conftest import gpu_present

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_present(), reason="needs the MI355X")]

torch = pytest.importorskip("torch")

from coldforce_amd import cfws  # noqa: E402

NEED_FREE = 32 << 30


@pytest.fixture(scope="module", autouse=True)
def device():
    cfws.init()
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"{free >> 30} GiB of device memory free, the cases need {NEED_FREE >> 30}")
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


FAULTED = []          # a case whose call ended in a HIP error: nothing more runs on the device after it


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_wide(name):
    assert not FAULTED, f"not run: {FAULTED[0]} ended in a HIP error"
    case = U.cases()[name]
    try:
        assert case.device_bytes() <= U.BUDGET
        case.run()
    except AssertionError:
        raise
    except Exception as e:
        if any(s in str(e) for s in ("HIP error", "hipError", "illegal memory", "rc=-3")):
            FAULTED.append(name)
        raise
    finally:
        case.release()
        if not FAULTED:
            torch.cuda.synchronize()
